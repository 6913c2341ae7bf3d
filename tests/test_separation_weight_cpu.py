"""The separation weight without a GPU: the numpy reference (tests/separation_ref.py) on hand-computed rasters, the table, the model
config keys and ``rs train``'s refusals, the modules' new argument, the new entry points."""

import argparse
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import separation_ref as S  # noqa: E402

from robosat_amd import ops  # noqa: E402
from robosat_amd.config import load_config, save_config, separation_options  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference on hand-computed rasters ---------------------------------------------------------------------------------------
def test_two_pixels_three_apart_in_a_row():
    """1 0 0 2: either middle pixel is 1 from one object and 2 from the other: a = 1, b = 4, s2 = 1 + 4 + isqrt(16) = 9 = (1 + 2)^2."""

    row = np.array([[1, 0, 0, 2]])
    a, b = S.nearest_two(row, 3)
    assert a.tolist() == [[S.FAR, 1, 1, S.FAR]] and b.tolist() == [[S.FAR, 4, 4, S.FAR]]
    assert S.s2_of(a, b).tolist() == [[S.FAR, 9, 9, S.FAR]]
    tab = S.table(10.0, 1.5)  # reach 5: 9 < 25
    assert S.term(row, 10.0, 1.5, 3).tolist() == [[0.0, float(tab[9]), float(tab[9]), 0.0]]
    assert S.plane(row[None], 10.0, 1.5, 3)[0].tolist() == [[1.0, float(np.float32(1) + tab[9]), float(np.float32(1) + tab[9]), 1.0]]
    assert S.term(row, 10.0, 1.0, 3).tolist() == [[0.0] * 4]  # reach 3: s2 = 9 sits AT the cap
    assert S.plane(row.T[None], 10.0, 1.5, 3)[0].T.tolist() == S.plane(row[None], 10.0, 1.5, 3)[0].tolist()
    # the floor in s2: a = 1, b = 2 (a diagonal neighbour) gives 3 + isqrt(8) = 5 = floor((1 + sqrt 2)^2 = 5.83)
    t = np.array([[1, 0, 0], [0, 0, 2]])
    a, b = S.nearest_two(t, 3)
    assert (a[0, 1], b[0, 1], S.s2_of(a, b)[0, 1]) == (1, 2, 5)


def test_a_courtyard_and_a_lone_object_weigh_nothing():
    u = S.rectangles(12, 12, [(2, 9, 2, 9, 1), (2, 7, 5, 6, 0)])  # a U: the courtyard is two columns wide and open at the top
    assert int(S.objects(u > 0).max()) == 1 and S.exercised(u, 5, 3)["same"] > 0
    assert not S.term(u, 10.0, 5, 3).any()
    assert (S.plane(u[None], 10.0, 5, 3) == 1).all()
    assert not S.term(S.rectangles(9, 9, [(3, 5, 3, 5, 2)]), 10.0, 10.6, 3).any()
    assert not S.term(np.zeros((4, 5), dtype=np.int64), 10.0, 5, 3).any()
    # cut the U's base and it is two objects: the same courtyard now counts
    two = u.copy()
    two[8:10, 5:7] = 0
    assert int(S.objects(two > 0).max()) == 2 and S.term(two, 10.0, 5, 3)[4, 5] > 0


def test_classes_ignore_and_images():
    t = np.array([[1, 2, 0, 0, 1]])  # 1 and 2 touch: one object
    assert S.objects(S.classes_of(t, 3)[0]).tolist() == [[1, 1, 0, 0, 2]]
    assert S.nearest_two(t, 3)[0].tolist() == [[S.FAR, S.FAR, 1, 1, S.FAR]]
    assert S.classes_of(t, 2)[0].tolist() == [[True, False, False, False, True]]  # with 2 classes the label 2 is no object
    band = np.array([[1, 0, 255, 0, 2]])
    a, b = S.nearest_two(band, 3, ignore=255)
    assert a.tolist() == [[S.FAR, 1, S.FAR, 1, S.FAR]] and b.tolist() == [[S.FAR, 9, S.FAR, 9, S.FAR]]  # the distance passes over the band
    p = S.plane(band[None], 10.0, 5, 3, ignore=255)[0]
    assert p[0, 2] == 0 and p[0, 1] > 1 and p[0, 0] == 1
    base = torch.full((1, 1, 5), 0.25)
    assert S.plane(band[None], 10.0, 5, 3, ignore=255, base=base)[0, 0].tolist()[::2] == [0.25, 0.25, 0.25]
    two = np.stack([np.array([[1, 0, 0, 0]]), np.array([[0, 0, 0, 2]])])  # images never see each other
    assert (S.plane(two, 10.0, 5, 3) == 1).all()


@pytest.mark.parametrize("h, w", [(65, 65), (64, 130), (130, 63)])
def test_the_standard_raster_puts_every_case_to_the_test(h, w):
    for sigma in (1.5, 5, 10.6):
        seen = S.exercised(S.standard_raster(h, w, True), sigma, 3, S.IGNORE)
        assert min(seen.values()) > 0, (sigma, seen)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws, sigma", [(10.0, 5.0), (4.0, 1.5), (0.5, 10.6), (1e-3, 0.2), (10, 10 + 2 / 3)])
def test_the_table_is_float32_non_increasing_and_as_long_as_the_reach_squared(ws, sigma):
    tab = S.table(ws, sigma)
    d = S.reach(sigma)
    assert tab.dtype == np.float32 and tab.shape == (d * d,) and 1 <= d <= 32
    assert (np.diff(tab) <= 0).all() and (tab >= 0).all()
    assert float(tab[0]) == float(np.float32(ws))
    assert float(tab[-1]) == float(np.float32(ws * math.exp(-(d * d - 1) / (2.0 * sigma * sigma))))
    mine = ops.separation_table(ws, sigma)  # the package's table is the same bits
    assert mine.dtype == np.float32 and mine.tobytes() == tab.tobytes()
    assert ops.separation_reach(ws, sigma) == d


def test_the_reach_is_refused_beyond_32():
    assert ops.SEPARATION_MAX_REACH == 32 and ops.separation_reach(10.0, 5.0) == 15
    assert ops.separation_reach(1, 32 / 3) == 32
    for ws, sigma in ((10.0, 10.7), (0.0, 5.0), (-1.0, 5.0), (10.0, 0.0), (float("nan"), 5.0), (10.0, float("inf")), (True, 5.0), ("1", 5.0)):
        with pytest.raises(ValueError):
            ops.separation_reach(ws, sigma)
        with pytest.raises(ValueError):
            ops.separation_table(ws, sigma)


# ---- the model config keys and rs train's refusals ----------------------------------------------------------------------------------
def _model(loss="CrossEntropy", **opt):
    return {"common": {"cuda": True, "batch_size": 2, "image_size": 64, "checkpoint": "/nowhere"},
            "opt": dict({"epochs": 1, "lr": 1e-4, "loss": loss}, **opt)}


def _dataset(classes=("background", "parking")):
    return {"common": {"dataset": "/nowhere", "classes": list(classes), "colors": ["denim", "orange"][:len(classes)]},
            "weights": {"values": [1.0, 2.0][:len(classes)]}}


REFUSALS = [
    ({"separation_weight": "10"}, "separation_weight"), ({"separation_weight": True}, "separation_weight"),
    ({"separation_weight": float("inf")}, "separation_weight"), ({"separation_weight": float("nan")}, "separation_weight"),
    ({"separation_weight": 0}, "separation_weight"), ({"separation_weight": -1.0}, "separation_weight"),
    ({"separation_weight": 10.0, "separation_sigma": "5"}, "separation_sigma"),
    ({"separation_weight": 10.0, "separation_sigma": 0.0}, "separation_sigma"),
    ({"separation_weight": 10.0, "separation_sigma": float("inf")}, "separation_sigma"),
    ({"separation_weight": 10.0, "separation_sigma": -2.0}, "separation_sigma"),
    ({"separation_weight": 10.0, "separation_sigma": 10.7}, "separation_sigma"),  # ceil(32.1) = 33
    ({"separation_sigma": 5.0}, "separation_sigma"),
]
OTHER_LOSSES = ("mIoU", "Lovasz", "LovaszSoftmax", "Tversky")


def test_the_config_keys():
    assert separation_options(_model()) is None and separation_options(_model(), _dataset()) is None
    assert separation_options(_model(separation_weight=10.0)) == (10.0, 5.0)
    assert separation_options(_model("Focal", separation_weight=2, separation_sigma=1.5), _dataset()) == (2.0, 1.5)
    assert separation_options(_model(separation_weight=10.0, separation_sigma=10.6)) == (10.0, 10.6)  # ceil(31.8) = 32
    assert separation_options(_model(separation_weight=10.0, boundary_weight=4.0)) == (10.0, 5.0)  # (the two keys go together)
    for opt, key in REFUSALS:
        with pytest.raises(ValueError, match=r"\[opt\] " + key):
            separation_options(_model(**opt))
    for loss in OTHER_LOSSES:
        with pytest.raises(ValueError, match=r"\[opt\] separation_weight"):
            separation_options(_model(loss, separation_weight=10.0))
    with pytest.raises(ValueError, match=r"\[opt\] separation_weight needs an object class"):
        separation_options(_model(separation_weight=10.0), _dataset(("background",)))


@pytest.mark.parametrize("case", range(len(REFUSALS) + len(OTHER_LOSSES) + 1))
def test_rs_train_ends_on_a_bad_key_before_any_work(tmp_path, case):
    """Every refusal is an ``Error: [opt] separation_...`` exit of ``rs train`` itself, before it asks for a device or makes the
    checkpoint directory; the last case is a dataset with a single class."""

    from robosat_amd.tools import train as train_tool

    classes = ("background", "parking")
    if case < len(REFUSALS):
        loss, (opt, key) = "CrossEntropy", REFUSALS[case]
    elif case < len(REFUSALS) + len(OTHER_LOSSES):
        loss, opt, key = OTHER_LOSSES[case - len(REFUSALS)], {"separation_weight": 10.0}, "separation_weight"
    else:
        loss, opt, key, classes = "Focal", {"separation_weight": 10.0}, "separation_weight", ("background",)
    ds = str(tmp_path / "dataset.toml")
    cfg_ds = _dataset(classes)
    cfg_ds["common"]["dataset"] = str(tmp_path)
    save_config(cfg_ds, ds)
    ck = str(tmp_path / "pth")
    cfg = _model(loss, **opt)
    cfg["common"]["checkpoint"] = ck
    cfg["model"] = {"pretrained": False}
    model = str(tmp_path / "model.toml")
    save_config(cfg, model)
    assert load_config(model)["opt"].keys() == cfg["opt"].keys()
    with pytest.raises(SystemExit) as err:
        train_tool.main(argparse.Namespace(model=model, dataset=ds, checkpoint=None, resume=False, workers=0))
    assert str(err.value).startswith("Error: [opt] " + key), str(err.value)
    assert not os.path.exists(ck)


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
def test_the_modules_take_separation_and_validate_it():
    from robosat_amd import losses

    for cls in (losses.CrossEntropyLoss2d, losses.FocalLoss2d):
        assert cls().separation is None and cls(separation=(10, 5)).separation == (10.0, 5.0)
        both = cls(boundary=(4, 3), separation=(10, 5), hard=0.25)
        assert (both.boundary, both.separation, both.hard) == ((4.0, 3.0), (10.0, 5.0), (0.25, None))
        for bad in ((0, 5), (10, 0), (10, 10.7), (float("nan"), 5), (10,), 10.0, ("10", 5), (True, 5)):
            with pytest.raises(ValueError):
                cls(separation=bad)
    for cls in (losses.mIoULoss2d, losses.LovaszLoss2d, losses.LovaszSoftmax2d, losses.TverskyLoss2d):
        with pytest.raises(TypeError):
            cls(separation=(10, 5))
    with pytest.raises(RuntimeError, match="no CPU"):  # and there is no CPU path for the plane either
        ops.separation_weight_plane(torch.zeros(1, 4, 4, dtype=torch.int64), 10.0, 5.0)


def test_without_the_key_the_criteria_are_the_ones_of_today(monkeypatch):
    """``separation=None`` constructs the same criterion, and its call goes to the autograd function it went to before, with the
    arguments it had."""

    from robosat_amd import losses

    for cls, kw in ((losses.CrossEntropyLoss2d, {}), (losses.FocalLoss2d, {"gamma": 3}),
                    (losses.CrossEntropyLoss2d, {"boundary": (4, 3)}), (losses.FocalLoss2d, {"hard": (0.5, 0.2), "ignore_index": 255})):
        a, b = cls(weight=[1.0, 2.0], **kw), cls(weight=[1.0, 2.0], separation=None, **kw)
        assert b.separation is None
        assert {k: v for k, v in vars(a).items() if not k.startswith("_")} == {k: v for k, v in vars(b).items() if not k.startswith("_")}
        assert torch.equal(a.weight, b.weight) and list(a.state_dict()) == list(b.state_dict())

    calls = []
    for fn in ("_NLLFn", "_NLLBoundaryFn", "_NLLHardFn", "_NLLSeparationFn"):
        monkeypatch.setattr(getattr(losses, fn), "apply", staticmethod(lambda *args, fn=fn: calls.append((fn, len(args))) or torch.zeros(())))
    monkeypatch.setattr(losses, "_check", lambda inputs, targets: (inputs, targets))
    x, t = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    losses.CrossEntropyLoss2d()(x, t)
    losses.FocalLoss2d(ignore_index=255)(x, t)
    losses.CrossEntropyLoss2d(boundary=(4, 3))(x, t)
    losses.FocalLoss2d(hard=0.5)(x, t)
    losses.FocalLoss2d(hard=0.5).eval()(x, t)
    assert calls == [("_NLLFn", 6), ("_NLLFn", 7), ("_NLLBoundaryFn", 8), ("_NLLHardFn", 9), ("_NLLFn", 6)]
    del calls[:]
    losses.CrossEntropyLoss2d(separation=(10, 5))(x, t)
    losses.FocalLoss2d(separation=(10, 5), boundary=(4, 3), hard=0.5).eval()(x, t)
    assert calls == [("_NLLSeparationFn", 10)] * 2


# ---- the entry points -------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_bound_and_the_abi_version_stays():
    from ctypes import c_int, c_long

    from robosat_amd import _lib
    from robosat_amd._lib import P

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    assert re.search(r"\bint rs_separation_weight_plane\(const long long\* targets, const float\* table, const float\* base, float\* plane, "
                     r"int N, int C, int H, int W,\s+int D, int ignore, void\* workspace, rs_stream_t stream\);", header)
    assert "long rs_separation_weight_plane_workspace_bytes(int N, int H, int W);" in header
    assert _lib.SIGNATURES["rs_separation_weight_plane_workspace_bytes"] == (c_long, [c_int] * 3)
    assert _lib.SIGNATURES["rs_separation_weight_plane"] == (c_int, [P] * 4 + [c_int] * 6 + [P, P])
    assert _lib.ABI_VERSION == 24  # (new symbols, no old one changed)
    for line in ("s2 = a + b + isqrt(4*a*b)", "Reach D = ceil(3*sigma), 1 <= D <= 32", "Two touching objects of different classes are one object"):
        assert line in header
    assert "is not built" not in header[header.index("BOUNDARY-WEIGHTED"):header.index("HARD-PIXEL MINING")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Separation weight" in design and "s2 = a + b + isqrt(4·a·b)" in design
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        assert lib.rs_abi_version() == 24
        assert lib.rs_separation_weight_plane_workspace_bytes(2, 5, 7) == 16 + 14 * 70
        for bad in ((0, 5, 7), (2, 0, 7), (2, 5, -1), (65536, 1, 1), (1, 4097, 1), (1 << 9, 1 << 10, 1 << 10)):
            assert lib.rs_separation_weight_plane_workspace_bytes(*bad) == _lib.RS_EINVAL
