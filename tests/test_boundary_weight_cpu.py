"""The boundary weight without a GPU: the numpy reference (tests/boundary_ref.py) against a hand-worked case and the brute-force
transform, the table, the rasters the GPU tests use, the model config keys and ``rs train``'s refusals, the new entry points."""

import argparse
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as B  # noqa: E402
import edt_ref  # noqa: E402
import losses_ref as L  # noqa: E402

from robosat_amd import ops  # noqa: E402
from robosat_amd.config import boundary_options, load_config, save_config  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDARD = [(24, 20, 1.0), (40, 48, 1.5), (70, 66, 3.0)]


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_the_hand_worked_row():
    row = np.array([[0, 0, 0, 1, 1, 1]])
    assert B.boundary_set(row).astype(int).tolist() == [[0, 0, 1, 1, 0, 0]]
    assert B.distance2(row, 1.0).tolist() == [[4, 1, 0, 0, 1, 4]]  # reach 3: the cap 9 is not met
    assert B.distance2(row, 0.5).tolist() == [[4, 1, 0, 0, 1, 4]]  # reach 2: the ends sit AT the cap 4
    tab = B.table(4.0, 0.5)
    assert B.plane(row[None], 4.0, 0.5)[0].tolist() == [[1.0, float(tab[1]), float(tab[0]), float(tab[0]), float(tab[1]), 1.0]]
    assert float(tab[0]) == 5.0
    column = B.plane(row.T[None], 4.0, 0.5)[0]
    assert column.T.tolist() == B.plane(row[None], 4.0, 0.5)[0].tolist()


def test_edges_of_the_image_and_of_ignored_regions_are_no_boundary():
    assert not B.boundary_set(np.ones((3, 4))).any()  # the raster's edge
    t = np.array([[1, 1, 255, 0, 0]])
    assert not B.boundary_set(t, ignore=255).any() and B.boundary_set(t).any()  # 1 | 255 | 0: nothing is known in between
    assert B.plane(t[None], 4.0, 1.0, ignore=255)[0].tolist() == [[1.0, 1.0, 0.0, 1.0, 1.0]]
    assert B.plane(np.full((1, 2, 3), 255), 4.0, 1.0, ignore=255).tolist() == [[[0.0] * 3] * 2]
    two = np.stack([np.array([[0, 1, 1, 1]]), np.array([[1, 1, 1, 1]])])  # images never see each other
    assert (B.plane(two, 4.0, 2.0)[1] == 1).all() and (B.plane(two, 4.0, 2.0)[0] > 1).all()


@pytest.mark.parametrize("h, w, sigma", STANDARD[:1] + [(24, 24, 2.0), (5, 7, 2.0), (1, 9, 1.0), (9, 1, 1.0), (17, 23, 8.0)])
@pytest.mark.parametrize("ignore", [False, True])
def test_the_two_pass_transform_is_the_brute_force_one_on_the_complement_masks(h, w, sigma, ignore):
    t = B.standard_raster(h, w, ignore)
    mask = ~B.boundary_set(t, B.IGNORE if ignore else None)
    assert (edt_ref.edt(mask, B.reach(sigma)) == edt_ref.edt_brute(mask, B.reach(sigma))).all()
    rng = np.random.RandomState(h * 100 + w)
    noisy = rng.randint(0, 3, size=(h, w))
    mask = ~B.boundary_set(noisy)
    assert (edt_ref.edt(mask, B.reach(sigma)) == edt_ref.edt_brute(mask, B.reach(sigma))).all()


@pytest.mark.parametrize("w0, sigma", [(4.0, 3.0), (10.0, 1.0), (0.5, 42.6), (1e-3, 0.2), (4.0, 1.5)])
def test_the_table_is_float32_non_increasing_and_above_one(w0, sigma):
    tab = B.table(w0, sigma)
    assert tab.dtype == np.float32 and tab.shape == (B.reach(sigma) ** 2,)
    assert (np.diff(tab) <= 0).all() and (tab > 1).all()
    assert float(tab[0]) == float(np.float32(1.0 + w0))
    mine = ops.boundary_table(w0, sigma)  # the package's table is the same bits
    assert mine.dtype == np.float32 and mine.tobytes() == tab.tobytes()
    assert ops.boundary_reach(w0, sigma) == B.reach(sigma)


@pytest.mark.parametrize("h, w, sigma", STANDARD)
def test_the_standard_raster_has_both_kinds_of_pixel(h, w, sigma):
    t, m = B.standard_case(h, w, sigma)
    above, at = B.shares(m[0], t[0].numpy())
    print("{}x{} sigma {}: {:.0%} above 1, {:.0%} at 1".format(h, w, sigma, above, at))
    want = {(40, 48): (0.59, 0.41), (70, 66): (0.64, 0.36), (24, 20): (0.68, 0.32)}[(h, w)]
    assert abs(above - want[0]) <= 0.005 + 1e-9 and abs(at - want[1]) <= 0.005 + 1e-9  # (the whole per cent they round to)
    ti, mi = B.standard_case(h, w, sigma, ignore=True)  # (asserts its own 20 % / 20 % and that the boundary set differs)
    assert (mi[ti == B.IGNORE] == 0).all() and (mi[ti != B.IGNORE] >= 1).all()
    assert int((ti == B.IGNORE).sum()) > 0


def test_the_reference_loss_is_the_weighted_family():
    t, m = B.standard_case(24, 20, 1.0, ignore=True)
    x, w = B.logits_for(t, 3, seed=5)
    for name in ("CrossEntropy", "Focal"):
        loss, grad, den = B.loss64(name, x, t, w, m, ignore=B.IGNORE)
        valid = t != B.IGNORE
        assert abs(den - float((w.double()[t.clamp(max=2)] * m.double())[valid].sum())) < 1e-9
        assert not grad[:, :, ~valid[0]].any() and grad[:, :, valid[0]].abs().min() > 0
        ones, _, _ = B.loss64(name, x, t, w, torch.ones_like(m), ignore=B.IGNORE)
        assert abs(loss - ones) > 1e-3  # (the plane matters on this case)
    assert B.loss64("Focal", x, torch.full_like(t, 255), w, m, ignore=255)[0] == 0.0
    # nothing ignored, all ones: the oracle's criterion
    t, m = B.standard_case(24, 20, 1.0)
    want, grad = L.ref64("CrossEntropy", x, t, w)
    got, g, _ = B.loss64("CrossEntropy", x, t, w, torch.ones_like(m))
    assert abs(got - want) < 1e-12 and float((g - grad).abs().max()) < 1e-12


# ---- the model config keys and rs train's refusals ----------------------------------------------------------------------------------
def _model(loss="CrossEntropy", **opt):
    return {"common": {"cuda": True, "batch_size": 2, "image_size": 64, "checkpoint": "/nowhere"},
            "opt": dict({"epochs": 1, "lr": 1e-4, "loss": loss}, **opt)}


REFUSALS = [
    ({"boundary_weight": "4"}, "boundary_weight"), ({"boundary_weight": True}, "boundary_weight"),
    ({"boundary_weight": float("inf")}, "boundary_weight"), ({"boundary_weight": float("nan")}, "boundary_weight"),
    ({"boundary_weight": 0}, "boundary_weight"), ({"boundary_weight": -1.0}, "boundary_weight"),
    ({"boundary_weight": 4.0, "boundary_sigma": "3"}, "boundary_sigma"), ({"boundary_weight": 4.0, "boundary_sigma": 0.0}, "boundary_sigma"),
    ({"boundary_weight": 4.0, "boundary_sigma": float("inf")}, "boundary_sigma"),
    ({"boundary_weight": 4.0, "boundary_sigma": -2.0}, "boundary_sigma"),
    ({"boundary_weight": 4.0, "boundary_sigma": 42.7}, "boundary_sigma"),  # ceil(128.1) = 129
    ({"boundary_sigma": 3.0}, "boundary_sigma"),
]


def test_the_config_keys():
    assert boundary_options(_model()) is None
    assert boundary_options(_model(boundary_weight=4.0)) == (4.0, 3.0)
    assert boundary_options(_model("Focal", boundary_weight=2, boundary_sigma=1.5)) == (2.0, 1.5)
    assert boundary_options(_model(boundary_weight=4.0, boundary_sigma=42.6)) == (4.0, 42.6)  # ceil(127.8) = 128
    for opt, key in REFUSALS:
        with pytest.raises(ValueError, match=r"\[opt\] " + key):
            boundary_options(_model(**opt))
    for loss in ("mIoU", "Lovasz", "LovaszSoftmax"):
        with pytest.raises(ValueError, match=r"\[opt\] boundary_weight"):
            boundary_options(_model(loss, boundary_weight=4.0))


@pytest.mark.parametrize("case", range(len(REFUSALS) + 3))
def test_rs_train_ends_on_a_bad_key_before_any_work(tmp_path, case):
    """Every refusal is an ``Error: [opt] boundary_...`` exit of ``rs train`` itself, before it asks for a device or makes the
    checkpoint directory."""

    from robosat_amd.tools import train as train_tool

    if case < len(REFUSALS):
        loss, (opt, key) = "CrossEntropy", REFUSALS[case]
    else:
        loss, opt, key = ("mIoU", "Lovasz", "LovaszSoftmax")[case - len(REFUSALS)], {"boundary_weight": 4.0}, "boundary_weight"
    ds = str(tmp_path / "dataset.toml")
    save_config({"common": {"dataset": str(tmp_path), "classes": ["background", "parking"], "colors": ["denim", "orange"]},
                 "weights": {"values": [1.0, 2.0]}}, ds)
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


def test_the_modules_take_boundary_and_validate_it():
    from robosat_amd import losses

    for cls in (losses.CrossEntropyLoss2d, losses.FocalLoss2d):
        assert cls().boundary is None and cls(boundary=(4, 3)).boundary == (4.0, 3.0)
        for bad in ((0, 3), (4, 0), (4, 42.7), (float("nan"), 3), (4,), 4.0, ("4", 3), (True, 3)):
            with pytest.raises(ValueError):
                cls(boundary=bad)
    for cls in (losses.mIoULoss2d, losses.LovaszLoss2d, losses.LovaszSoftmax2d):
        with pytest.raises(TypeError):
            cls(boundary=(4, 3))
    with pytest.raises(RuntimeError, match="no CPU"):  # and there is no CPU path for the plane either
        ops.boundary_weight_plane(torch.zeros(1, 4, 4, dtype=torch.int64), 4.0, 3.0)


# ---- the entry points -------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_bound_and_the_abi_version_stays():
    from ctypes import c_int, c_long

    from robosat_amd import _lib
    from robosat_amd._lib import P

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    for name, base in (("rs_nll_loss_fwd_pw", "rs_nll_loss_fwd"), ("rs_nll_loss_bwd_pw", "rs_nll_loss_bwd")):
        assert re.search(r"\bint {}\([^;]*rs_stream_t stream, const float\* pixel_weight,\s+int ignore\);".format(name), header), name
        assert _lib.SIGNATURES[name] == (_lib.SIGNATURES[base][0], _lib.SIGNATURES[base][1] + [P, c_int])
    assert re.search(r"\bint rs_boundary_weight_plane\(const long long\* targets, const float\* table, float\* plane, int N, int C, int H, "
                     r"int W, int R, int ignore,\s+void\* workspace, rs_stream_t stream\);", header)
    assert "long rs_boundary_weight_plane_workspace_bytes(int N, int H, int W);" in header
    assert _lib.SIGNATURES["rs_boundary_weight_plane_workspace_bytes"] == (c_long, [c_int] * 3)
    assert len(_lib.SIGNATURES["rs_boundary_weight_plane"][1]) == 11
    assert _lib.ABI_VERSION == 24  # (new symbols, no old one changed)
    for line in ("exactly 1.0f where d2(p) == R^2", "exactly 0.0f at an ignored pixel", "The edge of an ignored region is no boundary."):
        assert line in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Boundary weight" in design and "table[k] = float32(1 + w0·exp(−k / (2·sigma²)))" in design
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        assert lib.rs_abi_version() == 24
        assert lib.rs_boundary_weight_plane_workspace_bytes(2, 5, 7) == 6 * 70
        for bad in ((0, 5, 7), (2, 0, 7), (2, 5, -1), (65536, 1, 1), (1, 4097, 1), (1 << 9, 1 << 10, 1 << 10)):
            assert lib.rs_boundary_weight_plane_workspace_bytes(*bad) == _lib.RS_EINVAL
