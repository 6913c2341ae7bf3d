"""Hard-pixel mining without a GPU: the numpy reference (tests/hard_ref.py) against a brute-force count, k at and just above an integer
product, the cap against struct-packed float32, the model config keys and ``rs train``'s refusals, the modules' argument checks, the new
entry points."""

import argparse
import math
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hard_ref as H  # noqa: E402
import losses_ref as L  # noqa: E402

from robosat_amd import ops  # noqa: E402
from robosat_amd.config import hard_options, load_config, save_config  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("fraction", [1e-12, 0.1, 0.25, 0.5, 0.99, 1.0])
def test_the_sort_is_the_count_on_tiny_inputs(seed, fraction):
    """Few distinct values (ties at the threshold are the rule), an image that is all ignored, the extremes present."""

    rng = np.random.RandomState(seed)
    pool = np.array([0, 1, 2, 0x3F800000, 0x7F800000, 0xFFFFFFFF, 77, 0x80000000], dtype=np.uint32)
    keys = pool[rng.randint(0, len(pool) if seed % 2 else 3, size=(3, 3, 5))]
    valid = rng.rand(3, 3, 5) < 0.7
    valid[1] = False
    for cap in (H.NO_CAP, 0x3F800000, 1, 0):
        plane, info = H.select(keys, valid, fraction, cap)
        want_plane, want_info = H.select_brute(keys, valid, fraction, cap)
        assert info.tolist() == want_info.tolist() and plane.tobytes() == want_plane.tobytes()
        assert info[1].tolist() == [0, 0, 0, 0] and not plane[1].any()
        for i in (0, 2):
            v, k, tau, kept = info[i].tolist()
            assert v == int(valid[i].sum()) and kept >= k >= (1 if v else 0) and kept == int(plane[i].sum())
            if cap == H.NO_CAP and v:
                assert int((keys[i][valid[i]] > tau).sum()) < k  # fewer than k above tau: tau is the k-th largest


def test_the_base_plane_is_carried_by_the_kept_pixels():
    keys = np.arange(12, dtype=np.uint32).reshape(1, 3, 4)
    base = (np.arange(12, dtype=np.float32).reshape(1, 3, 4) + 0.5)
    plane, info = H.select(keys, np.ones((1, 3, 4), dtype=bool), 0.25, base=base)
    assert info.tolist() == [[12, 3, 9, 3]]
    assert plane.reshape(-1).tolist() == [0.0] * 9 + [9.5, 10.5, 11.5]


def test_k_at_an_integer_product_and_just_above_one():
    assert H.k_of(256, 0.25) == 64  # 0.25 * 256 is exactly 64.0: ceil adds nothing
    assert H.k_of(256, math.nextafter(0.25, 1.0)) == 65  # one ulp above: 64.00000000000001 -> 65
    assert H.k_of(257, 0.25) == 65  # 64.25
    assert H.k_of(0, 0.5) == 0 and H.k_of(1, 1e-12) == 1 and H.k_of(10 ** 6, 1e-12) == 1
    assert H.k_of(7, 1.0) == 7 and H.k_of(3, 0.999999) == 3
    # the definition is the IEEE double product, whatever the decimal reading: 0.3 * 10.0 rounds to exactly 3.0, 0.07 * 100.0 above 7.0,
    # 0.29 * 100.0 below 29.0
    assert 0.3 * 10.0 == 3.0 and H.k_of(10, 0.3) == 3 and H.k_of(10, 0.1) == 1
    assert 0.07 * 100.0 == 7.000000000000001 and H.k_of(100, 0.07) == 8
    assert 0.29 * 100.0 == 28.999999999999996 and H.k_of(100, 0.29) == 29


@pytest.mark.parametrize("below", [0.5, 0.3, 0.05, 1e-3, 0.999, 1e-30])
def test_the_cap_is_the_float32_of_minus_log(below):
    want = struct.unpack("<I", struct.pack("<f", -math.log(below)))[0]
    assert ops.hard_cap(below) == want == H.cap_of(below)
    assert int(np.array([np.float32(-math.log(below))]).view(np.uint32)[0]) == want
    assert 0 < want < 0x7F800000


def test_the_cap_and_the_fraction_refuse_bad_values():
    for bad in (0, 1, 1.5, -0.1, float("nan"), float("inf"), "0.5", True, None):
        with pytest.raises(ValueError):
            ops.hard_cap(bad)
    for bad in (0, -0.5, 1.0000001, float("nan"), float("inf"), "0.5", True, None):
        with pytest.raises(ValueError):
            ops.hard_fraction(bad)
    assert ops.hard_fraction(1) == 1.0 and ops.hard_fraction(1e-12) == 1e-12
    assert ops.HARD_NO_CAP == H.NO_CAP == 0xFFFFFFFF
    # the fraction crosses the C ABI as the 64 bits of the double, exactly
    for f in (0.25, 1.0, 1e-12, math.nextafter(0.25, 1.0), 0.1):
        assert struct.unpack("<d", struct.pack("<q", ops.hard_fraction_bits(f)))[0] == f
    assert ops.hard_fraction_bits(1.0) == 0x3FF0000000000000


def test_the_key_mapping_and_the_reference_loss():
    assert H.keys_u32(np.array([0.0, -0.0, -1e-9, float("nan"), 1.0, float("inf"), 1e-45])).tolist() == [0, 0, 0, 0, 0x3F800000, 0x7F800000, 1]
    x, t, w = L.random_case(2, 3, 7, 9, seed=5)
    k64 = H.keys64(x, t)
    want = -torch.log_softmax(x.double(), 1).gather(1, t.unsqueeze(1)).squeeze(1).numpy()
    assert np.abs(k64 - want).max() < 1e-12
    # a plane of ones is the oracle's criterion; a selected plane is the family's sum over the kept pixels
    ones = np.ones((2, 7, 9), dtype=np.float32)
    for name in ("CrossEntropy", "Focal"):
        got, grad, _ = H.loss64(name, x, t, w, ones)
        ref, ref_grad = L.ref64(name, x, t, w)
        assert abs(got - ref) < 1e-12 and float((grad - ref_grad).abs().max()) < 1e-12
    plane, info = H.select(H.keys_u32(k64), H.valid_of(t), 0.25)
    assert info[:, 1].tolist() == [16, 16] and info[:, 3].tolist() == [16, 16]
    got, grad, den = H.loss64("CrossEntropy", x, t, None, plane)
    assert abs(got - float(np.sort(k64.reshape(2, -1), axis=1)[:, -16:].sum()) / 32) < 1e-12 and den == 32.0
    assert int(torch.count_nonzero(grad.permute(0, 2, 3, 1)[torch.from_numpy(plane) == 0])) == 0
    assert H.selection_is_safe(k64, H.valid_of(t), 0.25) > 1e-4
    k64[0, 0, 0] = k64[0, 0, 1] = 50.0  # a tie across the threshold of a top-1 selection is not safe
    with pytest.raises(AssertionError):
        H.selection_is_safe(k64, H.valid_of(t), 1e-12)


# ---- the model config keys and rs train's refusals ----------------------------------------------------------------------------------
def _model(loss="CrossEntropy", **opt):
    return {"common": {"cuda": True, "batch_size": 2, "image_size": 64, "checkpoint": "/nowhere"},
            "opt": dict({"epochs": 1, "lr": 1e-4, "loss": loss}, **opt)}


REFUSALS = [
    ({"hard_fraction": "0.25"}, "hard_fraction"), ({"hard_fraction": True}, "hard_fraction"), ({"hard_fraction": 0}, "hard_fraction"),
    ({"hard_fraction": 0.0}, "hard_fraction"), ({"hard_fraction": -0.25}, "hard_fraction"), ({"hard_fraction": 1.5}, "hard_fraction"),
    ({"hard_fraction": float("inf")}, "hard_fraction"), ({"hard_fraction": float("nan")}, "hard_fraction"),
    ({"hard_fraction": 0.25, "hard_below": "0.3"}, "hard_below"), ({"hard_fraction": 0.25, "hard_below": 0.0}, "hard_below"),
    ({"hard_fraction": 0.25, "hard_below": 1.0}, "hard_below"), ({"hard_fraction": 0.25, "hard_below": 1}, "hard_below"),
    ({"hard_fraction": 0.25, "hard_below": -0.3}, "hard_below"), ({"hard_fraction": 0.25, "hard_below": float("nan")}, "hard_below"),
    ({"hard_fraction": 0.25, "hard_below": False}, "hard_below"),
    ({"hard_below": 0.3}, "hard_below"),
]
OTHER_LOSSES = ("mIoU", "Lovasz", "LovaszSoftmax")


def test_the_config_keys():
    assert hard_options(_model()) is None and hard_options(_model("mIoU")) is None
    assert hard_options(_model(hard_fraction=0.25)) == (0.25, None)
    assert hard_options(_model("Focal", hard_fraction=1, hard_below=0.3)) == (1.0, 0.3)
    assert hard_options(_model(hard_fraction=1e-12, boundary_weight=4.0)) == (1e-12, None)
    for opt, key in REFUSALS:
        with pytest.raises(ValueError, match=r"\[opt\] " + key):
            hard_options(_model(**opt))
    for loss in OTHER_LOSSES:
        with pytest.raises(ValueError, match=r"\[opt\] hard_fraction"):
            hard_options(_model(loss, hard_fraction=0.25))


@pytest.mark.parametrize("case", range(len(REFUSALS) + len(OTHER_LOSSES)))
def test_rs_train_ends_on_a_bad_key_before_any_work(tmp_path, case):
    """Every refusal is an ``Error: [opt] hard_...`` exit of ``rs train`` itself, before it asks for a device or makes the checkpoint
    directory."""

    from robosat_amd.tools import train as train_tool

    if case < len(REFUSALS):
        loss, (opt, key) = "CrossEntropy", REFUSALS[case]
    else:
        loss, opt, key = OTHER_LOSSES[case - len(REFUSALS)], {"hard_fraction": 0.25}, "hard_fraction"
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


def test_the_modules_take_hard_and_validate_it():
    from robosat_amd import losses

    for cls in (losses.CrossEntropyLoss2d, losses.FocalLoss2d):
        assert cls().hard is None and cls(hard=0.25).hard == (0.25, None) and cls(hard=(1, 0.3)).hard == (1.0, 0.3)
        assert cls(hard=(0.5, None), boundary=(4, 3)).hard == (0.5, None)
        for bad in (0, 1.5, -1, float("nan"), (0.25, 0), (0.25, 1), (0.25, 0.3, 1), "0.25", True, (True, 0.3), ("0.25", None)):
            with pytest.raises(ValueError):
                cls(hard=bad)
    for cls in (losses.mIoULoss2d, losses.LovaszLoss2d, losses.LovaszSoftmax2d):
        with pytest.raises(TypeError):
            cls(hard=0.25)
    with pytest.raises(RuntimeError, match="no CPU"):  # and there is no CPU path for the plane either
        ops.hard_pixel_plane(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), 0.25)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.hard_pixel_select(torch.zeros(1, 4, 4, dtype=torch.int32), 0.25)


# ---- the entry points -------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_bound_and_the_abi_version_stays():
    from ctypes import c_int, c_long

    from robosat_amd import _lib
    from robosat_amd._lib import P

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    assert "long rs_hard_pixel_workspace_bytes(int N, int H, int W);" in header
    assert re.search(r"\bint rs_hard_pixel_plane\(const float\* logits, const long long\* targets, const float\* base, float\* plane, "
                     r"unsigned\* keys_out,\s+long long\* info, int N, int C, int H, int W, long fraction_bits, long cap, int ignore, "
                     r"void\* workspace,\s+rs_stream_t stream\);", header)
    assert re.search(r"\bint rs_hard_pixel_select\(const unsigned\* keys, const long long\* targets, const float\* base, float\* plane, "
                     r"long long\* info, int N,\s+int H, int W, long fraction_bits, long cap, int ignore, void\* workspace, "
                     r"rs_stream_t stream\);", header)
    assert _lib.SIGNATURES["rs_hard_pixel_workspace_bytes"] == (c_long, [c_int] * 3)
    assert _lib.SIGNATURES["rs_hard_pixel_plane"] == (c_int, [P] * 6 + [c_int] * 4 + [c_long, c_long, c_int, P, P])
    assert _lib.SIGNATURES["rs_hard_pixel_select"] == (c_int, [P] * 5 + [c_int] * 3 + [c_long, c_long, c_int, P, P])
    assert _lib.ABI_VERSION == 24  # (new symbols, no old one changed)
    for line in ("k_n = min(V_n, max(1, (int64) ceil(fraction * (double) V_n)))", "Ties at tau_n are all kept", "gets exactly +0.0f",
                 "0xFFFFFFFF means \"no cap\""):
        assert line in header, line
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7e" in design and "Hard-pixel mining" in design and "Per image, not per batch" in design
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        assert lib.rs_abi_version() == 24
        assert lib.rs_hard_pixel_workspace_bytes(2, 5, 7) == (2 * (3 * 2048 + 4) + 70) * 4
        for bad in ((0, 5, 7), (2, 0, 7), (2, 5, -1), (1, 1 << 16, 1 << 15), (-1, 1, 1)):
            assert lib.rs_hard_pixel_workspace_bytes(*bad) == _lib.RS_EINVAL
        assert lib.rs_hard_pixel_workspace_bytes(1, 1 << 15, (1 << 16) - 1) > 0  # H * W = 2^31 - 2^15
