"""Boundary label relaxation without a GPU: the reference (tests/relax_ref.py) held against itself and against the strict references,
the purpose of the feature shown on the reference, the model config key and ``rs train``'s refusals, the modules' new argument, the
new entry points."""

import argparse
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as B  # noqa: E402
import losses_ref as L  # noqa: E402
import relax_ref as X  # noqa: E402

from robosat_amd import ops  # noqa: E402
from robosat_amd.config import RELAX_LOSSES, load_config, relax_options, save_config  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the set plane ------------------------------------------------------------------------------------------------------------------
def test_the_window_by_hand():
    """0 0 0 1 0 0 2 at radius 1: a pixel sees itself and its two neighbours; at radius 2 the middle zero sees both objects."""

    row = np.array([[[0, 0, 0, 1, 0, 0, 2]]])
    assert X.sets_brute(row, 1)[0, 0].tolist() == [1, 1, 3, 3, 3, 5, 5]
    assert X.sets_brute(row, 2)[0, 0].tolist() == [1, 3, 3, 3, 7, 7, 5]
    assert X.sets_brute(np.transpose(row, (0, 2, 1)), 2)[0, :, 0].tolist() == [1, 3, 3, 3, 7, 7, 5]
    # an ignored pixel has no set and adds no bit; the valid pixel it encloses keeps its own
    ig = np.array([[[255, 255, 255], [255, 1, 255], [255, 255, 255]]])
    assert X.sets_brute(ig, 1, 255)[0].tolist() == [[0, 0, 0], [0, 2, 0], [0, 0, 0]]
    assert X.sets_brute(np.full((1, 2, 3), 255), 2, 255).tolist() == [[[0, 0, 0], [0, 0, 0]]]
    # a diagonal neighbour counts: the window is a square
    diag = np.array([[[0, 0], [0, 3]]])
    assert X.sets_brute(diag, 1)[0].tolist() == [[9, 9], [9, 9]]
    # bit 7
    assert X.sets_brute(np.array([[[7, 0]]]), 1)[0].tolist() == [[129, 129]]


@pytest.mark.parametrize("radius", [1, 2, 5, 11, 16])
@pytest.mark.parametrize("ignore", [False, True])
def test_brute_force_sets_agree_with_the_separable_form(radius, ignore):
    t = X.blocks_raster(2, 8, 23, 37, seed=radius, ignore=ignore)
    ig = X.IGNORE if ignore else None
    brute = X.sets_brute(t, radius, ig)
    cen = X.census(t, brute, ig)
    assert cen["bits"] == 255 and cen["more"] > 0 and (cen["ignored"] > 0) == ignore, cen
    assert np.array_equal(brute, X.sets_separable(t, radius, ig))
    valid = t != X.IGNORE
    assert ((brute[valid] >> t[valid]) & 1).all() and (brute[~valid] == 0).all()  # own bit; nothing at an ignored pixel
    small = X.blocks_raster(1, 3, 5, 7, seed=3, ignore=ignore)
    assert np.array_equal(X.sets_brute(small, radius, ig), X.sets_separable(small, radius, ig))


def test_images_never_see_each_other():
    t = np.zeros((2, 6, 6), dtype=np.int64)
    t[1] = 1
    assert X.sets_brute(t, 3)[0].max() == 1 and X.sets_brute(t, 3)[1].min() == 2


# ---- the loss -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["CrossEntropy", "Focal"])
@pytest.mark.parametrize("ignore", [False, True])
def test_an_all_singleton_input_is_the_strict_loss(name, ignore):
    """Every valid pixel's set is its own label alone: ``loss64`` is ``boundary_ref.loss64`` / ``losses_ref.nll_family64``."""

    c, radius = 3, 2
    t = X.singleton_raster(2, c, 9, 31, radius) if ignore else np.full((2, 9, 31), 1, dtype=np.int64)
    ig = X.IGNORE if ignore else None
    sets = X.sets_brute(t, radius, ig)
    cen = X.census(t, sets, ig)
    assert cen["two"] == 0 and cen["more"] == 0 and cen["one"] > 0 and (cen["ignored"] > 0) == ignore, cen
    targets = torch.from_numpy(t)
    logits, weight = X.logits_for((2, c, 9, 31), 5)
    mult = X.pixel_weights(2, 9, 31, 6)
    got = X.loss64(name, logits, targets, sets, weight, mult, ig)
    want = B.loss64(name, logits, targets, weight, mult, ig)
    assert abs(got[0] - want[0]) <= 1e-12 * max(1.0, abs(want[0])) and abs(got[2] - want[2]) <= 1e-12 * want[2]
    assert float((got[1] - want[1]).abs().max()) <= 1e-12 * float(want[1].abs().max())
    if not ignore:
        plain = L.nll_family64(name, logits, targets, weight)
        unweighted = X.loss64(name, logits, targets, sets, weight)
        assert abs(unweighted[0] - plain[0]) <= 1e-12 * max(1.0, abs(plain[0]))
        assert float((unweighted[1] - plain[1]).abs().max()) <= 1e-12 * float(plain[1].abs().max())


def test_the_denominator_is_the_strict_one_and_a_full_set_costs_nothing():
    c = 3
    targets, sets = X.loss_case(c, "wide", True)
    logits, weight = X.logits_for((3, c, 33, 65), 9)
    relaxed = X.loss64("CrossEntropy", logits, targets, sets, weight, None, X.IGNORE)
    strict = B.loss64("CrossEntropy", logits, targets, weight, torch.ones(3, 33, 65), X.IGNORE)
    assert relaxed[2] == strict[2] and 0 < relaxed[0] < strict[0]
    t = X.noise_raster(1, c, 6, 6, 1)
    full = X.sets_brute(t, 5)
    assert (full == 7).all()
    loss, grad, _ = X.loss64("CrossEntropy", logits[:1, :, :6, :6], torch.from_numpy(t), full)
    assert loss == 0.0 and float(grad.abs().max()) == 0.0
    none = X.loss64("Focal", logits[:1, :, :6, :6], torch.full((1, 6, 6), X.IGNORE), np.zeros((1, 6, 6), np.uint8), None, None, X.IGNORE)
    assert none[0] == 0.0 and none[2] == 0.0 and float(none[1].abs().max()) == 0.0


# ---- the purpose ------------------------------------------------------------------------------------------------------------------------
SHIFT_RADIUS = 2
SHIFTS = [(dx, dy) for dx in (-SHIFT_RADIUS, 0, 1, SHIFT_RADIUS) for dy in (-SHIFT_RADIUS, 0, SHIFT_RADIUS) if (dx, dy) != (0, 0)]


@pytest.mark.parametrize("dx, dy", SHIFTS)
def test_labels_shifted_within_the_radius_cost_nothing(dx, dy):
    """Confident logits that follow the true shape, labels moved by (dx, dy) with |dx|, |dy| <= R: relaxed loss below 1e-6, strict
    cross-entropy above 0.1."""

    logits, labels = X.shifted_case(24, 28, SHIFT_RADIUS, dx, dy)
    sets = X.sets_brute(labels.numpy(), SHIFT_RADIUS)
    relaxed = X.loss64("CrossEntropy", logits, labels, sets)[0]
    strict = L.nll_family64("CrossEntropy", logits, labels)[0]
    assert relaxed < 1e-6 and strict > 0.1, (relaxed, strict)
    assert X.loss64("Focal", logits, labels, sets)[0] < 1e-6


@pytest.mark.parametrize("dx, dy", [(SHIFT_RADIUS + 1, 0), (0, -SHIFT_RADIUS - 1), (SHIFT_RADIUS + 1, SHIFT_RADIUS + 1)])
def test_a_shift_beyond_the_radius_costs_again(dx, dy):
    logits, labels = X.shifted_case(24, 28, SHIFT_RADIUS, dx, dy)
    sets = X.sets_brute(labels.numpy(), SHIFT_RADIUS)
    assert X.loss64("CrossEntropy", logits, labels, sets)[0] > 0.1


# ---- [opt] relax ----------------------------------------------------------------------------------------------------------------------
def _model(**opt):
    return {"opt": dict({"loss": "CrossEntropy"}, **opt)}


def test_relax_options_accepts():
    assert relax_options(_model()) is None
    assert RELAX_LOSSES == ("CrossEntropy", "Focal")
    for loss in RELAX_LOSSES:
        for r in (1, 2, 16):
            assert relax_options(_model(loss=loss, relax=r)) == r
    assert relax_options(_model(relax=3, boundary_weight=4.0, separation_weight=10.0)) == 3  # (it composes with both planes)
    assert ops.RELAX_MAX_RADIUS == 16


@pytest.mark.parametrize("value", [0, 17, -1, True, False, 2.0, 2.5, "2", [2], float("nan")])
def test_relax_options_refuses_a_bad_value(value):
    with pytest.raises(ValueError) as err:
        relax_options(_model(relax=value))
    assert str(err.value).startswith("[opt] relax must be an integer radius in 1..16 pixels"), str(err.value)


@pytest.mark.parametrize("loss", ["mIoU", "Lovasz", "LovaszSoftmax", "Tversky", None])
def test_relax_options_refuses_another_loss(loss):
    with pytest.raises(ValueError) as err:
        relax_options(_model(loss=loss, relax=2))
    assert str(err.value).startswith("[opt] relax relaxes the pixel terms of CrossEntropy and Focal only"), str(err.value)


def test_relax_options_refuses_hard_fraction_beside_it():
    with pytest.raises(ValueError) as err:
        relax_options(_model(relax=2, hard_fraction=0.25))
    assert str(err.value).startswith("[opt] relax cannot stand beside [opt] hard_fraction"), str(err.value)
    assert "relaxed loss" in str(err.value)


@pytest.mark.parametrize("extra, prefix", [({"relax": 0}, "Error: [opt] relax must be"), ({"relax": 2.0}, "Error: [opt] relax must be"),
                                           ({"relax": 2, "loss": "Lovasz"}, "Error: [opt] relax relaxes"),
                                           ({"relax": 2, "hard_fraction": 0.5}, "Error: [opt] relax cannot stand beside")])
def test_rs_train_ends_before_any_device_is_touched(tmp_path, monkeypatch, extra, prefix):
    import synth
    from robosat_amd.tools import train as train_tool

    ckdir = os.path.join(str(tmp_path), "pth")
    model_toml, ds_toml = synth.write_configs(str(tmp_path), os.path.join(str(tmp_path), "nowhere"), ckdir, loss="CrossEntropy",
                                              batch_size=2, image_size=64, epochs=1)
    cfg = load_config(model_toml)
    cfg["opt"].update(extra)
    save_config(cfg, model_toml)

    def no_device(*a, **k):
        raise AssertionError("rs train asked for the device before it refused the key")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(SystemExit) as err:
        train_tool.main(argparse.Namespace(model=model_toml, dataset=ds_toml, checkpoint=None, resume=False, workers=0))
    assert str(err.value).startswith(prefix), str(err.value)
    assert not os.path.exists(ckdir)


# ---- the criteria ---------------------------------------------------------------------------------------------------------------------
def test_the_criteria_take_relax_and_refuse_what_the_text_says():
    from robosat_amd.losses import ClDiceLoss2d, CrossEntropyLoss2d, FocalLoss2d

    for cls in (CrossEntropyLoss2d, FocalLoss2d):
        assert cls().relax is None and cls(relax=1).relax == 1 and cls(relax=16, boundary=(4.0, 2.0), separation=(10.0, 2.0)).relax == 16
        for bad in (0, 17, True, 2.0, "2", (2,)):
            with pytest.raises(ValueError, match="relax"):
                cls(relax=bad)
        with pytest.raises(ValueError, match="relax cannot be combined with hard.*relaxed loss"):
            cls(relax=2, hard=0.25)
    assert ClDiceLoss2d(CrossEntropyLoss2d(relax=2), 0.3).relax == 2 and ClDiceLoss2d(CrossEntropyLoss2d(), 0.3).relax is None


def test_a_cpu_tensor_is_refused_not_computed():
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.label_set_plane(torch.zeros(1, 4, 4, dtype=torch.int64), 2)
    for bad in (0, 17, True, 1.0):
        with pytest.raises(ValueError, match="relaxation radius"):
            ops.label_set_plane(torch.zeros(1, 4, 4, dtype=torch.int64), bad)


def test_the_entry_points_are_declared_and_exported():
    from robosat_amd import _lib

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    for name in ("rs_label_set_plane", "rs_nll_loss_fwd_rx", "rs_nll_loss_bwd_rx"):
        assert name in _lib.SIGNATURES and re.search(r"\bint {}\(".format(name), header), name
    pw, rx = _lib.SIGNATURES["rs_nll_loss_fwd_pw"], _lib.SIGNATURES["rs_nll_loss_fwd_rx"]
    assert rx[1][:-1] == pw[1] and rx[0] is pw[0]  # the `_pw` signature plus the sets
    pw, rx = _lib.SIGNATURES["rs_nll_loss_bwd_pw"], _lib.SIGNATURES["rs_nll_loss_bwd_rx"]
    assert rx[1][:-1] == pw[1]
