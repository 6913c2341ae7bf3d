"""CPU checks of the Tversky loss family (no kernel is launched): the float64 reference of tests/tversky_ref.py against the original
project's soft IoU and against ``losses_ref.nll_family64``, the Dice identity, the two-shard identity of the data-parallel recipe on
the reference itself, the config keys, the module's constructor and the declared entry points."""

import argparse
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import losses_ref as L  # noqa: E402
import tversky_ref as T  # noqa: E402

from robosat_amd import ops  # noqa: E402
from robosat_amd.config import boundary_options, hard_options, load_config, save_config, tversky_options  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 3, 8])
def test_the_soft_jaccard_is_the_original_soft_iou_term(c):
    logits, targets, _ = T.random_case(3, c, 7, 9, seed=c)
    miou, _, x = L.miou_terms64(logits, targets)
    miou.backward()
    loss, grad, t = T.ref64(logits, targets, alpha=1.0, beta=1.0, gamma=1.0, smooth=0.0, per_image=True, classes="all", ce=0.0)
    assert abs(loss - float(miou.detach())) <= 1e-12 and loss == t
    assert float((grad - x.grad).abs().max()) <= 1e-12


def test_the_dice_identity():
    logits, targets, _ = T.random_case(2, 4, 9, 11, seed=1)
    tp, sp, cnt = T.segment_sums(logits.double(), targets)
    ti = T.tversky_index(tp, sp, cnt, 0.5, 0.5, 0.0)
    assert float((ti - 2 * tp / (sp + cnt)).abs().max()) <= 1e-15
    want = (1 - 2 * tp / (sp + cnt)).mean()  # (every class is present in both images)
    assert bool((cnt > 0).all())
    assert abs(T.ref64(logits, targets, smooth=0.0)[0] - float(want)) <= 1e-15


@pytest.mark.parametrize("per_image", [True, False])
def test_the_compound_is_the_term_plus_the_weighted_cross_entropy(per_image):
    logits, targets, weight = T.random_case(2, 3, 9, 11, seed=2)
    for w in (None, weight):
        t_loss, t_grad, _ = T.ref64(logits, targets, 0.3, 0.7, 0.75, 1.0, per_image=per_image)
        ce_loss, ce_grad, _ = L.nll_family64("CrossEntropy", logits, targets, w)
        loss, grad, t = T.ref64(logits, targets, 0.3, 0.7, 0.75, 1.0, per_image=per_image, ce=0.5, weight=w)
        assert t == t_loss and abs(loss - (t_loss + 0.5 * ce_loss)) <= 1e-14
        assert float((grad - (t_grad + 0.5 * ce_grad)).abs().max()) <= 1e-14


def test_the_reference_with_an_ignore_label():
    """Ignored pixels enter no sum: cutting a column of ignored pixels out of every image changes nothing; an image with no valid
    pixel contributes 0 and the divisor stays N."""

    logits, targets, weight = T.random_case(2, 3, 6, 8, seed=3)
    marked = targets.clone()
    marked[:, :, 5] = T.IGNORE
    keep = [0, 1, 2, 3, 4, 6, 7]
    for per_image in (True, False):
        a = T.ref64(logits, marked, 0.3, 0.7, 2.0, 1.0, per_image=per_image, ce=0.5, weight=weight, ignore=T.IGNORE)
        b = T.ref64(logits[:, :, :, keep], targets[:, :, keep], 0.3, 0.7, 2.0, 1.0, per_image=per_image, ce=0.5, weight=weight)
        assert abs(a[0] - b[0]) <= 1e-14 and float((a[1][:, :, :, keep] - b[1]).abs().max()) <= 1e-14
        assert float(a[1][:, :, :, 5].abs().max()) == 0.0
    marked = targets.clone()
    marked[1] = T.IGNORE
    for classes in ("present", "all"):
        a = T.ref64(logits, marked, classes=classes, ignore=T.IGNORE)
        b = T.ref64(logits[:1], targets[:1], classes=classes)
        assert abs(a[0] - 0.5 * b[0]) <= 1e-15 and float(a[1][1].abs().max()) == 0.0


@pytest.mark.parametrize("params", T.PARAMS)
@pytest.mark.parametrize("per_image", [True, False])
def test_the_two_shard_identity_on_the_reference(params, per_image):
    """The data-parallel recipe (per image: only the CE denominator; batch form: the whole block, coefficients times world) gives
    the single evaluation over the 4 images; for the batch form the un-exchanged per-shard evaluation misses it by more than 10 bars."""

    alpha, beta, gamma, smooth = params
    logits, targets, weight = T.shard_case()
    kw = dict(alpha=alpha, beta=beta, gamma=gamma, smooth=smooth, classes="present", ce=0.5)
    (loss, grad), (naive_loss, naive_grad) = T.two_shard_reference(logits, targets, weight, per_image, **kw)
    got_loss, got_grad = T.exchanged64(logits, targets, weight, per_image, **kw)
    assert abs(got_loss - loss) <= 1e-13 and float((got_grad - grad).abs().max()) <= 1e-13 * float(grad.abs().max())
    dl, dg = L.distances(naive_loss, naive_grad, loss, grad)
    if not per_image:
        assert dl > 10 * L.LOSS_BAR and dg > 10 * L.MIOU_GRAD_BAR, (dl, dg)
    else:
        assert dl > 10 * L.LOSS_BAR, dl  # (the CE denominators of the two shards differ)


def test_float32_torch_stays_far_inside_the_bars():
    """What the number format alone costs on the inputs of the GPU tests: far below LOSS_BAR and MIOU_GRAD_BAR."""

    worst = [0.0, 0.0]
    for c, (n, h, w) in ((2, (3, 33, 31)), (8, (3, 33, 31)), (3, (2, 129, 129))):
        logits, targets, weight = T.random_case(n, c, h, w, seed=c)
        for alpha, beta, gamma, smooth in T.PARAMS:
            for per_image in (True, False):
                kw = dict(alpha=alpha, beta=beta, gamma=gamma, smooth=smooth, per_image=per_image, ce=0.5, weight=weight)
                want = T.ref64(logits, targets, **kw)
                got = T.ref32(logits, targets, **kw)
                dl, dg = L.distances(got[0], got[1], want[0], want[1])
                worst = [max(worst[0], dl), max(worst[1], dg)]
    print("float32 torch: loss distance {:.1e}, gradient distance {:.1e}".format(*worst))
    assert worst[0] <= L.LOSS_BAR / 20 and worst[1] <= L.MIOU_GRAD_BAR / 20, worst


def test_the_builders_hold_what_they_are_named_after():
    T.absent_class_case()
    logits, targets, _ = T.shard_case()
    mixes = [torch.bincount(targets[s].reshape(-1), minlength=3).double() / targets[s].numel() for s in (slice(0, 2), slice(2, 4))]
    assert float((mixes[0] - mixes[1]).abs().max()) > 0.5
    marked = T.with_ignored(targets)
    assert 0.25 < float((marked == T.IGNORE).double().mean()) < 0.42


# ---- the config keys ----------------------------------------------------------------------------------------------------------------
def _model(loss="Tversky", **opt):
    return {"common": {"cuda": True, "batch_size": 2, "image_size": 64, "checkpoint": "/nonexistent"},
            "opt": dict({"epochs": 1, "lr": 1e-4, "loss": loss}, **opt)}


DEFAULTS = {"alpha": 0.5, "beta": 0.5, "gamma": 1.0, "smooth": 1.0, "per_image": True, "classes": "present", "ce": 0.0}
REFUSALS = [
    ({"tversky_alpha": -1}, "tversky_alpha"), ({"tversky_alpha": "0.5"}, "tversky_alpha"), ({"tversky_alpha": True}, "tversky_alpha"),
    ({"tversky_alpha": float("nan")}, "tversky_alpha"), ({"tversky_beta": -0.1}, "tversky_beta"),
    ({"tversky_beta": float("inf")}, "tversky_beta"), ({"tversky_alpha": 0, "tversky_beta": 0.0}, "tversky_alpha"),
    ({"tversky_gamma": 0}, "tversky_gamma"), ({"tversky_gamma": -1.0}, "tversky_gamma"), ({"tversky_gamma": "2"}, "tversky_gamma"),
    ({"tversky_smooth": -1e-3}, "tversky_smooth"), ({"tversky_smooth": False}, "tversky_smooth"),
    ({"tversky_ce": -1}, "tversky_ce"), ({"tversky_ce": float("nan")}, "tversky_ce"),
    ({"tversky_per_image": 1}, "tversky_per_image"), ({"tversky_per_image": "true"}, "tversky_per_image"),
    ({"tversky_classes": "some"}, "tversky_classes"), ({"tversky_classes": True}, "tversky_classes"),
]
OTHER_LOSSES = ("CrossEntropy", "Focal", "mIoU", "Lovasz", "LovaszSoftmax")


def test_the_config_keys():
    assert tversky_options(_model()) == DEFAULTS
    for loss in OTHER_LOSSES:
        assert tversky_options(_model(loss)) is None
    got = tversky_options(_model(tversky_alpha=0.3, tversky_beta=0.7, tversky_gamma=0.75, tversky_smooth=0, tversky_per_image=False,
                                 tversky_classes="all", tversky_ce=1))
    assert got == {"alpha": 0.3, "beta": 0.7, "gamma": 0.75, "smooth": 0.0, "per_image": False, "classes": "all", "ce": 1.0}
    assert tversky_options(_model(tversky_alpha=0, tversky_beta=1))["alpha"] == 0.0
    for opt, key in REFUSALS:
        with pytest.raises(ValueError, match=r"\[opt\] " + key):
            tversky_options(_model(**opt))
    for loss in OTHER_LOSSES:
        with pytest.raises(ValueError, match=r"\[opt\] tversky_ce belongs to \[opt\] loss = 'Tversky'"):
            tversky_options(_model(loss, tversky_ce=0.5))
    # the per-pixel weights of CrossEntropy and Focal refuse this loss
    with pytest.raises(ValueError, match=r"\[opt\] boundary_weight"):
        boundary_options(_model(boundary_weight=4.0))
    with pytest.raises(ValueError, match=r"\[opt\] hard_fraction"):
        hard_options(_model(hard_fraction=0.25))
    assert boundary_options(_model()) is None and hard_options(_model()) is None


CLI_REFUSALS = [("Tversky", opt, key) for opt, key in REFUSALS[:3] + REFUSALS[6:8] + REFUSALS[-2:]] + [
    ("CrossEntropy", {"tversky_alpha": 0.3}, "tversky_alpha"), ("mIoU", {"tversky_ce": 1.0}, "tversky_ce"),
    ("Tversky", {"boundary_weight": 4.0}, "boundary_weight"), ("Tversky", {"hard_fraction": 0.25}, "hard_fraction"),
]


@pytest.mark.parametrize("case", range(len(CLI_REFUSALS)))
def test_rs_train_ends_on_a_bad_key_before_any_work(tmp_path, case):
    """Every refusal is an ``Error: [opt] ...`` exit of ``rs train`` itself, before it asks for a device or makes the checkpoint
    directory."""

    from robosat_amd.tools import train as train_tool

    loss, opt, key = CLI_REFUSALS[case]
    ds = str(tmp_path / "dataset.toml")
    save_config({"common": {"dataset": str(tmp_path), "classes": ["background", "parking"], "colors": ["denim", "orange"]}}, ds)
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


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def test_the_module_validates_its_arguments():
    from robosat_amd import losses

    crit = losses.TverskyLoss2d()
    assert (crit.alpha, crit.beta, crit.gamma, crit.smooth, crit.ce) == (0.5, 0.5, 1.0, 1.0, 0.0)
    assert crit.per_image is True and crit.classes == "present" and crit.weight is None and crit.ignore_index is None
    assert crit.global_batch is False and isinstance(crit, losses._WeightedLoss)
    crit = losses.TverskyLoss2d(0.3, 0.7, 0.75, 0, False, "all", 1, weight=[1.0, 2.0], ignore_index=255)
    assert (crit.alpha, crit.beta, crit.gamma, crit.smooth, crit.ce) == (0.3, 0.7, 0.75, 0.0, 1.0)
    assert crit.per_image is False and crit.classes == "all" and crit.weight.dtype == torch.float32 and crit.ignore_index == 255
    assert "weight" in dict(crit.named_buffers())
    for bad in (dict(alpha=-1), dict(beta=-0.5), dict(alpha=0, beta=0), dict(gamma=0), dict(gamma=-2), dict(smooth=-1), dict(ce=-0.5),
                dict(alpha=float("nan")), dict(gamma=float("inf")), dict(ce="1"), dict(smooth=True), dict(classes="some"),
                dict(per_image=1)):
        with pytest.raises(ValueError):
            losses.TverskyLoss2d(**bad)
    for extra in (dict(boundary=(4, 3)), dict(hard=0.25)):
        with pytest.raises(TypeError):
            losses.TverskyLoss2d(**extra)
    with pytest.raises(ValueError, match="alpha and beta"):
        ops.tversky_params(0, 0, 1, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU"):
        losses.TverskyLoss2d()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.tversky_sums(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_bound_and_the_abi_version_stays():
    from ctypes import c_float, c_int, c_long

    from robosat_amd import _lib
    from robosat_amd._lib import P

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    for name in ("rs_tversky_workspace_bytes", "rs_tversky_sums", "rs_tversky_finalize", "rs_tversky_bwd"):
        assert name + "(" in header and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["rs_tversky_workspace_bytes"] == (c_long, [c_int, c_int])
    assert _lib.SIGNATURES["rs_tversky_sums"] == (c_int, [P] * 4 + [c_int] * 6 + [P, P])
    assert _lib.SIGNATURES["rs_tversky_finalize"] == (c_int, [P] * 3 + [c_int] * 2 + [c_float] * 5 + [c_int] * 3 + [P])
    assert _lib.SIGNATURES["rs_tversky_bwd"] == (c_int, [P] * 6 + [c_int] * 5 + [c_float, c_int, P])
    assert _lib.ABI_VERSION == 24  # (new symbols, no old one changed)
    for line in ("TI_s = (TP + eps) / (TP + alpha*FP + beta*FN + eps)", "l_s = max(1 - TI_s, 0)^gamma", "exactly +0.0f",
                 "its coefficients are multiplied by world"):
        assert line in header, line
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7g" in design and "Tversky loss family" in design
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        assert lib.rs_abi_version() == 24
        assert lib.rs_tversky_workspace_bytes(2, 3) == 2 * 65 * 11 * 8
        for bad in ((0, 3), (2, 1), (2, 9), (-1, 2), (65536, 2)):
            assert lib.rs_tversky_workspace_bytes(*bad) == _lib.RS_EINVAL
        # the argument checks come before any launch: null pointers and bad parameters are refused on a host without a device
        assert lib.rs_tversky_sums(None, None, None, None, 1, 2, 4, 4, 1, -1, None, None) == _lib.RS_EINVAL
        assert lib.rs_tversky_finalize(None, None, None, 1, 2, 0.5, 0.5, 1.0, 1.0, 0.0, 0, 1, 1, None) == _lib.RS_EINVAL
        assert lib.rs_tversky_bwd(None, None, None, None, None, None, 1, 2, 4, 4, 1, 0.0, -1, None) == _lib.RS_EINVAL
