"""The float64 loss reference, its input builders and its comparison function (tests/losses_ref.py), checked on the CPU:
the reference reproduces the goldens of the unmodified reference, every builder's case is what it claims to be, and the
comparison at the project's bars sees a dropped or doubled probe pixel -- while a random case with a pixel dropped passes it,
which is why the GPU tests (tests/test_gpu_losses.py) carry single-pixel probes."""

import math
import os

import numpy as np
import pytest
import torch

import losses_ref as L
from oracle import robosat_ref as R


@pytest.mark.parametrize("tag", ["c2", "c4"])
@pytest.mark.parametrize("name", L.CRITERIA)
def test_float64_reference_reproduces_goldens(golden_dir, tag, name):
    g = np.load(os.path.join(golden_dir, "losses.npz"))
    logits, targets, weight = (torch.from_numpy(g["{}_{}".format(tag, k)]) for k in ("logits", "targets", "weight"))
    loss, grad = L.ref64(name, logits, targets, weight)
    want_loss, want_grad = float(g["{}_{}_loss".format(tag, name)]), torch.from_numpy(g["{}_{}_grad".format(tag, name)])
    dl, dg = L.distances(loss, grad, want_loss, want_grad)
    print(tag, name, "loss distance {:.2e} gradient distance {:.2e}".format(dl, dg))
    assert dl <= 2e-6 and dg <= 2e-6


@pytest.mark.parametrize("name", ["CrossEntropy", "Focal"])
def test_multiplicity_form_is_the_reference(name):
    logits, targets, weight = L.random_case(3, 5, 7, 9, 1)
    for wt in (weight, None):
        want_loss, want_grad = L.ref64(name, logits, targets, wt, gamma=2)
        loss, grad, sw = L.nll_family64(name, logits, targets, wt, gamma=2)
        assert abs(loss - want_loss) <= 1e-14 * max(1, abs(want_loss)) and float((grad - want_grad).abs().max()) <= 1e-15
        assert abs(sw - (float(weight.double()[targets].sum()) if wt is not None else targets.numel())) <= 1e-9


def test_masked_miou_form_is_the_reference():
    for kind in ("uniform", "confident"):
        logits, targets, weight = L.miou_case(kind)
        want_loss, want_grad = L.ref64("mIoU", logits, targets, weight)
        miou, nll, x = L.miou_terms64(logits, targets, weight)
        loss = max(miou, nll)
        loss.backward()
        assert abs(float(loss.detach()) - want_loss) <= 1e-14 and float((x.grad - want_grad).abs().max()) <= 1e-15


def test_focal_gamma_zero_is_cross_entropy_in_the_reference():
    logits, targets, weight = L.random_case(3, 5, 7, 9, 2)
    a, ga = L.ref64("Focal", logits, targets, weight, gamma=0)
    b, gb = L.ref64("CrossEntropy", logits, targets, weight)
    assert abs(a - b) <= 1e-14 and float((ga - gb).abs().max()) <= 1e-15


def test_single_class_is_exactly_zero_in_the_reference():
    logits, targets, weight = L.random_case(3, 1, 7, 9, 3)
    for name in L.CRITERIA:
        loss, grad = L.ref64(name, logits, targets, weight)
        assert loss == 0.0 and float(grad.abs().max()) == 0.0


# ---- every builder's stated property --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(L.MIOU_CASES))
def test_miou_cases_take_their_branch(kind):
    logits, targets, weight = L.miou_case(kind)  # (asserts branch and gap itself)
    assert tuple(logits.shape) == L.MIOU_SHAPE
    branch, gap = L.miou_branch64(logits, targets, weight)
    print(kind, branch, "gap {:.3f}".format(gap))
    assert branch == L.MIOU_CASES[kind][3]
    _, grad = L.ref64("mIoU", logits, targets, weight)
    assert bool(torch.isfinite(grad).all())
    if kind == "absent_class":
        assert int((targets[0] == 2).sum()) == 0
    if kind == "all_background":
        assert int(targets[1].abs().sum()) == 0 and int(targets[0].max()) == 2


def test_every_miou_case_is_far_from_the_branch_point():
    """The class-count, shape and weight cases of tests/test_gpu_losses.py: random logits take the NLL branch, confident ones
    the soft-IoU branch, each by >= 1e-2 on the float64 reference."""

    for confident, branch in ((False, "nll"), (True, "miou")):
        for c in range(1, 9):
            L.assert_miou_branch_is_safe(*L.class_count_case(c, confident), branch=branch)
        for n, h, w in L.SHAPES:
            for c in (2, 5):
                L.assert_miou_branch_is_safe(*L.shape_case(n, c, h, w, confident), branch=branch)
    logits, targets = L.rare_class_case(2, 5, 33, 31, 70)
    for wt in L.weight_cases(5, targets).values():
        L.assert_miou_branch_is_safe(logits, targets, wt)
    L.assert_miou_branch_is_safe(*L.random_case(2, 2, 7, 9, seed=81))
    L.assert_miou_branch_is_safe(*L.random_case(1, 8, 513, 513, seed=80))


@pytest.mark.parametrize("s,m", [(1, 60), (30, 60)])
def test_saturated_cases_are_finite_and_within_the_bars_in_float32(s, m):
    logits, targets, weight = L.saturated_case(s, m, seed=50 + s)
    for name in ("CrossEntropy", "Focal"):
        want_loss, want_grad = L.ref64(name, logits, targets, weight, gamma=2)
        assert math.isfinite(want_loss) and bool(torch.isfinite(want_grad).all())
        loss, grad = L.ref32(name, logits, targets, weight, gamma=2)
        L.compare(name, loss, grad, want_loss, want_grad, "saturated s={} m={} fp32 vs fp64".format(s, m))


def test_unsaturated_case_has_a_finite_reference_gradient_below_gamma_one():
    for c in (2, 5):
        for n, h, w in ((3, 7, 9), (2, 129, 129)):
            logits, targets, weight = L.unsaturated_case(n, c, h, w, seed=60 + c)
            loss, grad = L.ref64("Focal", logits, targets, weight, gamma=0.5)
            assert math.isfinite(loss) and bool(torch.isfinite(grad).all())
    # the corner the builder keeps out: pt == 1 in float32 makes the reference's own gradient NaN for gamma < 1
    sat, tg, wt = L.saturated_case(1, 60, seed=51)
    _, grad32 = L.ref32("Focal", sat, tg, wt, gamma=0.5)
    assert not bool(torch.isfinite(grad32).all())


def test_weight_cases():
    logits, targets = L.rare_class_case(2, 5, 33, 31, 70)
    ws = L.weight_cases(5, targets)
    assert ws["none"] is None
    zero_class = int((ws["zero"] == 0).nonzero()[0])
    assert int((ws["zero"] == 0).sum()) == 1 and int((targets == zero_class).sum()) > 0
    rare_class = int(ws["rare1e3"].argmax())
    assert float(ws["rare1e3"][rare_class]) == 1e3 and rare_class == 4
    assert 0 < int((targets == rare_class).sum()) < targets.numel() // 50
    for wt in ws.values():
        for name in L.CRITERIA:
            loss, grad = L.ref64(name, logits, targets, wt)
            assert math.isfinite(loss) and bool(torch.isfinite(grad).all())


def test_probe_positions_are_the_edges_they_are_named_for():
    n, c, h, w = L.NLL_PROBE_SHAPE
    hw, p = h * w, n * h * w
    assert hw % 256 == 185 and p > 1024 * 256
    assert L.NLL_PROBE_POSITIONS == (0, 255, 256, hw - 1, hw, 1024 * 256 - 1, 1024 * 256, p - 1)
    n, c, h, w = L.MIOU_PROBE_SHAPE
    assert L.MIOU_PROBE_HW == (0, 255, 256, 64 * 256 - 1, 64 * 256, h * w - 1) and h * w > 64 * 256


def test_miou_probe_rests_on_its_six_pixels():
    logits, targets, weight, moves = L.miou_probe_case()  # (asserts the branch, the gap and the six moves itself)
    print("moves of the float64 loss with one probe pixel left out:", ["{:.2e}".format(m) for m in moves])
    assert int((targets == 2).sum()) == 6 and int((targets[0] == 2).sum()) == 0
    assert min(moves) > 100 * L.LOSS_BAR


# ---- the comparison is sensitive where it has to be -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["CrossEntropy", "Focal"])
@pytest.mark.parametrize("pstar", L.NLL_PROBE_POSITIONS)
def test_comparison_sees_a_dropped_or_doubled_probe_pixel(name, pstar):
    logits, targets, weight = L.nll_probe_case(pstar)
    n, c, h, w = logits.shape
    want_loss, want_grad = L.ref64(name, logits, targets, weight)
    share, away = L.nll_probe_share(name, logits, targets, weight, pstar)
    print(name, pstar, "probe share of the loss {:.6f}, gradient elsewhere / at the probe {:.1e}".format(share, away))
    assert share > 0.999 and away < 1e-6
    sw = float(weight.double()[targets].sum())
    for m in (0.0, 2.0):
        mult = torch.ones(n * h * w)
        mult[pstar] = m
        loss, grad, sw_m = L.nll_family64(name, logits, targets, weight, mult=mult.view(n, h, w))
        with pytest.raises(AssertionError):
            L.compare(name, loss, grad, want_loss, want_grad, "probe {} counted {} times".format(pstar, int(m)))
        assert abs(sw_m - sw) > 1e-6 * sw  # and the weight-sum check of the GPU test sees it too
    loss, grad, _ = L.nll_family64(name, logits, targets, weight)
    L.compare(name, loss, grad, want_loss, want_grad, "probe {} counted once".format(pstar))


def test_comparison_sees_a_dropped_miou_probe_pixel():
    logits, targets, weight, _ = L.miou_probe_case()
    n, c, h, w = logits.shape
    want_loss, want_grad = L.ref64("mIoU", logits, targets, weight)
    for hw in L.MIOU_PROBE_HW:
        keep = torch.ones(n, h * w, dtype=torch.bool)
        keep[1, hw] = False
        miou, _, x = L.miou_terms64(logits, targets, weight, keep.view(n, h, w))
        miou.backward()
        with pytest.raises(AssertionError):
            L.compare("mIoU", float(miou.detach()), x.grad, want_loss, want_grad, "probe hw {} left out".format(hw))


@pytest.mark.parametrize("name", ["CrossEntropy", "Focal"])
def test_random_inputs_do_not_see_a_dropped_pixel(name):
    """Why the probes exist: on the largest random case the last pixel can go missing and the project's bars still hold."""

    logits, targets, weight = L.random_case(1, 8, 513, 513, 80)
    want_loss, want_grad = L.ref64(name, logits, targets, weight)
    mult = torch.ones(513 * 513)
    mult[-1] = 0
    loss, grad, _ = L.nll_family64(name, logits, targets, weight, mult=mult.view(1, 513, 513))
    grad.view(8, -1)[:, -1] = want_grad.view(8, -1)[:, -1]  # (a kernel that drops the pixel from the SUMS still writes its gradient)
    dl, _ = L.compare(name, loss, grad, want_loss, want_grad, "random 1x8x513x513, last pixel left out of the sums")
    assert dl > 0


@pytest.mark.parametrize("n,c,h,w", L.COUNT_SHAPES)
def test_counts_case_has_ties_and_dropped_pixels(n, c, h, w):
    scores, targets = L.counts_case(n, c, h, w, seed=90 + c)
    total, dropped = L.counts_ref(scores, targets)
    assert (dropped > 0) == (c > 2)
    assert bool((scores * 2 == torch.round(scores * 2)).all())
