"""CrossEntropyLoss2d, FocalLoss2d, mIoULoss2d and the confusion counts (csrc/loss.hip) on the MI355X against the oracle in
float64 (tests/losses_ref.py), at the sizes and inputs where these kernels take the code the golden vectors never run: every
class count 1..8 (9 refused), the second trip of the grid-stride loops (1 024 blocks of 256 pixels; 64 blocks per image for
mIoU), image borders inside a block, blocks with fewer than 64 live threads, no weights / a zero weight / a 1e3 weight, gamma
0 / 0.5 / 1 / 2 / 5, saturated pixels, both mIoU branches with absent classes, strided inputs, workspace reuse -- and
single-pixel probes on which one dropped, doubled or mis-indexed pixel is the whole answer.

Bars: the project's own (losses_ref.compare), at every size.  Every case runs with upstream gradients 1 and 1.5.

Measured on the MI355X, largest distance over all cases of this file (the module prints them when it finishes, ``-s``):
CrossEntropy loss 4.9e-8 / gradient 2.8e-7, Focal 6.0e-8 / 6.1e-7, mIoU 4.9e-8 / 1.7e-6 -- within 10x of what the float32
oracle differs from the float64 one on a CPU (5e-7 / 6e-7), against bars of 2e-5 / 2e-4 (mIoU gradient 1e-3).

Kept on purpose, not tested: labels outside [0, C) (the kernels index ``weight[t]`` unchecked: DESIGN.md), a batch whose
weights sum to 0 (0/0 in the reference too), and gamma < 1 on a pixel with pt == 1 (the reference's own gradient is NaN there)."""

import functools

import numpy as np
import pytest
import torch

import losses_ref as L
from oracle import tools_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UPSTREAM = 1.5

RECORD = {}  # criterion -> (largest loss distance, largest gradient distance) seen by this module


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, (dl, dg) in sorted(RECORD.items()):
        print("\nlargest distances, {}: loss {:.2e} (bar {:.0e}), gradient {:.2e} (bar {:.0e})".format(
            name, dl, L.LOSS_BAR, dg, L.grad_bar(name)))


def criterion(name, weight, gamma=2):
    from robosat_amd import losses

    if name == "CrossEntropy":
        return losses.CrossEntropyLoss2d(weight=weight).to(DEV)
    if name == "Focal":
        return losses.FocalLoss2d(gamma=gamma, weight=weight).to(DEV)
    return losses.mIoULoss2d(weight=weight).to(DEV)


def run_raw(name, logits_dev, targets_dev, weight, gamma=2, upstream=UPSTREAM):
    """(loss, gradient) as the device computed them for ``upstream`` * loss, copied to the host untouched."""

    x = logits_dev.detach().requires_grad_(True)
    loss = criterion(name, weight, gamma)(x, targets_dev)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss * upstream).backward()
    return loss.detach().cpu(), x.grad.cpu()


def check(name, logits, targets, weight, gamma=2, what="", want=None, branch=None):
    """Runs criterion ``name`` on the GPU with upstream gradients 1 and 1.5 and compares both with the float64 reference."""

    if name == "mIoU":
        L.assert_miou_branch_is_safe(logits, targets, weight, branch)
    want_loss, want_grad = want if want is not None else L.ref64(name, logits, targets, weight, gamma)
    x, t = logits.to(DEV), targets.to(DEV)
    out = None
    for upstream in (1.0, UPSTREAM):
        loss, grad = run_raw(name, x, t, weight, gamma, upstream)
        out = L.compare(name, loss.item(), grad.double() / upstream, want_loss, want_grad,
                        "{} upstream {}".format(what, upstream), RECORD)
    return out


@functools.lru_cache(maxsize=None)
def shape_case(n, c, h, w, confident=False):
    return L.shape_case(n, c, h, w, confident)


# ---- 1. every class count -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", L.CRITERIA)
@pytest.mark.parametrize("c", range(1, 9))
def test_every_class_count(c, name):
    """N = 3, H x W = 7 x 9: HW = 63 puts both image borders inside the one block and leaves one partial wave."""

    logits, targets, weight = L.class_count_case(c)
    check(name, logits, targets, weight, what="C={} 3x7x9".format(c), branch="nll")
    if name == "mIoU":  # and the soft-IoU branch of every instance
        check(name, *L.class_count_case(c, confident=True), what="C={} 3x7x9 confident".format(c), branch="miou")
    if c == 1:
        loss, grad = run_raw(name, logits.to(DEV), targets.to(DEV), weight)
        assert loss.item() == 0.0 and float(grad.abs().max()) == 0.0  # exactly


def test_nine_classes_are_refused():
    """The ABI returns RS_EINVAL before any launch: C = 9 must not run as the 8-class kernel."""

    from robosat_amd import ops

    logits, targets, weight = L.random_case(1, 9, 7, 9, seed=19)
    x, t, w = logits.to(DEV), targets.to(DEV), weight.to(DEV)
    for name in L.CRITERIA:
        with pytest.raises(ValueError):
            criterion(name, weight)(x, t)
    with pytest.raises(ValueError):
        ops.nll_loss_fwd(x, t, w, ops.NLL_CROSS_ENTROPY, 0.0)
    with pytest.raises(ValueError):
        ops.nll_loss_fwd(x, t, None, ops.NLL_FOCAL, 2.0)
    with pytest.raises(ValueError):
        ops.miou_loss_fwd(x, t, w)
    counts = torch.zeros(4, device=DEV, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.confusion_counts(x, t, counts)
    assert counts.tolist() == [0, 0, 0, 0]


# ---- 2. shapes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", L.CRITERIA)
@pytest.mark.parametrize("c", [2, 5])
@pytest.mark.parametrize("n,h,w", L.SHAPES, ids=["{}x{}x{}".format(*s) for s in L.SHAPES])
def test_shapes(n, h, w, c, name):
    logits, targets, weight = shape_case(n, c, h, w)
    check(name, logits, targets, weight, what="{}x{}x{}x{}".format(n, c, h, w), branch="nll")
    if name == "mIoU":  # random logits take the NLL branch; confident ones (noise 0.5, margin 4) the soft-IoU branch
        check(name, *shape_case(n, c, h, w, True), what="{}x{}x{}x{} confident".format(n, c, h, w), branch="miou")


# ---- 3. weights -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", L.CRITERIA)
@pytest.mark.parametrize("kind", ["none", "zero", "rare1e3"])
def test_weights(kind, name):
    """No weights (the criterion's default: a null pointer in the kernels), a present class at exactly 0, 1e3 on a rare class."""

    logits, targets = L.rare_class_case(2, 5, 33, 31, seed=70)
    weight = L.weight_cases(5, targets)[kind]
    check(name, logits, targets, weight, what="weight " + kind)


# ---- 4. gamma -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [2, 5])
@pytest.mark.parametrize("gamma", [0, 1, 2, 5])
def test_focal_gamma(gamma, c):
    logits, targets, weight = L.random_case(3, c, 37, 41, seed=20 + c, scale=3.0)
    check("Focal", logits, targets, weight, gamma=gamma, what="gamma={} C={}".format(gamma, c))
    if gamma == 0:  # must be the cross-entropy of the same inputs, to the same bars
        check("Focal", logits, targets, weight, gamma=0, what="gamma=0 vs CrossEntropy C={}".format(c),
              want=L.ref64("CrossEntropy", logits, targets, weight))


@pytest.mark.parametrize("n,c,h,w", [(3, 2, 7, 9), (3, 5, 7, 9), (2, 2, 129, 129), (2, 5, 129, 129)])
def test_focal_gamma_below_one(n, c, h, w):
    """Gamma in (0, 1) only where no pixel is saturated: the reference's own gradient is NaN (inf * 0) where pt == 1."""

    logits, targets, weight = L.unsaturated_case(n, c, h, w, seed=60 + c)
    check("Focal", logits, targets, weight, gamma=0.5, what="gamma=0.5 {}x{}x{}x{}".format(n, c, h, w))


# ---- 5. saturation --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["CrossEntropy", "Focal"])
@pytest.mark.parametrize("s,m", [(1, 60), (30, 60)])
def test_saturated_pixels(s, m, name):
    """pt rounds to exactly 1 on the right pixels and to (nearly) 0 on the wrong ones: everything finite, same bars."""

    logits, targets, weight = L.saturated_case(s, m, seed=50 + s)
    check(name, logits, targets, weight, gamma=2, what="saturated s={} m={}".format(s, m))


# ---- 6. mIoU branches at more than 64 blocks per image --------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(L.MIOU_CASES))
def test_miou_branches(kind):
    from robosat_amd import ops

    logits, targets, weight = L.miou_case(kind)  # asserts the branch on the float64 reference, >= 1e-2 from the other
    check("mIoU", logits, targets, weight, what=kind, branch=L.MIOU_CASES[kind][3])
    _, stats = ops.miou_loss_fwd(logits.to(DEV), targets.to(DEV), weight.to(DEV))
    assert (float(stats[2]) > 0.5) == (L.MIOU_CASES[kind][3] == "nll")


# ---- 7. inputs the criteria accept ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", L.CRITERIA)
def test_strided_inputs_equal_contiguous_copies(name):
    """A channels-last (permuted) logits view and a targets slice of a larger tensor: same bits as their contiguous copies."""

    n, c, h, w = 2, 3, 19, 23
    g = torch.Generator().manual_seed(77)
    nhwc = (torch.randn(n, h, w, c, generator=g) * 2).to(DEV)
    big = torch.randint(0, c, (n + 2, h, w + 3), generator=g).to(DEV)
    view, tslice = nhwc.permute(0, 3, 1, 2), big[1:n + 1, :, 2:w + 2]
    assert not view.is_contiguous() and not tslice.is_contiguous()
    weight = torch.tensor([0.7, 1.3, 2.1])
    loss_v, grad_v = run_raw(name, view, tslice, weight)
    loss_c, grad_c = run_raw(name, view.contiguous(), tslice.contiguous(), weight)
    assert torch.equal(loss_v, loss_c) and torch.equal(grad_v, grad_c)
    if name == "mIoU":
        L.assert_miou_branch_is_safe(view.cpu(), tslice.cpu(), weight)
    want_loss, want_grad = L.ref64(name, view.cpu(), tslice.cpu(), weight)
    L.compare(name, loss_v.item(), grad_v.double() / UPSTREAM, want_loss, want_grad, "strided view", RECORD)


# ---- 8. determinism and workspace reuse -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", L.CRITERIA)
def test_same_bits_twice(name):
    logits, targets, weight = shape_case(3, 5, 297, 297)
    x, t = logits.to(DEV), targets.to(DEV)
    a, b = run_raw(name, x, t, weight), run_raw(name, x, t, weight)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", L.CRITERIA)
def test_small_call_after_large_call(name):
    """The workspace keeps the partial sums of the large call: the finalize kernels must read only this call's."""

    small, big = L.random_case(2, 2, 7, 9, seed=81), L.random_case(1, 8, 513, 513, seed=80)
    xs, ts = small[0].to(DEV), small[1].to(DEV)
    first = run_raw(name, xs, ts, small[2])
    run_raw(name, big[0].to(DEV), big[1].to(DEV), big[2])
    after = run_raw(name, xs, ts, small[2])
    assert torch.equal(first[0], after[0]) and torch.equal(first[1], after[1])
    L.compare(name, after[0].item(), after[1].double() / UPSTREAM, *L.ref64(name, *small), "small after large", RECORD)


# ---- single-pixel probes --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["CrossEntropy", "Focal"])
@pytest.mark.parametrize("pstar", L.NLL_PROBE_POSITIONS)
def test_nll_single_pixel_probe(pstar, name):
    """2x3x363x363 (HW = 131 769 = 514 * 256 + 185, P = 263 538): every pixel is right with margin 30 except the flat pixel
    ``pstar`` -- the first and last of a block, of an image, of the first trip of the 1 024-block loop, of the tensor -- which is
    wrong with margin 5.  The loss is that pixel's and the gradient is nonzero only there; the weight sum counts every pixel."""

    from robosat_amd import ops

    logits, targets, weight = L.nll_probe_case(pstar)
    check(name, logits, targets, weight, gamma=2, what="probe p*={}".format(pstar))
    mode = ops.NLL_CROSS_ENTROPY if name == "CrossEntropy" else ops.NLL_FOCAL
    loss, stats = ops.nll_loss_fwd(logits.to(DEV), targets.to(DEV), weight.to(DEV), mode, 2.0)
    sw = float(weight.double()[targets].sum())  # float32 weights summed in float64
    got = float(stats[1])
    print("sum of weights {!r} want {!r}: relative distance {:.2e} (one pixel is {:.1e})".format(got, sw, abs(got - sw) / sw, 1.0 / targets.numel()))
    assert abs(got - sw) <= 1e-6 * sw
    assert float(stats[0]) == float(loss)


def test_miou_single_pixel_probe():
    """2x3x129x129: class 2 occurs only at hw in {0, 255, 256, 16 383, 16 384, 16 640} of image 1 -- block borders, the last
    pixel of the first trip of the 64-block loop, the first of the second, the last of the image -- so its soft-IoU term rests
    on six pixels, each of which moves the loss by > 100 bars when left out (asserted on the reference by the builder)."""

    logits, targets, weight, _ = L.miou_probe_case()
    check("mIoU", logits, targets, weight, what="probe", branch="miou")


@pytest.mark.parametrize("n,c,h,w", L.COUNT_SHAPES)
def test_confusion_counts_and_matrix(n, c, h, w):
    """Scores on a 0.5 grid (ties: the first maximal index wins, as torch.argmax): the four counters equal the oracle's
    exactly, add to what the buffer held, and for C > 2 drop the pixels the reference's quotient drops; the C x C matrix
    equals the oracle's and accumulates over calls."""

    from robosat_amd import ops
    from robosat_amd.metrics import Metrics

    scores, targets = L.counts_case(n, c, h, w, seed=90 + c)
    want, dropped = L.counts_ref(scores, targets)
    s, t = scores.to(DEV), targets.to(DEV)
    before = [5, 6, 7, 8]
    counts = torch.tensor(before, device=DEV, dtype=torch.int64)
    ops.confusion_counts(s, t, counts)
    assert counts.tolist() == [a + b for a, b in zip(before, want)]
    ops.confusion_counts(s, t, counts)
    assert counts.tolist() == [a + 2 * b for a, b in zip(before, want)]
    assert sum(want) == n * h * w - dropped and (dropped > 0) == (c > 2)

    matrix = T.confusion_matrix(targets.numpy(), scores.numpy(), c)
    buf = torch.arange(c * c, device=DEV, dtype=torch.int64)
    ops.confusion_matrix(s, t, buf)
    assert np.array_equal(buf.cpu().numpy().reshape(c, c), matrix + np.arange(c * c).reshape(c, c))
    m = Metrics(range(c))
    m.add_batch(t, s)
    m.add(t[0], s[0])
    assert np.array_equal(m.confusion_matrix(), matrix + T.confusion_matrix(targets[:1].numpy(), scores[:1].numpy(), c))
    if c == 2:
        assert [m.tn, m.fn, m.fp, m.tp] == [a + b for a, b in zip(want, L.counts_ref(scores[:1], targets[:1])[0])]
