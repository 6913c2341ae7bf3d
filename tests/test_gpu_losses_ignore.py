"""The five losses, ``Metrics`` and ``rs_eval_confusion_ig`` with an ignore label on the MI355X, against the float64 compaction
reference of tests/ignore_ref.py under the bars each loss's own tests use (tests/losses_ref.py; tests/test_gpu_lovasz_softmax.py;
tests/lovasz_check.py with the 2e-5 / 2e-3 of tests/test_gpu_train_ops.py::test_lovasz_vs_oracle).

Every (shape, pattern) case checks, per loss: the reference; a gradient of exactly zero at the ignored pixels and finite
everywhere (pattern ``all``: loss exactly 0.0, gradient all zero); the same bits with other logits under the ignored pixels; and
for pattern ``none`` the same bits as the entry point without an ignore label."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_ref as V  # noqa: E402
import ignore_ref as I  # noqa: E402
import losses_ref as L  # noqa: E402
from lovasz_check import assert_lovasz_grad_close  # noqa: E402

from robosat_amd import losses, ops  # noqa: E402
from robosat_amd.metrics import Metrics  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IG = I.IGNORE
CASES = I.cases()
LOVASZ_LOSS_BAR, LOVASZ_GRAD_BAR = 2e-5, 2e-3  # tests/test_gpu_train_ops.py::test_lovasz_vs_oracle
SOFTMAX_BAR = 1e-5                             # tests/test_gpu_lovasz_softmax.py::test_vs_float64_truth_from_the_logits


def _dev(t):
    return None if t is None else t.to(DEV)


def _nll(name, x, t, w, ignore):
    mode = ops.NLL_CROSS_ENTROPY if name == "CrossEntropy" else ops.NLL_FOCAL
    loss, stats = ops.nll_loss_fwd(_dev(x), _dev(t), _dev(w), mode, 2.0, ignore=ignore)
    grad = ops.nll_loss_bwd(_dev(x), _dev(t), _dev(w), stats, None, mode, 2.0, ignore=ignore)
    return loss.cpu(), grad.cpu(), stats.cpu()


def _miou(x, t, w, ignore):
    loss, stats = ops.miou_loss_fwd(_dev(x), _dev(t), _dev(w), ignore=ignore)
    grad = ops.miou_loss_bwd(_dev(x), _dev(t), _dev(w), stats, None, ignore=ignore)
    return loss.cpu(), grad.cpu(), stats.cpu()


def _lovasz(x, t, ignore):
    loss, grad = ops.lovasz_fwd(_dev(x), _dev(t), want_grad=True, ignore=ignore)
    return loss.cpu(), grad.cpu()


def _softmax(x, t, per_image, classes, ignore):
    loss, grad, _ = ops.lovasz_softmax_fwd(_dev(x), _dev(t), per_image=per_image, classes=classes, want_grad=True, ignore=ignore)
    return loss.cpu(), grad.cpu()


def _common(run, run_plain, logits, targets, mask, pattern, what):
    """Assertions 2-4 of the module docstring for one loss; ``run(logits)`` -> (loss, grad) CPU tensors.  Returns that pair."""

    loss, grad = run(logits)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), what
    at_ignored = grad.permute(0, 2, 3, 1)[mask]
    assert int(torch.count_nonzero(at_ignored)) == 0, what
    assert not bool(torch.signbit(at_ignored).any()), what  # (+0.0f, not -0.0f)
    if pattern == "all":
        assert float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0, (what, float(loss))
    loss2, grad2 = run(I.other_logits_at(logits, mask))
    assert torch.equal(loss2, loss) and torch.equal(grad2, grad), what
    if pattern == "none":
        loss0, grad0 = run_plain(logits)
        assert torch.equal(loss0, loss) and torch.equal(grad0, grad), what
    return loss, grad


@pytest.mark.parametrize("case", CASES, ids=I.case_id)
@pytest.mark.parametrize("name", ["CrossEntropy", "Focal"])
def test_cross_entropy_and_focal(case, name):
    shape, pattern = case
    logits, targets, mask, weight = I.random_inputs(shape, pattern)
    for w in (None, weight):
        what = "{} {} weight={}".format(name, I.case_id(case), w is not None)
        want_loss, want_grad, _ = I.loss64(name, logits, targets, weight=w)
        loss, grad = _common(lambda x: _nll(name, x, targets, w, IG)[:2], lambda x: _nll(name, x, targets, w, None)[:2], logits, targets, mask,
                             pattern, what)
        L.compare(name, float(loss), grad, want_loss, want_grad, what)
        stats = _nll(name, logits, targets, w, IG)[2]
        valid = targets[~mask]
        den = float(valid.numel()) if w is None else float(w.double()[valid].sum())
        assert abs(float(stats[1]) - den) <= 1e-6 * max(1.0, den), what  # stats[1]: the denominator over the valid pixels


@pytest.mark.parametrize("case", CASES, ids=I.case_id)
def test_miou(case):
    shape, pattern = case
    for confident in (False, True):
        logits, targets, mask, weight = I.random_inputs(shape, pattern, confident=confident)
        for w in (None, weight):
            what = "mIoU {} confident={} weight={}".format(I.case_id(case), confident, w is not None)
            want_loss, want_grad, extras = I.loss64("mIoU", logits, targets, weight=w)
            I.assert_miou_terms_apart(extras, mask)
            loss, grad = _common(lambda x: _miou(x, targets, w, IG)[:2], lambda x: _miou(x, targets, w, None)[:2], logits, targets, mask,
                                 pattern, what)
            L.compare("mIoU", float(loss), grad, want_loss, want_grad, what)
            stats = _miou(logits, targets, w, IG)[2]
            assert float(stats[2]) == (1.0 if extras["nll"] > extras["miou"] else 0.0), what  # the branch the reference took


@pytest.mark.parametrize("case", CASES, ids=I.case_id)
def test_lovasz_hinge(case):
    shape, pattern = case
    logits, targets, mask, _ = I.random_inputs(shape, pattern)
    what = "Lovasz " + I.case_id(case)
    want_loss, want_grad, _ = I.loss64("Lovasz", logits, targets)
    loss, grad = _common(lambda x: _lovasz(x, targets, IG), lambda x: _lovasz(x, targets, None), logits, targets, mask, pattern, what)
    print("{}: loss {!r} want {!r}".format(what, float(loss), want_loss))
    assert abs(float(loss) - want_loss) <= LOVASZ_LOSS_BAR * max(1.0, abs(want_loss)), (what, float(loss), want_loss)
    # tie groups (equal fp32 errors may be visited in any order) on each image's COMPACTED pixels, where the order is what the
    # reference sorted; relative to the largest reference entry of that image
    c = shape[1]
    for i in range(shape[0]):
        keep = ~mask[i].view(-1)
        if not keep.any():
            continue
        xi = logits[i].reshape(c, -1)[:, keep].reshape(1, c, 1, -1)
        ti = targets[i].view(-1)[keep].view(1, 1, -1)
        gi, wi = (g[i].reshape(c, -1)[:, keep].reshape(1, c, 1, -1) for g in (grad, want_grad))
        assert_lovasz_grad_close(xi, ti, gi, wi, LOVASZ_GRAD_BAR, what + " image {}".format(i))


@pytest.mark.parametrize("case", CASES, ids=I.case_id)
def test_lovasz_softmax(case):
    shape, pattern = case
    logits, targets, mask = I.separated_softmax_inputs(shape, pattern)
    for per_image in (True, False):
        for classes in ("present", "all"):
            what = "LovaszSoftmax {} per_image={} classes={}".format(I.case_id(case), per_image, classes)
            want_loss, want_grad, _ = I.loss64("LovaszSoftmax", logits, targets, per_image=per_image, classes=classes)
            loss, grad = _common(lambda x: _softmax(x, targets, per_image, classes, IG), lambda x: _softmax(x, targets, per_image, classes, None),
                                 logits, targets, mask, pattern, what)
            print("{}: loss {!r} want {!r}".format(what, float(loss), want_loss))
            assert abs(float(loss) - want_loss) <= SOFTMAX_BAR * abs(want_loss), (what, float(loss), want_loss)
            scale = float(want_grad.abs().max())
            assert float((grad.double() - want_grad).abs().max()) <= SOFTMAX_BAR * scale, what


# ---- the modules ------------------------------------------------------------------------------------------------------------------
def _modules(weight, ignore_index):
    return {
        "CrossEntropy": losses.CrossEntropyLoss2d(weight=weight, ignore_index=ignore_index),
        "Focal": losses.FocalLoss2d(weight=weight, ignore_index=ignore_index),
        "mIoU": losses.mIoULoss2d(weight=weight, ignore_index=ignore_index),
        "Lovasz": losses.LovaszLoss2d(ignore_index=ignore_index),
        "LovaszSoftmax": losses.LovaszSoftmax2d(ignore_index=ignore_index),
        "LovaszSoftmaxFlatAll": losses.LovaszSoftmax2d(per_image=False, classes="all", ignore_index=ignore_index),
    }


def test_modules_scale_the_unit_gradient_and_validate_ignore_index():
    shape, pattern = (3, 4, 16, 16), "random30"
    logits, targets, mask, weight = I.random_inputs(shape, pattern)
    x, t = logits.to(DEV), targets.to(DEV)
    unit = {
        "CrossEntropy": _nll("CrossEntropy", logits, targets, weight, IG)[:2],
        "Focal": _nll("Focal", logits, targets, weight, IG)[:2],
        "mIoU": _miou(logits, targets, weight, IG)[:2],
        "Lovasz": _lovasz(logits, targets, IG),
        "LovaszSoftmax": _softmax(logits, targets, True, "present", IG),
        "LovaszSoftmaxFlatAll": _softmax(logits, targets, False, "all", IG),
    }
    for name, module in _modules(weight, IG).items():
        module = module.to(DEV)
        xr = x.clone().requires_grad_(True)
        loss = module(xr, t)
        (loss * 2.5).backward()
        assert torch.equal(loss.detach().cpu(), unit[name][0]), name
        got, want = xr.grad.cpu(), unit[name][1]
        if name in ("Lovasz", "LovaszSoftmax", "LovaszSoftmaxFlatAll"):
            assert torch.equal(got, want * 2.5), name  # (rs_scale_by_scalar of the unit gradient: one product)
        else:  # (the kernels fold grad_out into their own factor: equal to rounding)
            assert float((got - want * 2.5).abs().max()) <= 1e-6 * float(want.abs().max()) * 2.5, name
        assert int(torch.count_nonzero(got.permute(0, 2, 3, 1)[mask])) == 0, name
    for bad in (3, 0, 256, True):  # C = 4: a class index, or no byte
        for name, module in _modules(weight, bad).items():
            with pytest.raises(ValueError, match="ignore_index"):
                module.to(DEV)(x, t)
    # and None makes today's calls: labels in range, the same bits as the ops without `ignore`
    clean = L.random_case(*shape, seed=5)[1]
    for name, module in _modules(weight, None).items():
        if name == "CrossEntropy":
            assert torch.equal(module.to(DEV)(x, clean.to(DEV)).cpu(), _nll("CrossEntropy", logits, clean, weight, None)[0])


# ---- Metrics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 5, 7), (3, 4, 16, 16), (2, 8, 9, 9)], ids=lambda s: "x".join(map(str, s)))
def test_metrics_leave_labels_outside_the_classes_uncounted(shape):
    n, c, h, w = shape
    scores, targets = L.counts_case(n, c, h, w, seed=3)
    mask = I.ignored_mask("random30", targets, seed=1)
    targets = I.with_ignored(targets, mask)
    metrics = Metrics(range(c))
    metrics.add_batch(targets.to(DEV), scores.to(DEV))
    pred = torch.argmax(scores, 1)  # (the first maximal index, as the kernel)
    want = np.zeros((c, c), dtype=np.int64)
    np.add.at(want, (targets[~mask].numpy(), pred[~mask].numpy()), 1)
    got = metrics.confusion_matrix()
    assert got.tolist() == want.tolist() and int(got.sum()) == int((~mask).sum()) < n * h * w


# ---- rs_eval_confusion_ig -------------------------------------------------------------------------------------------------------------
def _confusion_ig(predicted, actual, classes, ignore):
    """numpy: (counts [B, C, C], bad [B], ignored [B]) per tile, by the definition in include/robosat_hip.h."""

    b = predicted.shape[0]
    counts, bad, ignored = np.zeros((b, classes, classes), dtype=np.int64), np.zeros(b, dtype=np.int64), np.zeros(b, dtype=np.int64)
    for g in range(b):
        p, a = predicted[g].reshape(-1).astype(np.int64), actual[g].reshape(-1).astype(np.int64)
        is_bad = (p >= classes) | ((a >= classes) & (a != ignore))
        is_ignored = ~is_bad & (a == ignore)
        cell = ~is_bad & ~is_ignored
        np.add.at(counts[g], (a[cell], p[cell]), 1)
        bad[g], ignored[g] = int(is_bad.sum()), int(is_ignored.sum())
    return counts, bad, ignored


def _eval_case(b, h, w, classes, seed, bad_bytes):
    rng = np.random.default_rng(seed)
    predicted = rng.integers(0, classes, size=(b, h, w)).astype(np.uint8)
    actual = rng.integers(0, classes, size=(b, h, w)).astype(np.uint8)
    actual[rng.random((b, h, w)) < 0.3] = IG
    actual[-1] = IG  # one tile wholly ignored
    if bad_bytes:
        predicted[0, 0, :3] = classes  # a mask byte that is no class: bad, whatever the label says
        actual[0, 0, :2] = IG
        actual[0, -1, -1] = classes + 1  # a label byte that is neither a class nor `ignore` (not in the last tile: it stays wholly ignored)
    return predicted, actual


@pytest.mark.parametrize("b,h,w,classes,bad_bytes", [(5, 7, 9, 3, True), (3, 64, 64, 2, False), (2, 96, 100, 8, True)],
                         ids=["5x7x9-many-groups-per-block", "3x64x64-one-group-per-block", "2x96x100-blocks-straddle"])
def test_eval_confusion_with_an_ignore_label(b, h, w, classes, bad_bytes):
    predicted, actual = _eval_case(b, h, w, classes, seed=b + classes, bad_bytes=bad_bytes)
    want_counts, want_bad, want_ignored = _confusion_ig(predicted, actual, classes, IG)
    assert want_ignored[-1] == h * w and want_counts[-1].sum() == 0 and (want_bad.sum() > 0) == bad_bytes
    p, a = torch.from_numpy(predicted).to(DEV), torch.from_numpy(actual).to(DEV)
    counts, bad, ignored = ops.mask_confusion(p, a, classes, ignore=IG)
    assert counts.cpu().numpy().tolist() == want_counts.tolist()
    assert bad.cpu().tolist() == want_bad.tolist() and ignored.cpu().tolist() == want_ignored.tolist()
    counts, bad, ignored = ops.mask_confusion(p, a, classes, stitched=True, ignore=IG)
    assert counts.cpu().numpy()[0].tolist() == want_counts.sum(0).tolist()
    assert bad.cpu().tolist() == [int(want_bad.sum())] and ignored.cpu().tolist() == [int(want_ignored.sum())]
    # an unaligned base address: views one byte into a larger buffer (the single checked loads)
    flat_p, flat_a = torch.zeros(p.numel() + 1, dtype=torch.uint8, device=DEV), torch.zeros(a.numel() + 1, dtype=torch.uint8, device=DEV)
    flat_p[1:] = p.view(-1)
    flat_a[1:] = a.view(-1)
    pv, av = flat_p[1:].view(b, h, w), flat_a[1:].view(b, h, w)
    assert pv.data_ptr() % 16 != 0 or av.data_ptr() % 16 != 0
    counts, bad, ignored = ops.mask_confusion(pv, av, classes, ignore=IG)
    assert counts.cpu().numpy().tolist() == want_counts.tolist() and ignored.cpu().tolist() == want_ignored.tolist()
    assert bad.cpu().tolist() == want_bad.tolist()
    # where no label is ignored, cells and bad are the base call's
    clean = np.where(actual == IG, 0, actual).astype(np.uint8)
    c0, b0 = ops.mask_confusion(p, torch.from_numpy(clean).to(DEV), classes)
    c1, b1, i1 = ops.mask_confusion(p, torch.from_numpy(clean).to(DEV), classes, ignore=IG)
    assert torch.equal(c0, c1) and torch.equal(b0, b1) and int(i1.sum()) == 0
    ref_counts, ref_bad = V.confusion(predicted, clean, classes)
    assert c0.cpu().numpy().tolist() == np.asarray(ref_counts).tolist() and b0.cpu().tolist() == np.asarray(ref_bad).tolist()
    with pytest.raises(ValueError):
        ops.mask_confusion(p, a, classes, ignore=classes - 1)
