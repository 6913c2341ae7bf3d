"""The exact Lovasz hinge reference and its checker, without a GPU: ``lovasz_hinge_ref.hinge_exact`` IS the oracle's ``lovasz2d`` once
the oracle's sort is made stable; with an ignore label it is the float64 compaction reference of ``ignore_ref``; and
``assert_hinge_exact`` rejects the gradients a subtly wrong sort or scan would give (made here from the reference's own
pieces -- no kernel is run, let alone a broken one)."""

import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ignore_ref as I
import lovasz_hinge_ref as H
from lovasz_check import assert_lovasz_grad_close
from oracle import robosat_ref as R

SHAPES = [(2, 3, 7, 9), (3, 2, 2, 257), (4, 2, 33, 32)]  # N = 3: the 1-ulp branch of the gradient bar


def lovasz2d_stable(logits, targets):
    """``oracle.robosat_ref.lovasz2d`` with ``stable=True`` in its sort, otherwise statement for statement."""

    n, c, h, w = logits.shape
    masks = R.onehot(targets, c).view(n, -1)
    flat = logits.reshape(n, -1)
    total = 0.0
    for i in range(n):
        m = masks[i]
        err = 1.0 - (m * 2 - 1) * flat[i]
        err_sorted, order = torch.sort(err, descending=True, stable=True)
        lab = m[order]
        gts = lab.sum()
        inter = gts - lab.cumsum(0)
        union = gts + (1.0 - lab).cumsum(0)
        jac = 1.0 - inter / union
        if jac.numel() > 1:
            jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        total = total + torch.dot(F.relu(err_sorted), jac)
    return total / n


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", H.FAMILIES)
def test_hinge_exact_is_the_oracle_with_a_stable_sort(name, shape):
    x, y = H.family(name, shape, seed=sum(shape))
    xa = x.clone().requires_grad_(True)
    want = lovasz2d_stable(xa, y)
    want.backward()
    assert want.dtype == torch.float32
    loss, unit, detail = H.hinge_exact(x, y, detail=True)
    n, p = shape[0], shape[1] * shape[2] * shape[3]
    # the oracle's loss: an fp32 dot product of P non-negative terms per image (any order of additions: at most P * 2^-24 of its
    # value), an fp32 sum of N images and one division -- against the float64 sum of the same fp32 products
    bound = (p + n + 2) * 2.0 ** -24 * abs(loss)
    assert abs(want.item() - loss) <= bound, (want.item(), loss, bound)
    # autograd hands every element delta * fp32(1 / N), the arithmetic the checker's gradient rule is made for; the loss was
    # compared above with the fp32 dot product's own bound
    H.assert_hinge_exact(loss, xa.grad, loss, unit, n, detail, what="{} {}".format(name, shape))
    assert not unit[~(detail.err > 0)].any()


@pytest.mark.parametrize("case", I.cases(), ids=I.case_id)
def test_hinge_exact_with_ignore_is_the_compaction_reference(case):
    """Under the bars of tests/test_gpu_losses_ignore.py::test_lovasz_hinge (2e-5 on the loss; 2e-3 of the image's largest entry per
    tie group of its compacted pixels)."""

    shape, pattern = case
    logits, targets, mask, _ = I.random_inputs(shape, pattern)
    want_loss, want_grad, _ = I.loss64("Lovasz", logits, targets)
    loss, unit, detail = H.hinge_exact(logits, targets, ignore=I.IGNORE, detail=True)
    assert np.array_equal(detail.ignored, mask.numpy())
    grad = torch.from_numpy(unit / np.float32(shape[0]))
    assert abs(loss - want_loss) <= 2e-5 * max(1.0, abs(want_loss)), (loss, want_loss)
    at_ignored = grad.permute(0, 2, 3, 1)[mask]
    assert int(torch.count_nonzero(at_ignored)) == 0 and not bool(torch.signbit(at_ignored).any())
    if pattern == "all":
        assert loss == 0.0 and int(torch.count_nonzero(grad)) == 0
    c = shape[1]
    for i in range(shape[0]):
        keep = ~mask[i].view(-1)
        if not keep.any():
            assert int(torch.count_nonzero(grad[i])) == 0
            continue
        xi = logits[i].reshape(c, -1)[:, keep].reshape(1, c, 1, -1)
        ti = targets[i].view(-1)[keep].view(1, 1, -1)
        gi, wi = (g[i].reshape(c, -1)[:, keep].reshape(1, c, 1, -1) for g in (grad, want_grad))
        assert_lovasz_grad_close(xi, ti, gi, wi, 2e-3, "{} image {}".format(I.case_id(case), i))


def test_hinge_exact_without_ignored_pixels_is_the_plain_form():
    x, y = H.family("quant", (2, 3, 7, 9))
    plain, with_label = H.hinge_exact(x, y), H.hinge_exact(x, y, ignore=255)
    assert plain[0] == with_label[0] and np.array_equal(plain[1].view(np.int32), with_label[1].view(np.int32))


# ---- the checker rejects what a wrong kernel would write ----------------------------------------------------------------------

TIED_SHAPE = (1, 2, 32, 40)  # one image of 2560 keys: three scan chunks, forty runs of 64


class _Pieces:
    """The stable order of one image and what the deltas are made from, open to being spoiled before the gradient is formed."""

    def __init__(self, x, y):
        c = x.shape[1]
        m = (y.reshape(1, -1).numpy() == np.arange(c)[:, None]).reshape(-1)
        self.sign = np.where(m, np.float32(1), np.float32(-1))
        self.err = np.float32(1) - self.sign * x.numpy().reshape(-1)
        self.m, self.hw, self.shape = m, y.numel(), tuple(x.shape)
        self.order = np.argsort(-self.err, kind="stable")
        self.cs = np.cumsum(m[self.order].astype(np.int64))
        self.r1 = np.arange(1, m.size + 1, dtype=np.int64)

    def relabel(self):
        self.cs = np.cumsum(self.m[self.order].astype(np.int64))

    def unit(self):
        delta = H.jaccard_deltas(self.cs, self.r1, self.hw)
        e = self.err[self.order]
        out = np.empty(e.size, np.float32)
        out[self.order] = np.where(e > 0, delta, np.float32(0)) * -self.sign[self.order]
        return out.reshape(self.shape), delta


@pytest.fixture(scope="module")
def tied():
    x, y = H.family("quant", TIED_SHAPE, seed=1)
    loss, unit, detail = H.hinge_exact(x, y, detail=True)
    pieces = _Pieces(x, y)
    assert np.array_equal(pieces.unit()[0].view(np.int32), unit.view(np.int32))  # the pieces, unspoiled, are the reference
    return x, y, loss, unit, detail


def _rejected(tied, got):
    _, _, loss, unit, detail = tied
    with pytest.raises(AssertionError) as info:
        H.assert_hinge_exact(loss, got, loss, unit, 1, detail)
    text = str(info.value)
    found = re.search(r"(\d+) of \d+ gradient entries.*rank (\d+) of its image \(scan chunk (\d+)", text)
    assert found, text
    return text, int(found.group(1)), int(found.group(2)), int(found.group(3))


def test_the_checker_accepts_the_reference_itself(tied):
    _, _, loss, unit, detail = tied
    H.assert_hinge_exact(np.float32(loss), unit, loss, unit, 1, detail)
    H.assert_hinge_exact(np.float32(loss), np.where(unit == 0, np.float32(-0.0), unit), loss, unit, 1)  # -0.0 == 0.0 by value


def test_the_checker_rejects_two_tied_elements_of_different_label_swapped(tied):
    p = _Pieces(*tied[:2])
    e, lab = p.err[p.order], p.m[p.order]
    r = int(np.flatnonzero((e[:-1] == e[1:]) & (lab[:-1] != lab[1:]) & (e[:-1] > 0))[0])
    p.order[[r, r + 1]] = p.order[[r + 1, r]]
    p.relabel()
    text, count, rank, _ = _rejected(tied, p.unit()[0])
    assert count == 2 and rank in (r, r + 1) and "in a tie group" in text


def test_the_checker_rejects_ranks_shifted_by_one_inside_one_run_of_64(tied):
    p = _Pieces(*tied[:2])
    assert bool((p.err[p.order][64:129] > 0).all())
    p.r1[64:128] += 1
    _, count, rank, _ = _rejected(tied, p.unit()[0])
    assert 60 <= count <= 65 and 64 <= rank <= 128  # the run, and the neighbour whose delta spans the run's end


def test_the_checker_rejects_a_scan_chunk_whose_label_offset_is_off_by_one(tied):
    p = _Pieces(*tied[:2])
    positive = int((p.err > 0).sum())
    assert positive > 1024 + 64
    p.cs[1024:2048] += 1
    _, count, rank, chunk = _rejected(tied, p.unit()[0])
    in_chunk = min(positive, 2048) - 1024  # (the first wrong FLAT index lies anywhere in the chunk; a few deltas round alike)
    assert chunk == 1 and 1024 <= rank < 2048 and in_chunk // 2 < count <= in_chunk + 1


def test_the_checker_rejects_a_gradient_left_at_an_error_of_exactly_zero(tied):
    x, _, loss, unit, detail = tied
    p = _Pieces(*tied[:2])
    delta = p.unit()[1]
    flat = int(np.flatnonzero(p.err == 0)[0])
    rank = int(detail.rank.reshape(-1)[flat])
    got = unit.copy()
    got.reshape(-1)[flat] = -p.sign[flat] * delta[rank]  # what `err >= 0` in place of `err > 0` writes
    assert got.reshape(-1)[flat] != 0
    text, count, got_rank, _ = _rejected(tied, got)
    assert count == 1 and got_rank == rank and "error 0.0" in text


def test_the_checker_holds_ignored_pixels_to_plus_zero_and_the_loss_to_one_ulp():
    shape = (3, 2, 6, 10)
    x, y = H.family("quant", shape, seed=2)
    mask = H.ignored_mask("scattered", shape)
    y = torch.where(mask, torch.full_like(y, 255), y)
    loss, unit, detail = H.hinge_exact(x, y, ignore=255, detail=True)
    good = unit / np.float32(3)
    H.assert_hinge_exact(np.float32(loss), good, loss, unit, 3, detail)
    # N = 3: one ulp either way is the product with fp32(1 / 3); two are not
    moved = np.where(good != 0, np.nextafter(good, np.float32(np.inf)), good)
    H.assert_hinge_exact(np.float32(loss), moved, loss, unit, 3, detail)
    with pytest.raises(AssertionError, match="differ by more than 1 ulp"):
        H.assert_hinge_exact(np.float32(loss), np.where(good != 0, np.nextafter(moved, np.float32(np.inf)), good), loss, unit, 3, detail)
    minus = good.copy()
    minus[np.broadcast_to(detail.ignored[:, None], good.shape)] = np.float32(-0.0)
    with pytest.raises(AssertionError, match=r"\+0\.0 at an ignored pixel"):
        H.assert_hinge_exact(np.float32(loss), minus, loss, unit, 3, detail)
    l32 = np.float32(loss)
    up1 = np.nextafter(l32, np.float32(np.inf))
    with pytest.raises(AssertionError, match="loss"):
        H.assert_hinge_exact(np.nextafter(up1, np.float32(np.inf)), good, loss, unit, 3, detail)
    with pytest.raises(AssertionError, match="differ by more than 0 ulp"):  # a power of two: no ulp to spare
        H.assert_hinge_exact(l32, np.where(unit != 0, np.nextafter(unit, np.float32(np.inf)), unit), loss, unit, 1, detail)
