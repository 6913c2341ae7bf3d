"""``ops.prob_histogram`` (``rs_eval_prob_hist``, csrc/evaluate.hip) and ``rs_softvote_masks_threshold`` (csrc/postproc.hip) on the
MI355X against numpy (tests/prob_ref.py: ``np.bincount``; ``np.average(...) >= T``).  Every value is an integer or a byte, so every
comparison is equality.  The shapes are the smallest at which the kernel can go wrong: one pixel, groups that begin at odd byte
offsets (7 x 9 = 63), many groups in one block (5 x 5), exactly a block (64 x 64), a second block of one pixel (1 x 4097), a block
across a tile border (70 x 70), rasters at odd addresses, and the two ends of the load: every pixel of a tile in one bin, and all
512 bins filled."""

import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prob_ref as P  # noqa: E402

from robosat_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK = 4096
SHAPES = [(3, 7, 9), (1, 64, 64), (1, 1, 4097), (1, 1, 1), (40, 5, 5), (2, 70, 70)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
BAD = 9  # a label byte that is no class of up to 8 and not the ignore value


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _borders(shape):
    """The first pixel of every group and of every block, and the end of the call: flat indices in 0 .. pixels."""

    pixels, group = shape[0] * shape[1] * shape[2], shape[1] * shape[2]
    return sorted(set(range(0, pixels + 1, group)) | set(range(0, pixels, BLOCK)) | {pixels})


def _rasters(shape, classes, seed, marks=None):
    """Random bytes and random labels; with ``marks`` = (left, right) those two label bytes on the two sides of every border."""

    rng = np.random.RandomState(seed)
    prob = rng.randint(0, 256, size=shape).astype(np.uint8)
    actual = rng.randint(0, classes, size=shape).astype(np.uint8)
    if marks is not None:
        flat, borders = actual.reshape(-1), _borders(shape)
        for b in borders:
            if b < flat.size:
                flat[b] = marks[1]
            if b > 0 and (b - 1) not in borders:  # (a one-pixel group keeps the mark of its own start)
                flat[b - 1] = marks[0]
    return prob, actual


def _check(prob, actual, classes, cls, stitched=False, ignore=None, tensors=None):
    """The device's histogram, twice, checked for form and against the restatement; the reference is returned."""

    dp, da = tensors if tensors is not None else (_dev(prob), _dev(actual))
    want = P.histogram(prob, actual, classes, cls, stitched=stitched, ignore=ignore)
    groups = 1 if stitched else prob.shape[0]
    for _ in range(2):
        hist, bad, ignored = ops.prob_histogram(dp, da, classes, cls, stitched=stitched, ignore=ignore)
        assert hist.dtype == torch.int64 and tuple(hist.shape) == (groups, 2, 256) and hist.is_cuda and hist.is_contiguous()
        assert bad.dtype == torch.int64 and tuple(bad.shape) == (groups,) and tuple(ignored.shape) == (groups,)
        assert torch.equal(hist.cpu(), torch.from_numpy(want[0])), np.argwhere(hist.cpu().numpy() != want[0])[:8]
        assert torch.equal(bad.cpu(), torch.from_numpy(want[1])), (bad.cpu().numpy(), want[1])
        assert torch.equal(ignored.cpu(), torch.from_numpy(want[2])), (ignored.cpu().numpy(), want[2])
    assert int(want[0].sum() + want[1].sum() + want[2].sum()) == prob.size  # every pixel is in exactly one place
    return want


@pytest.mark.parametrize("classes, cls", [(2, 1), (8, 1), (8, 7)])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_prob_histogram_is_the_bincount_per_tile(shape, classes, cls):
    prob, actual = _rasters(shape, classes, 11 * classes + cls + shape[2])
    hist, bad, ignored = _check(prob, actual, classes, cls)
    assert not bad.any() and not ignored.any() and (hist.sum(axis=(1, 2)) == shape[1] * shape[2]).all()


@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("marks", [(255, BAD), (BAD, 255)], ids=["ignored_left", "bad_left"])
@pytest.mark.parametrize("classes, cls", [(2, 1), (8, 7)])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ignored_and_bad_labels_on_both_sides_of_every_border(shape, classes, cls, marks, ignore):
    prob, actual = _rasters(shape, classes, 3 * classes + shape[1], marks)
    hist, bad, ignored = _check(prob, actual, classes, cls, ignore=ignore)
    if ignore is None:
        assert (bad > 0).all() and not ignored.any()  # without an ignore label 255 is one more bad byte
    elif shape[1] * shape[2] > 1:
        assert (bad > 0).all() and (ignored > 0).all()
    else:
        assert int(bad.sum() + ignored.sum()) == 1 and not hist.any()  # the one pixel carries the mark of its group's start


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_pixel_at_the_first_and_last_place_of_every_block_and_group(shape):
    """All (negative, byte 1) but one (positive, byte 200): the wave that holds it leaves the one-bin shortcut, the others keep it."""

    pixels = shape[0] * shape[1] * shape[2]
    probes = sorted({b for b in _borders(shape) if b < pixels} | {b - 1 for b in _borders(shape) if b > 0})
    da = torch.zeros(shape, dtype=torch.uint8, device="cuda:0")
    dp = torch.ones(shape, dtype=torch.uint8, device="cuda:0")
    for at in probes:
        prob, actual = np.ones(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
        prob.reshape(-1)[at], actual.reshape(-1)[at] = 200, 1
        da.view(-1)[at], dp.view(-1)[at] = 1, 200
        hist, _, _ = _check(prob, actual, 2, 1, tensors=(dp, da))
        da.view(-1)[at], dp.view(-1)[at] = 0, 1
        assert int(hist[:, 1, 200].sum()) == 1 and int(hist[:, 0, 1].sum()) == pixels - 1


def test_stitched_tiles_are_one_group():
    prob, actual = _rasters((3, 7, 9), 8, 4, (255, BAD))
    hist, bad, ignored = _check(prob, actual, 8, 3, stitched=True, ignore=255)
    per_tile = P.histogram(prob, actual, 8, 3, ignore=255)
    assert (hist[0] == per_tile[0].sum(axis=0)).all() and bad[0] == per_tile[1].sum() and ignored[0] == per_tile[2].sum()


@pytest.mark.parametrize("which", ["prob", "actual"])
def test_a_raster_at_an_odd_address_counts_the_same(which):
    """A view one byte into a larger buffer: no thread's 16 bytes of that raster are aligned, every load of it is the checked one."""

    shape = (2, 70, 70)
    prob, actual = _rasters(shape, 8, 21, (BAD, 255))
    n = prob.size
    store = torch.zeros(n + 16, dtype=torch.uint8, device="cuda:0")
    view = store[1:1 + n].view(shape)
    view.copy_(_dev(prob if which == "prob" else actual))
    assert view.data_ptr() % 16 == 1
    tensors = (view, _dev(actual)) if which == "prob" else (_dev(prob), view)
    _check(prob, actual, 8, 2, ignore=255, tensors=tensors)


def test_two_tiles_with_every_pixel_in_one_bin():
    shape = (2, 512, 512)
    prob, actual = np.ones(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    hist, _, _ = _check(prob, actual, 2, 1)
    assert (hist[:, 0, 1] == 262144).all() and int(hist.sum()) == 2 * 262144


def test_two_tiles_of_uniform_bytes_fill_every_bin():
    shape = (2, 512, 512)
    rng = np.random.RandomState(5)
    prob, actual = rng.randint(0, 256, size=shape).astype(np.uint8), rng.randint(0, 2, size=shape).astype(np.uint8)
    want = P.histogram(prob, actual, 2, 1)
    assert (want[0] > 0).all()  # of the input: all 512 bins of both tiles
    _check(prob, actual, 2, 1)


def test_the_outputs_share_one_buffer():
    prob, actual = _rasters((3, 7, 9), 2, 1)
    hist, bad, ignored = ops.prob_histogram(_dev(prob), _dev(actual), 2, 1)
    assert bad.data_ptr() == hist.data_ptr() + hist.numel() * 8 and ignored.data_ptr() == bad.data_ptr() + 8  # one fill


# ---- rs_softvote_masks_threshold ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", [1, 255, 257, 4097])
@pytest.mark.parametrize("weights", [None, "weights"])
@pytest.mark.parametrize("models", [1, 2, 3])
def test_the_threshold_mask_is_numpys_average_compared_with_t(models, weights, pixels):
    rng = np.random.RandomState(100 * models + pixels)
    q = rng.randint(0, 256, size=(models, pixels)).astype(np.uint8)
    q[:, 0] = 128
    w = None if weights is None else [0.5, 0.3, 1.25][:models]
    dq = _dev(q)
    # an anchor itself (with one model the mask is then `byte >= 128`), a value between two anchors, and both ends
    for t in (float(P.LIN[128]), 0.7, float(P.LIN[1]), 1.0):
        want = (np.average(P.LIN[q], axis=0, weights=w) >= t).astype(np.uint8)
        got = ops.softvote_masks(dq, w, threshold=t)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (pixels,)
        assert np.array_equal(got.cpu().numpy(), want), (t, np.flatnonzero(got.cpu().numpy() != want)[:8])
        if models == 1:
            k = int(np.searchsorted(P.LIN, t))  # the first anchor >= t
            assert np.array_equal(want, (q[0] >= k).astype(np.uint8))
    assert np.array_equal(ops.softvote_masks(dq, w).cpu().numpy(),
                          np.argmax(np.average(np.stack([1 - P.LIN[q], P.LIN[q]], axis=1), axis=0, weights=w), axis=0))  # the argmax is as it was


# ---- bad arguments -----------------------------------------------------------------------------------------------------------
EINVAL = -22


def test_prob_hist_refuses_bad_arguments():
    lib = _lib.lib()
    prob, actual = torch.zeros(126, dtype=torch.uint8, device="cuda:0"), torch.zeros(126, dtype=torch.uint8, device="cuda:0")
    out = torch.full((2 * 514 + 1,), -7, dtype=torch.int64, device="cuda:0")
    p, a, h = ctypes.c_void_p(prob.data_ptr()), ctypes.c_void_p(actual.data_ptr()), ctypes.c_void_p(out.data_ptr())
    s = ctypes.c_void_p(out.data_ptr() + 2 * 512 * 8)
    good = dict(prob=p, actual=a, hist=h, skipped=s, pixels=126, group=63, C=3, cls=1, ignore=-1)

    def call(**change):
        v = dict(good, **change)
        return lib.rs_eval_prob_hist(v["prob"], v["actual"], v["hist"], v["skipped"], v["pixels"], v["group"], v["C"], v["cls"], v["ignore"], None)

    for change in (dict(prob=None), dict(actual=None), dict(hist=None), dict(skipped=None), dict(hist=ctypes.c_void_p(out.data_ptr() + 4)),
                   dict(skipped=ctypes.c_void_p(out.data_ptr() + 2 * 512 * 8 + 4)), dict(pixels=0), dict(pixels=1 << 31), dict(group=0),
                   dict(group=64), dict(C=1), dict(C=9), dict(cls=0), dict(cls=3), dict(cls=-1), dict(ignore=-2), dict(ignore=2),
                   dict(ignore=0), dict(ignore=256)):
        assert call(**change) == EINVAL, change
    torch.cuda.synchronize()
    assert (out == -7).all()  # nothing was enqueued
    assert call() == 0 and call(ignore=3) == 0 and call(ignore=255) == 0
    torch.cuda.synchronize()
    assert out[:2 * 514].view(-1).sum() == 126 and out[0] == 63 and out[512] == 63 and out[-1] == -7


def test_softvote_threshold_refuses_bad_arguments():
    lib = _lib.lib()
    q = torch.zeros((2, 8), dtype=torch.uint8, device="cuda:0")
    out = torch.full((8,), 7, dtype=torch.uint8, device="cuda:0")
    anchors = _dev(P.LIN)
    good = dict(q=ctypes.c_void_p(q.data_ptr()), anchors=ctypes.c_void_p(anchors.data_ptr()), out=ctypes.c_void_p(out.data_ptr()), K=2, P=8, T=0.5)

    def call(**change):
        v = dict(good, **change)
        t = None if v["T"] is None else ctypes.byref(ctypes.c_double(v["T"]))  # (a double in host memory)
        return lib.rs_softvote_masks_threshold(v["q"], None, v["anchors"], v["out"], v["K"], v["P"], t, None)

    for change in (dict(q=None), dict(anchors=None), dict(out=None), dict(T=None), dict(K=0), dict(P=0), dict(T=0.0), dict(T=-0.1), dict(T=1.0000001),
                   dict(T=float("nan"))):
        assert call(**change) == EINVAL, change
    torch.cuda.synchronize()
    assert (out == 7).all()
    assert call() == 0 and call(T=1.0) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
