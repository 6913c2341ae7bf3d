"""Hard-pixel mining on the MI355X: the selection (``ops.hard_pixel_select`` / ``rs_hard_pixel_select``) on crafted keys against the
numpy reference of tests/hard_ref.py with ``torch.equal`` -- plane and info are defined bit for bit --, the keys made from logits
against float64 under a measured bar, and the mined CrossEntropy / Focal bit for bit against the ``_pw`` calls on the reference's
plane and under the bars of the plain losses' tests against float64.

The float64 side never sees the device's selection: where it needs the same set on both sides the case is first shown, on the float64
keys alone, to have a gap at the threshold that float32 rounding cannot close (``hard_ref.selection_is_safe``)."""

import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as B  # noqa: E402
import hard_ref as H  # noqa: E402
import losses_ref as L  # noqa: E402

from robosat_amd import _lib, losses, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IG = H.IGNORE
MODES = {"CrossEntropy": ops.NLL_CROSS_ENTROPY, "Focal": ops.NLL_FOCAL}
INF = 0x7F800000

# Largest |float32 key - float64 key| the device may show on the `random_case` inputs of `test_keys_from_logits`: four times the largest
# error recorded on the first run on the MI355X (profiles/hard_pixels/README.md: 7.94e-7, at C = 8 where the largest key is 12.35 and a
# float32 ulp 9.5e-7; 6.5e-7 and 6.7e-7 at C = 2 and 3), four for the spread over other logits of the same magnitude.
KEY_ERROR_RECORDED = 7.94e-7
KEY_BAR = 4 * KEY_ERROR_RECORDED


def _dev(t):
    return None if t is None else t.to(DEV)


def _as_i32(keys_u32):
    return torch.from_numpy(np.ascontiguousarray(keys_u32, dtype=np.uint32).view(np.int32))


def _as_u32(keys_i32):
    return keys_i32.cpu().numpy().view(np.uint32)


def _select(keys, fraction, below=None, targets=None, ignore=None, base=None):
    """The device's (plane, info) as CPU tensors for uint32 numpy keys [N, H, W]."""

    plane, info = ops.hard_pixel_select(_dev(_as_i32(keys)), fraction, below=below, targets=_dev(targets), ignore=ignore, base=_dev(base))
    return plane.cpu(), info.cpu()


def _check_select(keys, fraction, below=None, targets=None, ignore=None, base=None):
    """Plane and info equal the reference's, bit for bit; returns them."""

    valid = H.valid_of(targets, ignore) if targets is not None else np.ones(keys.shape, dtype=bool)
    want_plane, want_info = H.select(keys, valid, fraction, H.cap_of(below), None if base is None else base.numpy())
    plane, info = _select(keys, fraction, below, targets, ignore, base)
    assert plane.dtype == torch.float32 and info.dtype == torch.int64 and tuple(plane.shape) == keys.shape
    assert info.tolist() == want_info.tolist()
    assert torch.equal(plane, torch.from_numpy(want_plane)), "{} pixels differ".format(int((plane != torch.from_numpy(want_plane)).sum()))
    assert not torch.signbit(plane).any()
    return plane, info


# ---- the selection on crafted keys --------------------------------------------------------------------------------------------------
FRACTIONS = (1e-12, 0.1, 0.25, 0.5, 1.0)
SHAPES = {"1px": (1, 1), "5px": (1, 5), "255px": (15, 17), "256px": (16, 16), "257px": (1, 257), "513x513": (513, 513)}


def _distinct(rng, count):
    """``count`` distinct uint32 spread over every digit of all three rounds, in random order."""

    keys = np.unique(rng.randint(0, 1 << 32, size=count + count // 8 + 16, dtype=np.uint64).astype(np.uint32))
    assert keys.size >= count
    return rng.permutation(keys)[:count]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_distinct_keys_over_all_digits(shape):
    """1, 5, 255, 256 and 257 pixels; 513 x 513 is 129 trips of a block and more than one block per image."""

    h, w = SHAPES[shape]
    rng = np.random.RandomState(h * 1000 + w)
    keys = _distinct(rng, h * w).reshape(1, h, w)
    for fraction in FRACTIONS:
        _, info = _check_select(keys, fraction)
        assert int(info[0, 3]) == int(info[0, 1])  # no ties: exactly k are kept


@pytest.mark.parametrize("shape", ["5px", "257px", "513x513"])
def test_all_keys_equal_keeps_everything(shape):
    h, w = SHAPES[shape]
    for value in (0, 1, 0x3F800000, 0xFFFFFFFF):
        keys = np.full((1, h, w), value, dtype=np.uint32)
        for fraction in (1e-12, 0.5, 1.0):
            plane, info = _check_select(keys, fraction)
            assert info.tolist() == [[h * w, H.k_of(h * w, fraction), value, h * w]] and bool((plane == 1).all())


@pytest.mark.parametrize("where", ["last digit", "middle digit", "first digit"])
def test_keys_that_differ_in_one_digit_only(where):
    """All but the last 10 bits equal (rounds 0 and 1 see one bin, round 2 decides), all but bits 10..20, all but the first 11 bits."""

    rng = np.random.RandomState(3)
    n = 71 * 73
    if where == "last digit":
        keys = np.uint32(0xABCDE400) + (rng.randint(0, 1 << 10, size=n).astype(np.uint32))
    elif where == "middle digit":
        keys = np.uint32(0x5A600155) + (rng.randint(0, 1 << 11, size=n).astype(np.uint32) << np.uint32(10))
    else:
        keys = np.uint32(0x0012F0F1) + (rng.randint(0, 1 << 11, size=n).astype(np.uint32) << np.uint32(21))
    keys = keys.astype(np.uint32).reshape(1, 71, 73)
    for fraction in FRACTIONS:
        _check_select(keys, fraction)


def test_heavy_ties_at_the_threshold():
    """A third of the keys sit exactly at the threshold: kept > k, and every one of them is kept."""

    rng = np.random.RandomState(4)
    n = 129 * 131
    keys = _distinct(rng, n)
    order = np.sort(keys)
    tie = order[n // 2]
    keys[rng.rand(n) < 1 / 3] = tie
    keys = keys.reshape(1, 129, 131)
    k_above = int((keys > tie).sum())
    fraction = (k_above + 10) / n  # the k-th largest is among the ties
    plane, info = _check_select(keys, fraction)
    v, k, tau, kept = info[0].tolist()
    assert tau == int(tie) and kept == int((keys >= tie).sum()) and kept > k + 1000
    assert bool((plane[0][torch.from_numpy(keys[0] == tie)] == 1).all())


def test_the_extremes_are_keys_like_any_other():
    """0, the bits of +inf and 0xFFFFFFFF present; the top-1 is 0xFFFFFFFF, the whole image goes down to 0."""

    rng = np.random.RandomState(5)
    keys = _distinct(rng, 40 * 50)
    keys[:6] = (0, 0, INF, INF, 0xFFFFFFFF, 0xFFFFFFFE)
    keys = rng.permutation(keys).reshape(1, 40, 50)
    _, info = _check_select(keys, 1e-12)
    assert info[0].tolist() == [2000, 1, 0xFFFFFFFF, 1]
    _, info = _check_select(keys, 1.0)
    assert info[0].tolist() == [2000, 2000, 0, 2000]
    for fraction in (0.001, 0.3, 0.999):
        _check_select(keys, fraction)


def test_k_is_one_and_k_is_all():
    keys = _distinct(np.random.RandomState(6), 300 * 7).reshape(1, 300, 7)
    plane, info = _check_select(keys, 1e-12)
    assert info[0].tolist() == [2100, 1, int(keys.max()), 1] and int(plane.sum()) == 1
    plane, info = _check_select(keys, 1.0)
    assert info[0].tolist() == [2100, 2100, int(keys.min()), 2100] and bool((plane == 1).all())
    # and the double product at an integer, and one ulp above it (tests/test_hard_pixels_cpu.py has the host side)
    keys = _distinct(np.random.RandomState(7), 256).reshape(1, 16, 16)
    assert _check_select(keys, 0.25)[1][0, 1] == 64
    assert _check_select(keys, float(np.nextafter(0.25, 1.0)))[1][0, 1] == 65
    assert _check_select(_distinct(np.random.RandomState(8), 100).reshape(1, 10, 10), 0.07)[1][0, 1] == 8  # 0.07 * 100.0 > 7


@pytest.mark.parametrize("shape", ["257px", "513x513"])
def test_a_skewed_plane(shape):
    """99 % of the keys are 0, the others distinct: whole waves vote for one digit."""

    h, w = SHAPES[shape]
    rng = np.random.RandomState(9)
    keys = _distinct(rng, h * w)
    keys[rng.rand(h * w) < 0.99] = 0
    keys = keys.reshape(1, h, w)
    nonzero = int((keys != 0).sum())
    assert 0 < nonzero < h * w // 50
    for fraction in (1e-12, nonzero / (h * w) / 2, 0.25, 1.0):  # inside the distinct ones, and down among the zeros
        _check_select(keys, fraction)
    # and skew in the other two rounds: 99 % share everything but the last digit / sit on one value in the middle of the range
    keys2 = np.where(keys == 0, np.uint32(0x3A83126F), keys | np.uint32(0x3A800000)).astype(np.uint32)
    for fraction in (0.001, 0.5, 1.0):
        _check_select(keys2, fraction)


# ---- batches and ignored pixels ---------------------------------------------------------------------------------------------------------
def _batch_with_ignored(h=37, w=41):
    """Three images: about a third ignored, all ignored, none ignored.  Ignored pixels hold the largest keys there are (2^31
    and 0xFFFFFFFF; a pixel's key may hold anything where its label is ignored)."""

    rng = np.random.RandomState(10)
    keys = (_distinct(rng, 3 * h * w) >> np.uint32(1)).reshape(3, h, w)  # valid keys stay below 2^31, ignored ones lie above
    t = torch.from_numpy(rng.randint(0, 3, size=(3, h, w)).astype(np.int64))
    t[0][torch.from_numpy(rng.rand(h, w) < 0.35)] = IG
    t[1] = IG
    bad = (t == IG).numpy()
    keys[bad] = np.where(rng.rand(int(bad.sum())) < 0.5, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)
    return keys, t


def test_a_batch_with_different_valid_counts():
    keys, t = _batch_with_ignored()
    for fraction in (1e-12, 0.25, 1.0):
        plane, info = _check_select(keys, fraction, targets=t, ignore=IG)
        v = info[:, 0].tolist()
        assert v[1] == 0 and 0 < v[0] < v[2] == 37 * 41
        assert info[1].tolist() == [0, 0, 0, 0]
        assert int(torch.count_nonzero(plane[1])) == 0 and not torch.signbit(plane[1]).any()
        assert int(torch.count_nonzero(plane[0][t[0] == IG])) == 0  # the huge keys of ignored pixels count nowhere
        assert int(info[0, 2]) < 1 << 31
        # an image alone gives the bits it gives inside the batch, and a second run the same bits
        for i in range(3):
            alone_plane, alone_info = _select(keys[i:i + 1], fraction, targets=t[i:i + 1].contiguous(), ignore=IG)
            assert torch.equal(alone_plane[0], plane[i]) and torch.equal(alone_info[0], info[i])
        again_plane, again_info = _select(keys, fraction, targets=t, ignore=IG)
        assert torch.equal(again_plane, plane) and torch.equal(again_info, info)


def test_the_cap():
    """A cap below tau_k: more than k are kept and tau is the cap.  A cap above tau_k: nothing changes."""

    x, t, _ = L.random_case(2, 3, 33, 35, seed=12)
    keys = H.keys_u32(H.keys64(x, t))
    fraction = 0.1
    _, free = _check_select(keys, fraction)
    tau = [float(H.key_floats(np.array([u], dtype=np.uint32))[0]) for u in free[:, 2].tolist()]
    low, high = float(np.exp(-0.5 * min(tau))), float(np.exp(-2.0 * max(tau)))  # caps at tau / 2 and at 2 tau
    plane, info = _check_select(keys, fraction, below=low)
    assert info[:, 2].tolist() == [ops.hard_cap(low)] * 2 and bool((info[:, 3] > info[:, 1]).all())
    assert int(plane.sum()) == int((keys >= np.uint32(ops.hard_cap(low))).sum())
    _, info = _check_select(keys, fraction, below=high)
    assert torch.equal(info, free)


def test_the_base_plane():
    """A kept pixel carries ``base``'s bits, a dropped one +0.0f -- whatever sits in ``base`` there."""

    keys, t = _batch_with_ignored()
    rng = np.random.RandomState(13)
    base = torch.from_numpy((rng.rand(*keys.shape) * 5 + 0.25).astype(np.float32))
    base[0, 0, :5] = torch.tensor([1.0, 5e-39, 3.0e38, 0.0, 1.5])  # a subnormal and a huge weight travel as they are
    plane, info = _check_select(keys, 0.5, targets=t, ignore=IG, base=base)
    kept = plane != 0
    assert torch.equal(plane[kept], base[kept]) and int(kept.sum()) <= int(info[:, 3].sum())
    ones, _ = _check_select(keys, 0.5, targets=t, ignore=IG)
    assert torch.equal(torch.where(ones == 1, base, torch.zeros_like(base)), plane)


# ---- keys from logits ---------------------------------------------------------------------------------------------------------------
def _with_ignored(t, seed):
    g = torch.Generator().manual_seed(seed)
    t = t.clone()
    t[torch.rand(t.shape, generator=g) < 0.2] = IG
    return t


KEY_ERRORS = {}


@pytest.mark.parametrize("ignore", [False, True], ids=["plain", "ignore"])
@pytest.mark.parametrize("c", [2, 3, 8])
def test_keys_from_logits(c, ignore):
    """The selection on the device's own keys is exact; the keys lie within KEY_BAR of the float64 ones (the error is printed)."""

    x, t, _ = L.random_case(2, c, 65, 67, seed=20 + c)
    ig = IG if ignore else None
    if ignore:
        t = _with_ignored(t, c)
        x.permute(0, 2, 3, 1)[t == IG] = float("nan")  # an ignored pixel's logits reach nothing
    plane, info, keys = ops.hard_pixel_plane(_dev(x), _dev(t), 0.25, ignore=ig, want_keys=True)
    keys = _as_u32(keys)
    valid = H.valid_of(t, ig)
    want_plane, want_info = H.select(keys, valid, 0.25)
    assert torch.equal(plane.cpu(), torch.from_numpy(want_plane)) and info.cpu().tolist() == want_info.tolist()
    assert not keys[~valid].any()
    k64 = H.keys64(torch.nan_to_num(x), t, ig)
    err = float(np.abs(H.key_floats(keys) - k64)[valid].max())
    KEY_ERRORS[(c, ignore)] = err
    print("hard-pixel keys C = {} {}: largest |float32 key - float64 key| = {:.3e} (largest key {:.2f}, bar {:.1e})".format(
        c, "ignore" if ignore else "plain", err, float(k64.max()), KEY_BAR))
    assert err <= KEY_BAR
    # without the key plane: the same plane and info (the keys then live in the workspace)
    plane2, info2 = ops.hard_pixel_plane(_dev(x), _dev(t), 0.25, ignore=ig)
    assert torch.equal(plane2, plane) and torch.equal(info2, info)


# ---- loss and gradient ----------------------------------------------------------------------------------------------------------------
# (name, class weights, ignore, boundary, fraction, below, seed): seeds at which `selection_is_safe` holds (found and checked on the host;
# the third case's cap keeps 2631 and 2597 pixels where k is 1155, the fifth's lies above tau and changes nothing)
LOSS_CASES = [
    ("CrossEntropy", False, False, False, 0.25, None, 31), ("CrossEntropy", True, True, False, 0.1, None, 32),
    ("CrossEntropy", True, False, True, 0.25, 0.3, 34), ("Focal", False, True, False, 0.25, None, 31),
    ("Focal", True, False, False, 0.5, 0.2, 39), ("Focal", True, True, True, 0.25, None, 31),
]


def _loss_case(ignore, seed=31):
    t = torch.from_numpy(np.stack([B.standard_raster(70, 66, ignore), B.standard_raster(70, 66)[::-1].copy()]))
    x, w = B.logits_for(t, 3, seed=seed)
    return x, t, w


@pytest.mark.parametrize("name, weighted, ignore, boundary, fraction, below, seed", LOSS_CASES)
def test_the_mined_loss_and_gradient(name, weighted, ignore, boundary, fraction, below, seed):
    x, t, w = _loss_case(ignore, seed)
    w = w if weighted else None
    ig = IG if ignore else None
    valid = H.valid_of(t, ig)
    k64 = H.keys64(x, t, ig)
    H.selection_is_safe(k64, valid, fraction, below)  # on the reference alone; a failure here is an error of the case, not a skip
    base = B.plane(t, 4.0, 3.0, ig) if boundary else None
    cls = losses.CrossEntropyLoss2d if name == "CrossEntropy" else losses.FocalLoss2d
    crit = cls(weight=w, ignore_index=ig, boundary=(4.0, 3.0) if boundary else None, hard=fraction if below is None else (fraction, below)).to(DEV)
    assert crit.training
    xd = _dev(x).requires_grad_(True)
    loss = crit(xd, _dev(t))
    (loss * 0.5).backward()
    # bit for bit: the `_pw` calls on the plane the reference selects from the device's keys
    _, _, keys = ops.hard_pixel_plane(_dev(x), _dev(t), fraction, below=below, ignore=ig, want_keys=True)
    ref_plane, _ = H.select(_as_u32(keys), valid, fraction, H.cap_of(below), None if base is None else base.numpy())
    pd = _dev(torch.from_numpy(ref_plane))
    want, stats = ops.nll_loss_fwd(_dev(x), _dev(t), _dev(w), MODES[name], 2.0, ignore=ig, pixel_weight=pd)
    want_grad = ops.nll_loss_bwd(_dev(x), _dev(t), _dev(w), stats, torch.full((), 0.5, device=DEV), MODES[name], 2.0, ignore=ig, pixel_weight=pd)
    assert torch.equal(loss.detach(), want) and torch.equal(xd.grad, want_grad)
    # float64: the selection made from the float64 keys (the same set, by the precondition)
    plane64, info64 = H.select(H.keys_u32(k64), valid, fraction, H.cap_of(below), None if base is None else base.numpy())
    assert np.array_equal(plane64 != 0, ref_plane != 0)
    loss64, grad64, _ = H.loss64(name, x, t, w, plane64, ig)
    L.compare(name, loss.detach().cpu(), xd.grad.cpu(), loss64, 0.5 * grad64, what="hard {} {}".format(fraction, below))
    dropped = xd.grad.cpu().permute(0, 2, 3, 1)[torch.from_numpy(ref_plane == 0)]
    assert int(torch.count_nonzero(dropped)) == 0 and not torch.signbit(dropped).any()
    assert 0 < int((ref_plane != 0).sum()) < int(valid.sum())  # (something is kept and something is dropped on this case)


# ---- consistency --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODES))
def test_fraction_one_is_a_plane_of_ones_and_eval_mode_is_the_plain_criterion(name):
    x, t, w = _loss_case(True)
    cls = losses.CrossEntropyLoss2d if name == "CrossEntropy" else losses.FocalLoss2d

    def run(crit):
        xd = _dev(x).requires_grad_(True)
        loss = crit(xd, _dev(t))
        loss.backward()
        return loss.detach(), xd.grad

    ones = torch.ones(t.shape, device=DEV)
    base_loss, stats = ops.nll_loss_fwd(_dev(x), _dev(t), _dev(w), MODES[name], 2.0, ignore=IG, pixel_weight=ones)
    base_grad = ops.nll_loss_bwd(_dev(x), _dev(t), _dev(w), stats, torch.ones((), device=DEV), MODES[name], 2.0, ignore=IG, pixel_weight=ones)
    loss, grad = run(cls(weight=w, ignore_index=IG, hard=1.0).to(DEV))
    assert torch.equal(loss, base_loss) and torch.equal(grad, base_grad)
    plane, info = ops.hard_pixel_plane(_dev(x), _dev(t), 1.0, ignore=IG)
    assert torch.equal(plane.cpu(), (t != IG).float()) and torch.equal(info[:, 0], info[:, 3]) and torch.equal(info[:, 0], info[:, 1])
    # eval mode: the criterion without `hard`, bit for bit -- with and without a boundary weight
    for boundary in (None, (4.0, 3.0)):
        plain_loss, plain_grad = run(cls(weight=w, ignore_index=IG, boundary=boundary).to(DEV))
        mined = cls(weight=w, ignore_index=IG, boundary=boundary, hard=(0.1, 0.3)).to(DEV)
        train_loss, _ = run(mined)
        eval_loss, eval_grad = run(mined.eval())
        assert torch.equal(eval_loss, plain_loss) and torch.equal(eval_grad, plain_grad)
        assert abs(float(train_loss) - float(plain_loss)) > 1e-3  # (mining matters on this case)
        again, _ = run(mined.train())
        assert torch.equal(again, train_loss)


@pytest.mark.parametrize("name", list(MODES))
def test_shards_add_up_to_the_whole_batch(name):
    """N = 4 split 2 + 2: an image's plane does not depend on its batch, and sum_r loss_r * stats_r[1] = loss * stats[1] -- the identity
    the data-parallel exchange of the one scalar stats[1] rests on (``_global_batch_normaliser``)."""

    rows = [B.standard_raster(40, 48), B.standard_raster(40, 48, ignore=True), np.ones((40, 48), dtype=np.int64),
            B.standard_raster(40, 48)[::-1].copy()]
    t = torch.from_numpy(np.stack(rows))
    x, w = B.logits_for(t, 3, seed=11)
    xd, td, wd = _dev(x), _dev(t), _dev(w)
    plane, info = ops.hard_pixel_plane(xd, td, 0.25, ignore=IG)
    loss, stats = ops.nll_loss_fwd(xd, td, wd, MODES[name], 2.0, ignore=IG, pixel_weight=plane)
    parts = 0.0
    for lo in (0, 2):
        xs, ts = xd[lo:lo + 2].contiguous(), td[lo:lo + 2].contiguous()
        sub, sub_info = ops.hard_pixel_plane(xs, ts, 0.25, ignore=IG)
        assert torch.equal(sub, plane[lo:lo + 2]) and torch.equal(sub_info, info[lo:lo + 2])
        l, s = ops.nll_loss_fwd(xs, ts, wd, MODES[name], 2.0, ignore=IG, pixel_weight=sub)
        parts += float(l) * float(s[1])
    whole = float(loss) * float(stats[1])
    assert abs(parts - whole) <= L.LOSS_BAR * abs(whole), (parts, whole)


def test_forward_and_backward_capture_into_a_graph():
    """No host synchronisation: keys, selection, plane, forward and backward captured into one graph on one stream, replayed twice, give
    the eager bits."""

    x, t, w = _loss_case(True)
    xd, td, wd = _dev(x), _dev(t), _dev(w)
    gout = torch.full((), 0.5, device=DEV)

    def step():
        base = ops.boundary_weight_plane(td, 4.0, 3.0, ignore=IG, classes=3)
        plane, info = ops.hard_pixel_plane(xd, td, 0.25, below=0.3, ignore=IG, base=base)
        loss, stats = ops.nll_loss_fwd(xd, td, wd, ops.NLL_FOCAL, 2.0, ignore=IG, pixel_weight=plane)
        return loss, ops.nll_loss_bwd(xd, td, wd, stats, gout, ops.NLL_FOCAL, 2.0, ignore=IG, pixel_weight=plane), info

    loss, grad, info = step()
    eager = loss.clone(), grad.clone(), info.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (the table and the stream's workspace exist before the capture)
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = step()
    for _ in range(2):
        for out in captured:
            out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    lib = _lib.lib()
    n, c, h, w = 2, 3, 6, 7
    t = torch.zeros(n, h, w, dtype=torch.int64, device=DEV)
    x = torch.zeros(n, c, h, w, device=DEV)
    keys = torch.zeros(n, h, w, dtype=torch.int32, device=DEV)
    plane, info = torch.empty(n, h, w, device=DEV), torch.empty(n, 4, dtype=torch.int64, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.rs_hard_pixel_workspace_bytes(n, h, w) <= ws.numel() and ws.data_ptr() % 16 == 0

    bits = lambda f: struct.unpack("<q", struct.pack("<d", f))[0]  # noqa: E731  (the ABI's `fraction_bits`, unchecked)

    def make(n=n, c=c, h=h, w=w, fraction=0.25, cap=ops.HARD_NO_CAP, ignore=-1, x=x, t=t, plane=plane, info=info, ws=ws, off=0):
        return lib.rs_hard_pixel_plane(ptr(x), ptr(t), None, ptr(plane), None, ptr(info), n, c, h, w, bits(fraction), cap, ignore,
                                       None if ws is None else ctypes.c_void_p(ws.data_ptr() + off), stream)

    def select(n=n, c=c, h=h, w=w, fraction=0.25, cap=ops.HARD_NO_CAP, ignore=-1, x=keys, t=t, plane=plane, info=info, ws=ws, off=0):
        return lib.rs_hard_pixel_select(ptr(x), ptr(t), None, ptr(plane), ptr(info), n, h, w, bits(fraction), cap, ignore,
                                        None if ws is None else ctypes.c_void_p(ws.data_ptr() + off), stream)

    for call in (make, select):
        assert call() == 0 and call(ignore=255) == 0 and call(ignore=c) == 0 and call(fraction=1.0) == 0 and call(fraction=1e-300) == 0 and call(cap=0) == 0
        for bad in ({"fraction": 0.0}, {"fraction": -0.25}, {"fraction": 1.0000001}, {"fraction": float("nan")}, {"fraction": float("inf")},
                    {"fraction": -0.0}, {"cap": -1}, {"cap": 1 << 32},
                    {"ignore": 256}, {"ignore": -2}, {"n": 0}, {"h": 0}, {"w": 0}, {"n": -1}, {"h": -3}, {"w": -1},
                    {"x": None}, {"plane": None}, {"info": None}, {"ws": None}, {"off": 4}, {"off": 8}):
            assert call(**bad) == _lib.RS_EINVAL, (call.__name__, bad)
    for bad in ({"c": 0}, {"c": 9}, {"c": -1}, {"ignore": c - 1}, {"ignore": 0}, {"t": None}):
        assert make(**bad) == _lib.RS_EINVAL, bad
    assert make(c=8, ignore=8) == 0 and make(c=8, ignore=7) == _lib.RS_EINVAL
    assert select(t=None) == 0 and select(t=None, ignore=255) == _lib.RS_EINVAL  # the labels may be missing iff no label is ignored
    torch.cuda.synchronize()
    for bad in ({"fraction": 0}, {"fraction": 1.5}, {"fraction": 0.25, "below": 1.0}, {"fraction": 0.25, "below": 0}, {"fraction": 0.25, "ignore": 2}):
        with pytest.raises(ValueError):
            ops.hard_pixel_plane(x, t, **bad)
    with pytest.raises(ValueError):
        ops.hard_pixel_select(keys, 0.25, ignore=255)  # ignore without targets
    with pytest.raises(TypeError):
        ops.hard_pixel_select(keys.float(), 0.25)
