"""The boundary weight on the MI355X: ``ops.boundary_weight_plane`` (``rs_boundary_weight_plane``) against the numpy reference of
tests/boundary_ref.py with ``torch.equal`` -- the plane is defined bit for bit -- and the weighted CrossEntropy / Focal
(``rs_nll_loss_*_pw``) against float64 (``losses_ref.nll_family64(mult=plane)``) under the bars of the plain losses' tests
(``losses_ref.LOSS_BAR``, ``GRAD_BAR``: a per-pixel weight is the ``mult`` those bars were set for).

The float64 side always uses the REFERENCE plane, never the device's."""

import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as B  # noqa: E402
import losses_ref as L  # noqa: E402

from robosat_amd import _lib, losses, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IG = B.IGNORE
MODES = {"CrossEntropy": ops.NLL_CROSS_ENTROPY, "Focal": ops.NLL_FOCAL}
W0 = 4.0


def _dev(t):
    return None if t is None else t.to(DEV)


def _plane(targets, sigma, ignore=None, classes=None, w0=W0):
    return ops.boundary_weight_plane(_dev(targets), w0, sigma, ignore=ignore, classes=classes).cpu()


def _run(name, x, t, w, plane, ignore=None, gout=None):
    """(loss, gradient, stats) as CPU tensors through the general ``pixel_weight`` argument."""

    xd, td, wd, pd = _dev(x), _dev(t), _dev(w), _dev(plane)
    loss, stats = ops.nll_loss_fwd(xd, td, wd, MODES[name], 2.0, ignore=ignore, pixel_weight=pd)
    kept = stats.clone()
    grad = ops.nll_loss_bwd(xd, td, wd, stats, _dev(gout), MODES[name], 2.0, ignore=ignore, pixel_weight=pd)
    return loss.cpu(), grad.cpu(), kept.cpu()


# ---- the plane ----------------------------------------------------------------------------------------------------------------------
def _check_plane(targets, sigma, ignore=None, classes=None):
    want = B.plane(targets, W0, sigma, ignore)
    got = _plane(targets, sigma, ignore, classes)
    assert got.dtype == torch.float32 and got.shape == targets.shape
    assert torch.equal(got, want), "{} of {} pixels differ".format(int((got != want).sum()), want.numel())
    return got


@pytest.mark.parametrize("h, w, sigma", [(24, 20, 1.0), (40, 48, 1.5), (70, 66, 3.0), (130, 66, 3.0)])
@pytest.mark.parametrize("ignore", [False, True])
def test_the_plane_of_the_standard_raster(h, w, sigma, ignore):
    """Widths that are no multiple of 32 or 64; 130 rows are three strips of the column pass."""

    if (h, w) == (130, 66):
        t = torch.from_numpy(B.standard_raster(h, w, ignore)[None])
    else:
        t, _ = B.standard_case(h, w, sigma, ignore=ignore)  # (asserts both kinds of pixel on the reference)
    got = _check_plane(t, sigma, IG if ignore else None, classes=3)
    if ignore:
        assert (got[t == IG] == 0).all() and (got[t != IG] >= 1).all()
        assert not torch.signbit(got[t == IG]).any()


@pytest.mark.parametrize("h, w, sigma", [(5, 7, 2.0), (1, 9, 1.0), (9, 1, 1.0), (1, 1, 1.0), (2, 2, 0.2)])
def test_the_plane_of_rasters_smaller_than_the_reach(h, w, sigma):
    """H < R and W < R; one row; one column; one pixel; reach 1."""

    rng = np.random.RandomState(h * 10 + w)
    t = torch.from_numpy(rng.randint(0, 3, size=(2, h, w)).astype(np.int64))
    t[1, :, w // 2:] = t[1, 0, 0]
    _check_plane(t, sigma)
    t[0, h // 2, w // 2] = IG
    _check_plane(t, sigma, IG)


def test_the_plane_at_the_largest_reach():
    """R = 128 (sigma 42.6) on 40 x 300: two chunks either side in the row pass, every row in reach of every other."""

    assert B.reach(42.6) == 128
    t = np.zeros((1, 40, 300), dtype=np.int64)
    t[0, 10:30, 120:180] = 1  # (at most 119 columns and 10 rows from any pixel)
    got = _check_plane(torch.from_numpy(t), 42.6)
    assert float(got.min()) > 1.0 and (got[0, :, 0] < got[0, :, 100]).all()  # (no pixel is out of reach here)
    t = np.zeros((1, 40, 300), dtype=np.int64)
    t[0, :, 299] = 1  # the boundary at the right end: the left 171 columns are beyond it
    got = _check_plane(torch.from_numpy(t), 42.6)
    assert (got[0, :, :170] == 1).all() and (got[0, :, 172:] > 1).all()


@pytest.mark.parametrize("classes", [2, 8])
def test_the_plane_at_both_ends_of_the_class_count(classes):
    rng = np.random.RandomState(classes)
    coarse = rng.randint(0, classes, size=(2, 9, 11))
    t = torch.from_numpy(np.repeat(np.repeat(coarse, 5, 1), 5, 2)[:, :43, :53].astype(np.int64)).contiguous()
    _check_plane(t, 1.5, classes=classes)
    t[:, 7:23, 12:31] = classes  # the smallest ignore label there is
    _check_plane(t, 1.5, classes, classes=classes)
    t[t == classes] = IG
    _check_plane(t, 1.5, IG, classes=classes)


def test_images_never_see_each_other():
    """N = 3: image 0 has a boundary on its last row, image 1 is constant -- all 1.0f, or a distance crossed over from image 0 or 2
    -- and image 2 is the ignore variant with a boundary on its first row."""

    h, w, sigma = 40, 48, 1.5
    a = B.standard_raster(h, w)
    a[h - 1, : w // 2] = 2
    c = B.standard_raster(h, w, ignore=True)
    c[0, : w // 2] = 2
    t = torch.from_numpy(np.stack([a, np.ones((h, w), dtype=np.int64), c]))
    got = _check_plane(t, sigma, IG, classes=3)
    assert (got[1] == 1).all() and (got[0, h - 1, : w // 2] > 1).all() and (got[2, 0, : w // 2] > 1).all()


def test_a_raster_that_is_all_ignored_weighs_nothing():
    t = torch.full((2, 17, 33), IG, dtype=torch.int64)
    got = _check_plane(t, 3.0, IG, classes=2)
    assert int(torch.count_nonzero(got)) == 0 and not torch.signbit(got).any()


def test_the_plane_is_the_same_bits_in_every_run_and_the_table_is_cached():
    t, _ = B.standard_case(70, 66, 3.0, ignore=True)
    first = _plane(t, 3.0, IG, 3)
    table = ops._BOUNDARY_TABLES[(W0, 3.0, DEV)]
    assert torch.equal(_plane(t, 3.0, IG, 3), first)
    assert ops._BOUNDARY_TABLES[(W0, 3.0, DEV)] is table
    assert table.dtype == torch.float32 and table.cpu().numpy().tobytes() == B.table(W0, 3.0).tobytes()
    assert not torch.equal(_plane(t, 3.0, IG, 3, w0=2.0), first)


# ---- loss and gradient against float64 ------------------------------------------------------------------------------------------------
SIZES = {"5px": (1, 5), "255px": (15, 17), "256px": (16, 16), "257px": (1, 257), "513x513": (513, 513)}


def _sized_targets(h, w, ignore):
    """int64 [1, h, w] in 3 classes: the standard raster at 513 x 513, else runs of 3 pixels of a seeded coarse grid (a boundary
    every few pixels); ``ignore``: a 255 block inside."""

    if (h, w) == (513, 513):
        return torch.from_numpy(B.standard_raster(h, w, ignore)[None])
    if (h, w) == (1, 5):
        return torch.tensor([[[0, IG if ignore else 0, 1, 1, 2]]])
    g = torch.Generator().manual_seed(h * 1000 + w)
    coarse = torch.randint(0, 3, (1, (h + 2) // 3, (w + 2) // 3), generator=g)
    t = coarse.repeat_interleave(3, 1).repeat_interleave(3, 2)[:, :h, :w].contiguous()
    if ignore:
        t[:, h // 3:h // 3 + max(1, h // 4), w // 4:w // 4 + max(1, w // 3)] = IG
    return t


@pytest.fixture(scope="module")
def sized():
    """Per (size, ignore): targets, logits, class weight and the REFERENCE plane, made once."""

    out = {}
    for key, (h, w) in SIZES.items():
        for ignore in (False, True):
            t = _sized_targets(h, w, ignore)
            x, cw = B.logits_for(t, 3, seed=7 + h)
            m = B.plane(t, W0, 1.5, IG if ignore else None)
            valid = t != IG
            assert bool((m[valid] > 1).any()) and bool((m[~valid] == 0).all()) and bool((~valid).any()) == ignore
            out[(key, ignore)] = (t, x, cw, m)
    return out


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("ignore", [False, True], ids=["plain", "ignore"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "class-weights"])
@pytest.mark.parametrize("name", list(MODES))
def test_loss_and_gradient_with_a_device_made_plane(sized, name, weighted, ignore, size):
    """5 pixels; 255, 256 and 257 (one block less one, one block, one block and one); 263 169 (past the 1024 x 256 grid-stride border)."""

    t, x, cw, ref_plane = sized[(size, ignore)]
    w = cw if weighted else None
    ig = IG if ignore else None
    plane = _plane(t, 1.5, ig, 3)
    assert torch.equal(plane, ref_plane)
    loss, grad, stats = _run(name, x, t, w, plane, ig)
    want_loss, want_grad, want_den = B.loss64(name, x, t, w, ref_plane, ig)
    L.compare(name, loss, grad, want_loss, want_grad, what="{} {} {}".format(size, "w" if weighted else "-", "ig" if ignore else "-"))
    assert float(stats[0]) == float(loss)
    assert abs(float(stats[1]) - want_den) <= 1e-6 * want_den  # (a double sum rounded once to float32: 6e-8)
    if ignore:
        at = grad.permute(0, 2, 3, 1)[t == IG]
        assert int(torch.count_nonzero(at)) == 0 and not torch.signbit(at).any()  # +0.0f in every class plane


@pytest.fixture(scope="module")
def big():
    """1 x 3 x 513 x 513 random logits, labels and class weights, on the host and on the device."""

    x, t, w = L.random_case(1, 3, 513, 513, seed=77)
    return {"x": x, "t": t, "w": w, "xd": _dev(x), "td": _dev(t), "wd": _dev(w)}


PROBES = (0, 255, 256, 262143, 262144, 513 * 513 - 1)


@pytest.mark.parametrize("p", PROBES)
@pytest.mark.parametrize("name", list(MODES))
def test_a_plane_that_is_zero_except_at_one_pixel(big, name, p):
    """Through the general ``pixel_weight`` argument: the loss is pixel p's own (its weights cancel), the gradient is its own and
    exactly zero elsewhere -- a pixel dropped or doubled at a block or loop border cannot hide in a mean over 263 169 pixels."""

    x, t, w = big["x"], big["t"], big["w"]
    hw = 513 * 513
    plane = torch.zeros(1, 513, 513)
    plane.view(-1)[p] = 2.5
    pd = _dev(plane)
    loss, stats = ops.nll_loss_fwd(big["xd"], big["td"], big["wd"], MODES[name], 2.0, pixel_weight=pd)
    grad = ops.nll_loss_bwd(big["xd"], big["td"], big["wd"], stats, None, MODES[name], 2.0, pixel_weight=pd).cpu()
    xp = x.view(1, 3, hw)[:, :, p].reshape(1, 3, 1, 1)
    tp = t.view(1, hw)[:, p].reshape(1, 1, 1)
    want_loss, want_grad, want_den = L.nll_family64(name, xp, tp, w, mult=torch.full((1, 1, 1), 2.5))
    L.compare(name, loss.cpu(), grad.view(1, 3, hw)[:, :, p].reshape(1, 3, 1, 1), want_loss, want_grad, what="probe {}".format(p))
    assert abs(float(stats[1]) - want_den) <= 1e-6 * want_den
    assert int(torch.count_nonzero(grad.view(1, 3, hw)[:, :, p])) == 3
    rest = grad.view(1, 3, hw).clone()
    rest[:, :, p] = 0
    assert int(torch.count_nonzero(rest)) == 0


@pytest.mark.parametrize("name", list(MODES))
def test_a_plane_of_ones_gives_the_base_calls(big, name):
    """Within the bars of the float64 reference, as asked -- and in fact BIT-EQUAL to ``rs_nll_loss_fwd / bwd`` (asserted): 1.0f * w is
    w, and the sums run in the same order."""

    xd, td, wd = big["xd"], big["td"], big["wd"]
    ones = torch.ones(1, 513, 513, device=DEV)
    for w in (None, wd):
        base_loss, base_stats = ops.nll_loss_fwd(xd, td, w, MODES[name], 2.0)
        base_grad = ops.nll_loss_bwd(xd, td, w, base_stats, None, MODES[name], 2.0)
        loss, stats = ops.nll_loss_fwd(xd, td, w, MODES[name], 2.0, pixel_weight=ones)
        grad = ops.nll_loss_bwd(xd, td, w, stats, None, MODES[name], 2.0, pixel_weight=ones)
        want_loss, want_grad = L.ref64(name, big["x"], big["t"], None if w is None else big["w"])
        L.compare(name, loss.cpu(), grad.cpu(), want_loss, want_grad, what="ones")
        assert torch.equal(loss, base_loss) and torch.equal(stats, base_stats) and torch.equal(grad, base_grad)


@pytest.mark.parametrize("name", list(MODES))
def test_ignored_pixels_reach_nothing(name):
    t, ref_plane = B.standard_case(70, 66, 3.0, ignore=True)
    x, w = B.logits_for(t, 3, seed=3)
    plane = _plane(t, 3.0, IG, 3)
    loss, grad, stats = _run(name, x, t, w, plane, IG)
    at = grad.permute(0, 2, 3, 1)[t == IG]
    assert int(torch.count_nonzero(at)) == 0 and not torch.signbit(at).any()
    other = x.clone()
    other.permute(0, 2, 3, 1)[t == IG] = torch.tensor([1e4, -3e4, 7.0])
    loss2, grad2, stats2 = _run(name, other, t, w, _plane(t, 3.0, IG, 3), IG)
    assert torch.equal(loss2, loss) and torch.equal(grad2, grad) and torch.equal(stats2, stats)
    # two runs: the same bits
    loss3, grad3, stats3 = _run(name, x, t, w, plane, IG)
    assert torch.equal(loss3, loss) and torch.equal(grad3, grad) and torch.equal(stats3, stats)
    # every pixel ignored: loss 0, gradient 0, denominator 0
    none = torch.full_like(t, IG)
    loss0, grad0, stats0 = _run(name, x, none, w, _plane(none, 3.0, IG, 3), IG)
    assert float(loss0) == 0.0 and float(stats0[1]) == 0.0 and int(torch.count_nonzero(grad0)) == 0 and not torch.signbit(grad0).any()
    # and a plane of zeros over valid pixels likewise
    loss0, grad0, stats0 = _run(name, x, t, w, torch.zeros_like(plane), IG)
    assert float(loss0) == 0.0 and float(stats0[1]) == 0.0 and int(torch.count_nonzero(grad0)) == 0


@pytest.mark.parametrize("name", list(MODES))
def test_shards_add_up_to_the_whole_batch(name):
    """N = 4 split 2 + 2: sum_r loss_r * stats_r[1] = loss * stats[1] -- the identity the data-parallel exchange of the one scalar
    stats[1] rests on (``_global_batch_normaliser``)."""

    rows = [B.standard_raster(40, 48), B.standard_raster(40, 48, ignore=True), np.ones((40, 48), dtype=np.int64),
            B.standard_raster(40, 48)[::-1].copy()]
    t = torch.from_numpy(np.stack(rows))
    x, w = B.logits_for(t, 3, seed=11)
    plane = _plane(t, 1.5, IG, 3)
    assert torch.equal(plane, B.plane(t, W0, 1.5, IG))
    loss, _, stats = _run(name, x, t, w, plane, IG)
    parts = 0.0
    for lo in (0, 2):
        sub = _plane(t[lo:lo + 2].contiguous(), 1.5, IG, 3)
        assert torch.equal(sub, plane[lo:lo + 2])  # (an image's plane does not depend on its batch)
        l, _, s = _run(name, x[lo:lo + 2].contiguous(), t[lo:lo + 2].contiguous(), w, sub, IG)
        parts += float(l) * float(s[1])
    whole = float(loss) * float(stats[1])
    assert abs(parts - whole) <= L.LOSS_BAR * abs(whole), (parts, whole)


# ---- the modules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("ignore", [False, True], ids=["plain", "ignore"])
def test_modules_through_autograd(name, ignore):
    t, _ = B.standard_case(70, 66, 3.0, ignore=ignore)
    t = torch.cat([t, torch.from_numpy(B.standard_raster(70, 66)[None, ::-1].copy())])
    x, w = B.logits_for(t, 3, seed=13)
    ig = IG if ignore else None
    cls = losses.CrossEntropyLoss2d if name == "CrossEntropy" else losses.FocalLoss2d
    crit = cls(weight=w, ignore_index=ig, boundary=(4, 3)).to(DEV)
    xd = _dev(x).requires_grad_(True)
    loss = crit(xd, _dev(t))
    (loss * 0.5).backward()  # grad_out = 0.5
    want_loss, want_grad, _ = B.loss64(name, x, t, w, B.plane(t, 4.0, 3.0, ig), ig)
    L.compare(name, loss.detach().cpu(), xd.grad.cpu(), want_loss, 0.5 * want_grad, what="module")
    # boundary=None: the calls the module makes today, bit for bit
    plain = cls(weight=w, ignore_index=ig).to(DEV)
    assert plain.boundary is None
    xp = _dev(x).requires_grad_(True)
    got = plain(xp, _dev(t))
    got.backward()
    base_loss, base_stats = ops.nll_loss_fwd(_dev(x), _dev(t), _dev(w), MODES[name], 2.0, ignore=ig)
    base_grad = ops.nll_loss_bwd(_dev(x), _dev(t), _dev(w), base_stats, torch.ones((), device=DEV), MODES[name], 2.0, ignore=ig)
    assert torch.equal(got.detach(), base_loss) and torch.equal(xp.grad, base_grad)
    assert abs(float(got.detach()) - float(loss.detach())) > 1e-4  # (and the plane matters on this case)


def test_forward_and_backward_capture_into_a_graph():
    """No host synchronisation: plane, forward and backward captured into one graph, replayed twice, give the eager bits."""

    t, _ = B.standard_case(70, 66, 3.0, ignore=True)
    x, w = B.logits_for(t, 3, seed=17)
    xd, td, wd = _dev(x), _dev(t), _dev(w)
    gout = torch.full((), 0.5, device=DEV)

    def step():
        plane = ops.boundary_weight_plane(td, W0, 3.0, ignore=IG, classes=3)
        loss, stats = ops.nll_loss_fwd(xd, td, wd, ops.NLL_FOCAL, 2.0, ignore=IG, pixel_weight=plane)
        return loss, ops.nll_loss_bwd(xd, td, wd, stats, gout, ops.NLL_FOCAL, 2.0, ignore=IG, pixel_weight=plane)

    loss, grad = step()
    eager_loss, eager_grad = loss.clone(), grad.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (the table and the stream's workspace exist before the capture)
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g_loss, g_grad = step()
    for _ in range(2):
        g_loss.zero_()
        g_grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_loss, eager_loss) and torch.equal(g_grad, eager_grad)


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    lib = _lib.lib()
    n, c, h, w = 2, 3, 6, 7
    t = torch.zeros(n, h, w, dtype=torch.int64, device=DEV)
    x = torch.zeros(n, c, h, w, device=DEV)
    plane, dx = torch.ones(n, h, w, device=DEV), torch.empty(n, c, h, w, device=DEV)
    table = torch.ones(128 * 128, device=DEV)
    loss, stats = torch.zeros((), device=DEV), torch.ones(2, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def make(n=n, c=c, h=h, w=w, r=3, ignore=-1):
        return lib.rs_boundary_weight_plane(ptr(t), ptr(table), ptr(plane), n, c, h, w, r, ignore, ptr(ws), stream)

    def fwd(n=n, c=c, h=h, w=w, ignore=-1):
        return lib.rs_nll_loss_fwd_pw(ptr(x), ptr(t), None, ptr(loss), ptr(stats), n, c, h, w, 0, ctypes.c_float(2.0), ptr(ws), stream,
                                      ptr(plane), ignore)

    def bwd(n=n, c=c, h=h, w=w, ignore=-1):
        return lib.rs_nll_loss_bwd_pw(ptr(x), ptr(t), None, ptr(stats), None, ptr(dx), n, c, h, w, 0, ctypes.c_float(2.0), stream,
                                      ptr(plane), ignore)

    for call in (make, fwd, bwd):
        assert call() == 0 and call(ignore=255) == 0 and call(ignore=c) == 0
        for bad in ({"c": 0}, {"c": 9}, {"c": -1}, {"ignore": c - 1}, {"ignore": 0}, {"ignore": 256}, {"ignore": -2},
                    {"n": 0}, {"h": 0}, {"w": 0}, {"n": -1}, {"h": -3}, {"w": -1}):
            assert call(**bad) == _lib.RS_EINVAL, (call.__name__, bad)
    assert make(r=1) == 0 and make(r=128) == 0
    for r in (0, -1, 129, 1 << 20):
        assert make(r=r) == _lib.RS_EINVAL
    assert make(c=8, ignore=8) == 0 and make(c=8, ignore=7) == _lib.RS_EINVAL
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.boundary_weight_plane(t, 4.0, 42.7)
    with pytest.raises(ValueError):
        ops.boundary_weight_plane(t, 0.0, 3.0)
    with pytest.raises(ValueError):
        ops.boundary_weight_plane(t, 4.0, 3.0, ignore=2, classes=3)
