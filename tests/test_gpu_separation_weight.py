"""The separation weight on the MI355X: ``ops.separation_weight_plane`` (``rs_separation_weight_plane``) against the numpy reference of
tests/separation_ref.py with ``torch.equal`` -- the plane is defined bit for bit -- always with ``check=True`` (the labelling's error
word is read back), and the weighted CrossEntropy / Focal (``rs_nll_loss_*_pw``) against float64 (``boundary_ref.loss64``) under the
bars of the plain losses' tests, as tests/test_gpu_boundary_weight.py holds the boundary weight to them.

The float64 side always uses the REFERENCE plane, never the device's.  Every raster states on the reference what it puts to the test
(``separation_ref.exercised``) before the device is asked."""

import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as B  # noqa: E402
import losses_ref as L  # noqa: E402
import separation_ref as S  # noqa: E402

from robosat_amd import _lib, losses, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IG = S.IGNORE
MODES = {"CrossEntropy": ops.NLL_CROSS_ENTROPY, "Focal": ops.NLL_FOCAL}
WS = 10.0
SIGMAS = {1.5: 5, 5: 15, 10.6: 32}  # sigma -> reach


def _dev(t):
    return None if t is None else t.to(DEV)


def _tensor(t):
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    return t[None] if t.dim() == 2 else t


def _plane(targets, sigma, ignore=None, classes=3, base=None, ws=WS):
    return ops.separation_weight_plane(_dev(_tensor(targets)), ws, sigma, ignore=ignore, classes=classes, base=_dev(base), check=True).cpu()


def _check_plane(targets, sigma, ignore=None, classes=3, base=None):
    """The device's plane against the reference's, bit for bit; returns (plane, term > 0) of the reference."""

    t = _tensor(targets)
    want = S.plane(t, WS, sigma, classes, ignore, base)
    got = _plane(t, sigma, ignore, classes, base)
    assert got.dtype == torch.float32 and got.shape == t.shape
    assert torch.equal(got, want), "{} of {} pixels differ".format(int((got != want).sum()), want.numel())
    floor = torch.from_numpy(S.base_of(t, ignore)) if base is None else base
    return want, want != floor


def _run(name, x, t, w, plane, ignore=None, gout=None):
    """(loss, gradient, stats) as CPU tensors through the general ``pixel_weight`` argument."""

    xd, td, wd, pd = _dev(x), _dev(t), _dev(w), _dev(plane)
    loss, stats = ops.nll_loss_fwd(xd, td, wd, MODES[name], 2.0, ignore=ignore, pixel_weight=pd)
    kept = stats.clone()
    grad = ops.nll_loss_bwd(xd, td, wd, stats, _dev(gout), MODES[name], 2.0, ignore=ignore, pixel_weight=pd)
    return loss.cpu(), grad.cpu(), kept.cpu()


# ---- the plane: the standard raster ---------------------------------------------------------------------------------------------------
def test_the_reaches_under_test():
    assert {s: S.reach(s) for s in SIGMAS} == SIGMAS and ops.SEPARATION_MAX_REACH == 32
    assert [ops.separation_reach(WS, s) for s in SIGMAS] == list(SIGMAS.values())


@pytest.mark.parametrize("h, w", [(65, 65), (64, 130), (130, 63)])
@pytest.mark.parametrize("sigma", list(SIGMAS))
@pytest.mark.parametrize("ignore", [False, True], ids=["plain", "ignore"])
def test_the_plane_of_the_standard_raster(h, w, sigma, ignore):
    """Sizes that cross the 64-column chunk of the row pass and the 64-row strip of the column pass, at the reaches 5, 15 and 32."""

    t = S.standard_raster(h, w, ignore)
    ig = IG if ignore else None
    seen = S.exercised(t, sigma, 3, ig)
    assert seen["term"] > 0 and seen["far"] > 0 and seen["same"] > 0 and (seen["ignored"] > 0) == ignore, seen
    want, lit = _check_plane(t, sigma, ig)
    assert int(lit.sum()) > 0
    if ignore:
        assert (want[0][torch.from_numpy(t == IG)] == 0).all()


def test_images_never_see_each_other():
    """N = 3 with different images against three calls with N = 1: an object on an image's last row lights nothing in the next image."""

    h, w, sigma = 65, 65, 5
    a = S.standard_raster(h, w)
    a[h - 1, 10:20] = 1
    b = np.zeros((h, w), dtype=np.int64)
    b[0, 30:40] = 2  # (alone in its image: no term, whatever image 0 holds two rows away)
    c = S.standard_raster(h, w, ignore=True)[:, ::-1].copy()
    t = torch.from_numpy(np.stack([a, b, c]))
    whole = _plane(t, sigma, IG)
    for n in range(3):
        assert torch.equal(whole[n:n + 1], _plane(t[n:n + 1].contiguous(), sigma, IG))
    assert torch.equal(whole, S.plane(t, WS, sigma, 3, IG))
    assert (whole[1] == 1).all()


# ---- the plane: rasters smaller than the reach -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", [(1, 9), (1, 70), (9, 1), (70, 1), (5, 7), (1, 1), (2, 2)])
def test_the_plane_of_rasters_smaller_than_the_reach(h, w):
    """D = 32 on one row, one column (an object at both ends), 5 x 7, one pixel."""

    t = S.small_raster(h, w, seed=h * 100 + w)
    if h * w >= 9:
        assert S.exercised(t, 10.6, 3)["term"] > 0
    _check_plane(t, 10.6)
    _check_plane(t, 1.5)
    t[h // 2, w // 2] = IG
    _check_plane(t, 10.6, IG)


def test_one_column_with_an_object_at_both_ends():
    t = np.zeros((20, 1), dtype=np.int64)
    t[0, 0], t[19, 0] = 1, 2
    want, lit = _check_plane(t, 10.6)
    assert int(lit.sum()) == 18  # (a + b + isqrt(4ab) = 19^2 < 32^2 at each of them)
    assert len(set(want[0, 1:19, 0].tolist())) == 1


# ---- the plane: corridors --------------------------------------------------------------------------------------------------------------
def _three_in_a_row():
    """Row 5 holds u, v and k left to right; k's arm comes back along row 7, so from (5, 10) k is as near as u, through another row."""

    t = np.zeros((12, 30), dtype=np.int64)
    t[5, 8], t[5, 13] = 1, 1
    t[5:8, 16] = 2
    t[7, 9:17] = 2
    a, b = S.nearest_two(t, 3)
    assert (a[5, 10], b[5, 10]) == (4, 4) and int(S.objects(t > 0).max()) == 3
    return t


def _corridors():
    R = S.rectangles
    cases = {}
    for g in (1, 2, 3):
        cases["horizontal-{}".format(g)] = R(24, 40, [(4, 15, 5, 17, 1), (4, 15, 18 + g, 30, 1)])
        cases["vertical-{}".format(g)] = R(24, 40, [(3, 9, 8, 25, 1), (10 + g, 18, 8, 25, 2)])
        cases["diagonal-{}".format(g)] = R(24, 40, [(2, 9, 4, 14, 1), (10 + g, 20, 15 + g, 30, 1)])
    cases["columns-63-64"] = R(20, 100, [(4, 15, 50, 62, 1), (4, 15, 65, 80, 1)])
    cases["column-63"] = R(20, 100, [(4, 15, 50, 62, 1), (4, 15, 64, 80, 1)])
    cases["column-64"] = R(20, 100, [(4, 15, 50, 63, 1), (4, 15, 65, 80, 1)])
    cases["rows-63-64"] = R(100, 20, [(50, 62, 4, 15, 1), (65, 80, 4, 15, 1)])
    cases["row-63"] = R(100, 20, [(50, 62, 4, 15, 1), (64, 80, 4, 15, 1)])
    cases["row-64"] = R(100, 20, [(50, 63, 4, 15, 1), (65, 80, 4, 15, 1)])
    cases["three-in-a-row"] = _three_in_a_row()
    cases["equidistant"] = R(11, 21, [(5, 5, 8, 8, 1), (5, 5, 12, 12, 1)])
    cases["at-the-edge"] = R(24, 40, [(0, 5, 0, 8, 1), (0, 5, 11, 39, 2), (18, 23, 30, 39, 1)])
    cases["classes-1-and-2-touch"] = R(24, 40, [(4, 10, 4, 9, 1), (4, 10, 10, 15, 2), (4, 10, 18, 24, 1)])
    return cases


CORRIDORS = _corridors()


@pytest.mark.parametrize("case", list(CORRIDORS))
def test_corridors(case):
    """Each exact, and each with a term in it on the reference."""

    t = CORRIDORS[case]
    if case == "classes-1-and-2-touch":
        assert int(S.objects(S.classes_of(t, 3)[0]).max()) == 2  # (the touching pair is one object)
    if case == "equidistant":
        a, b = S.nearest_two(t, 3)
        assert (a[5, 10], b[5, 10]) == (4, 4)
    want, lit = _check_plane(t, 5)
    assert int(lit.sum()) > 0
    _check_plane(t, 1.5)
    _check_plane(t, 10.6)


@pytest.mark.parametrize("shape", ["U", "O"])
def test_a_courtyard_weighs_nothing(shape):
    """One object on every side: no term however narrow the courtyard is."""

    t = S.rectangles(30, 30, [(5, 24, 5, 24, 1), (8, 21, 13, 15, 0)])
    if shape == "U":
        t[5:8, 13:16] = 0
    assert S.exercised(t, 5, 3)["same"] > 0
    for sigma in SIGMAS:
        want, lit = _check_plane(t, sigma)
        assert int(lit.sum()) == 0


def test_an_ignored_band_between_two_objects():
    """The distance passes over the band; the band itself reads the base, which is 0 there."""

    t = S.rectangles(24, 40, [(4, 15, 5, 14, 1), (4, 15, 20, 30, 1), (0, 23, 16, 18, IG)])
    want, lit = _check_plane(t, 5, IG)
    band = torch.from_numpy(t == IG)
    assert (want[0][band] == 0).all() and not torch.signbit(want[0][band]).any()
    assert bool(lit[0, 10, 15]) and bool(lit[0, 10, 19])  # (either side of the band: the other object is 5 columns away, across it)
    base = torch.rand(1, 24, 40, generator=torch.Generator().manual_seed(1)) + 0.5
    want, _ = _check_plane(t, 5, IG, base=base)
    assert torch.equal(want[0][band], base[0][band])


# ---- the plane: nothing to separate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["object-free", "background-free", "one-object", "all-ignored"])
def test_with_nothing_to_separate_the_plane_is_the_base(what):
    t = np.zeros((2, 40, 70), dtype=np.int64)
    if what == "background-free":
        t[:] = 1
        t[1, :, 35:] = 2
    elif what == "one-object":
        t[:, 10:30, 20:50] = 1
    elif what == "all-ignored":
        t[:] = IG
    t[1, 3:6, 60:66] = IG
    base = torch.rand(2, 40, 70, generator=torch.Generator().manual_seed(2))
    for sigma in (1.5, 10.6):
        got = _plane(t, sigma, IG)
        assert torch.equal(got, torch.from_numpy(S.base_of(t, IG))) and not torch.signbit(got).any()
        assert torch.equal(_plane(t, sigma, IG, base=base), base)


# ---- a base plane ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore", [False, True], ids=["plain", "ignore"])
def test_the_boundary_plane_as_the_base(ignore):
    """Reference boundary plane + reference term, one float32 addition; the device makes both planes itself."""

    t = _tensor(S.standard_raster(65, 65, ignore))
    ig = IG if ignore else None
    ref_base = B.plane(t, 4.0, 3.0, ig)
    want = S.plane(t, WS, 5, 3, ig, base=ref_base)
    base = ops.boundary_weight_plane(_dev(t), 4.0, 3.0, ignore=ig, classes=3)
    assert torch.equal(base.cpu(), ref_base)
    got = ops.separation_weight_plane(_dev(t), WS, 5, ignore=ig, classes=3, base=base, check=True).cpu()
    assert torch.equal(got, want) and bool((got > ref_base).any())
    assert torch.equal(base.cpu(), ref_base)  # (the base is read, never written)


def test_a_random_base_stays_bit_exact_where_the_term_is_zero():
    t = _tensor(S.standard_raster(64, 130, True))
    base = torch.rand(1, 64, 130, generator=torch.Generator().manual_seed(3)) * 3.0
    base[0, ::7, ::5] = 0.0
    want, lit = _check_plane(t, 5, IG, base=base)
    assert 0 < int(lit.sum()) < lit.numel()
    got = _plane(t, 5, IG, base=base)
    assert torch.equal(got[~lit], base[~lit])
    term = torch.from_numpy(S.term(t[0].numpy(), WS, 5, 3, IG))
    assert torch.equal(got[0][lit[0]], (base[0] + term)[lit[0]])


def test_the_plane_is_the_same_bits_in_every_run_and_the_table_is_cached():
    t = S.standard_raster(130, 63, True)
    first = _plane(t, 5, IG)
    table = ops._SEPARATION_TABLES[(WS, 5.0, DEV)]
    for _ in range(2):
        assert torch.equal(_plane(t, 5, IG), first)
    assert ops._SEPARATION_TABLES[(WS, 5.0, DEV)] is table
    assert table.dtype == torch.float32 and table.cpu().numpy().tobytes() == S.table(WS, 5).tobytes()
    assert table.cpu().numpy().tobytes() == ops.separation_table(WS, 5).tobytes()
    assert not torch.equal(_plane(t, 5, IG, ws=2.0), first)


# ---- loss and gradient against float64 ------------------------------------------------------------------------------------------------
SIZES = {"5px": (1, 5), "255px": (15, 17), "256px": (16, 16), "257px": (1, 257), "513x513": (513, 513)}


def _sized_targets(h, w, ignore):
    """int64 [1, h, w] in 3 classes: at 513 x 513 pairs of small rectangles two or three pixels apart, spread over the raster and
    across its chunk and strip borders (few object pixels: the reference is pixels x object pixels); else runs of 2 pixels of a
    seeded coarse grid that is background at three cells in five; ``ignore``: a 255 block inside."""

    if (h, w) == (513, 513):
        boxes = []
        for k, (y, x) in enumerate(((5, 5), (60, 250), (254, 254), (100, 500), (505, 505))):
            boxes += [(y, y + 5, x - 4, x, 1 + k % 2), (y, y + 5, x + 3 + k % 2, x + 7, 1)]
        t = torch.from_numpy(S.rectangles(h, w, boxes)[None])
        if ignore:
            t[:, 250:262, 252:257] = IG
            t[:, 400:420, 200:260] = IG
        return t
    if (h, w) == (1, 5):
        return torch.tensor([[[1, 0, IG if ignore else 0, 0, 2]]])
    g = torch.Generator().manual_seed(h * 1000 + w)
    coarse = torch.randint(0, 5, (1, (h + 1) // 2, (w + 1) // 2), generator=g)
    coarse = torch.where(coarse > 2, torch.zeros_like(coarse), coarse)
    t = coarse.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :h, :w].contiguous()
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
            m = S.plane(t, WS, 1.5, 3, IG if ignore else None)
            valid = t != IG
            assert bool((m[valid] > 1).any()) and bool((m[~valid] == 0).all()) and bool((~valid).any()) == ignore
            out[(key, ignore)] = (t, x, cw, m)
    return out


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("ignore", [False, True], ids=["plain", "ignore"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "class-weights"])
@pytest.mark.parametrize("name", list(MODES))
def test_loss_and_gradient_with_a_device_made_plane(sized, name, weighted, ignore, size):
    """The sizes, modes and bars of the boundary weight's test of the same name."""

    t, x, cw, ref_plane = sized[(size, ignore)]
    w = cw if weighted else None
    ig = IG if ignore else None
    plane = _plane(t, 1.5, ig)
    assert torch.equal(plane, ref_plane)
    loss, grad, stats = _run(name, x, t, w, plane, ig)
    want_loss, want_grad, want_den = B.loss64(name, x, t, w, ref_plane, ig)
    L.compare(name, loss, grad, want_loss, want_grad, what="{} {} {}".format(size, "w" if weighted else "-", "ig" if ignore else "-"))
    assert float(stats[0]) == float(loss)
    assert abs(float(stats[1]) - want_den) <= 1e-6 * want_den  # (a double sum rounded once to float32: 6e-8)
    if ignore:
        at = grad.permute(0, 2, 3, 1)[t == IG]
        assert int(torch.count_nonzero(at)) == 0 and not torch.signbit(at).any()  # +0.0f in every class plane


@pytest.mark.parametrize("name", list(MODES))
def test_shards_add_up_to_the_whole_batch(name):
    """N = 4 split 2 + 2: sum_r loss_r * stats_r[1] = loss * stats[1] -- the identity the data-parallel exchange of the one scalar
    stats[1] rests on (``_global_batch_normaliser``); and an image's plane does not depend on its batch."""

    rows = [S.standard_raster(40, 48), S.standard_raster(40, 48, ignore=True), np.ones((40, 48), dtype=np.int64),
            S.standard_raster(40, 48)[::-1].copy()]
    t = torch.from_numpy(np.stack(rows))
    x, w = B.logits_for(t, 3, seed=11)
    plane = _plane(t, 1.5, IG)
    assert torch.equal(plane, S.plane(t, WS, 1.5, 3, IG)) and bool((plane > 1).any())
    loss, _, stats = _run(name, x, t, w, plane, IG)
    parts = 0.0
    for lo in (0, 2):
        sub = _plane(t[lo:lo + 2].contiguous(), 1.5, IG)
        assert torch.equal(sub, plane[lo:lo + 2])
        l, _, s = _run(name, x[lo:lo + 2].contiguous(), t[lo:lo + 2].contiguous(), w, sub, IG)
        parts += float(l) * float(s[1])
    whole = float(loss) * float(stats[1])
    assert abs(parts - whole) <= L.LOSS_BAR * abs(whole), (parts, whole)


# ---- the modules ------------------------------------------------------------------------------------------------------------------
VARIANTS = {"separation": {}, "separation+boundary": {"boundary": (4, 3)}, "separation+hard": {"hard": (0.25, 0.3)}}


@pytest.fixture(scope="module")
def module_case():
    """Two images of 65 x 65 (the second ignores), logits, class weights and the REFERENCE planes with and without the boundary base."""

    t = torch.from_numpy(np.stack([S.standard_raster(65, 65), S.standard_raster(65, 65, ignore=True)[::-1].copy()]))
    x, w = B.logits_for(t, 3, seed=13)
    planes = {False: S.plane(t, WS, 5, 3, IG), True: S.plane(t, WS, 5, 3, IG, base=B.plane(t, 4.0, 3.0, IG))}
    assert bool((planes[False] > 1).any()) and bool((planes[True] > planes[False]).any())
    return t, x, w, planes


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_modules_through_autograd_and_a_captured_graph(module_case, name, variant, training):
    """The criterion against float64 with the reference plane (mining: the reference plane at the pixels the device kept, which the
    explicit chain of ops confirms bit for bit); then forward and backward captured into a graph, two replays against the eager bits."""

    t, x, w, planes = module_case
    cls = losses.CrossEntropyLoss2d if name == "CrossEntropy" else losses.FocalLoss2d
    kw = VARIANTS[variant]
    crit = cls(weight=w, ignore_index=IG, separation=(WS, 5), **kw).to(DEV)
    crit.train(training)
    td = _dev(t)
    xd = _dev(x).requires_grad_(True)
    loss = crit(xd, td)
    (loss * 0.5).backward()  # grad_out = 0.5
    ref_plane = planes["boundary" in kw]
    if "hard" in kw and training:
        base = ops.separation_weight_plane(td, WS, 5, ignore=IG, classes=3, check=True)
        kept, _ = ops.hard_pixel_plane(_dev(x), td, 0.25, below=0.3, ignore=IG, base=base)
        assert torch.equal(base.cpu(), ref_plane)
        on = kept.cpu() != 0
        assert torch.equal(kept.cpu()[on], ref_plane[on]) and 0 < int(on.sum()) < int((ref_plane != 0).sum())
        ref_plane = torch.where(on, ref_plane, torch.zeros_like(ref_plane))
    want_loss, want_grad, _ = B.loss64(name, x, t, w, ref_plane, IG)
    L.compare(name, loss.detach().cpu(), xd.grad.cpu(), want_loss, 0.5 * want_grad, what="{} {}".format(variant, training))
    at = xd.grad.permute(0, 2, 3, 1)[td == IG]
    assert int(torch.count_nonzero(at)) == 0 and not torch.signbit(at).any()
    # the plane matters here: another number than the criterion without the key gives
    plain = cls(weight=w, ignore_index=IG, **kw).to(DEV)
    plain.train(training)
    assert plain.separation is None and abs(float(plain(_dev(x), td)) - float(loss.detach())) > 1e-4

    eager_loss, eager_grad = loss.detach().clone(), xd.grad.clone()
    xs = _dev(x).requires_grad_(True)

    def step():
        out = crit(xs, td)
        return out, torch.autograd.grad(out * 0.5, xs)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (the tables and the stream's workspace exist before the capture)
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g_loss, g_grad = step()
    for _ in range(2):
        g_loss.detach().zero_()
        g_grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_loss.detach(), eager_loss) and torch.equal(g_grad, eager_grad)


@pytest.mark.parametrize("name", list(MODES))
def test_without_the_key_the_modules_make_the_calls_they_made(name):
    t = _tensor(S.standard_raster(65, 65, True))
    x, w = B.logits_for(t, 3, seed=19)
    cls = losses.CrossEntropyLoss2d if name == "CrossEntropy" else losses.FocalLoss2d
    plain = cls(weight=w, ignore_index=IG, separation=None).to(DEV)
    xp = _dev(x).requires_grad_(True)
    got = plain(xp, _dev(t))
    got.backward()
    base_loss, base_stats = ops.nll_loss_fwd(_dev(x), _dev(t), _dev(w), MODES[name], 2.0, ignore=IG)
    base_grad = ops.nll_loss_bwd(_dev(x), _dev(t), _dev(w), base_stats, torch.ones((), device=DEV), MODES[name], 2.0, ignore=IG)
    assert torch.equal(got.detach(), base_loss) and torch.equal(xp.grad, base_grad)


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    lib = _lib.lib()
    n, c, h, w = 2, 3, 6, 7
    t = torch.zeros(n, h, w, dtype=torch.int64, device=DEV)
    t[:, 2, 1], t[:, 2, 4] = 1, 1
    plane = torch.full((n, h, w), -7.0, device=DEV)
    base = torch.ones(n, h, w, device=DEV)
    table = torch.ones(32 * 32, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def make(n=n, c=c, h=h, w=w, d=3, ignore=-1, targets=ptr(t), tab=ptr(table), out=ptr(plane), work=ptr(ws), base=None):
        return lib.rs_separation_weight_plane(targets, tab, base, out, n, c, h, w, d, ignore, work, stream)

    for bad in ({"c": 0}, {"c": 257}, {"c": -1}, {"ignore": 0}, {"ignore": 256}, {"ignore": -2}, {"n": 0}, {"h": 0}, {"w": 0},
                {"n": -1}, {"h": -3}, {"w": -1}, {"d": 0}, {"d": -1}, {"d": 33}, {"d": 1 << 20}, {"n": 65536}, {"h": 4097},
                {"targets": None}, {"tab": None}, {"out": None}, {"work": None}, {"work": ctypes.c_void_p(ws.data_ptr() + 4)}):
        assert make(**bad) == _lib.RS_EINVAL, bad
    for bad in ((0, 5, 7), (2, 0, 7), (2, 5, -1), (65536, 1, 1), (1, 4097, 1), (1 << 9, 1 << 10, 1 << 10)):
        assert lib.rs_separation_weight_plane_workspace_bytes(*bad) == _lib.RS_EINVAL
    assert lib.rs_separation_weight_plane_workspace_bytes(n, h, w) == 16 + 14 * n * h * w
    torch.cuda.synchronize()
    assert (plane == -7.0).all()  # (nothing was launched)
    assert make(d=1) == 0 and make(d=32) == 0 and make(ignore=255) == 0 and make(c=1) == 0 and make(c=256) == 0 and make(base=ptr(base)) == 0
    torch.cuda.synchronize()
    assert (plane >= 1.0).all()

    plane.fill_(-7.0)
    for call in (lambda: ops.separation_weight_plane(t, WS, 10.7),                                  # ceil(3 sigma) = 33
                 lambda: ops.separation_weight_plane(t, 0.0, 5.0),
                 lambda: ops.separation_weight_plane(t, WS, float("nan")),
                 lambda: ops.separation_weight_plane(t, float("inf"), 5.0),
                 lambda: ops.separation_weight_plane(t, WS, -1.0),
                 lambda: ops.separation_weight_plane(t, True, 5.0),
                 lambda: ops.separation_weight_plane(t, WS, 5.0, ignore=2, classes=3),
                 lambda: ops.separation_weight_plane(t, WS, 5.0, classes=0),
                 lambda: ops.separation_weight_plane(t, WS, 5.0, base=base[:1]),
                 lambda: ops.separation_weight_plane(t, WS, 5.0, base=base.double()),
                 lambda: ops.separation_weight_plane(t, WS, 5.0, base=base.cpu()),
                 lambda: losses.CrossEntropyLoss2d(separation=(WS, 10.7)),
                 lambda: losses.FocalLoss2d(separation=5.0),
                 lambda: losses.FocalLoss2d(separation=(0, 5.0))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError):
        ops.separation_weight_plane(t.cpu(), WS, 5.0)  # (no CPU path)
