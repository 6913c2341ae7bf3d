"""Boundary label relaxation on the MI355X: ``ops.label_set_plane`` (``rs_label_set_plane``) against the brute-force numpy reference of
tests/relax_ref.py with ``torch.equal`` -- the plane is integers, so it is defined bit for bit -- and the relaxed CrossEntropy / Focal
(``rs_nll_loss_*_rx``) against float64 (``relax_ref.loss64``) under the bars of the plain losses' tests (``losses_ref.LOSS_BAR`` /
``GRAD_BAR``), bit for bit against the ``_pw`` calls where every set is a singleton, and through the criteria.

The float64 side always uses the REFERENCE sets, never the device's.  Every case states on the reference what it puts to the test
(``relax_ref.census``) before the device is asked."""

import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as B  # noqa: E402
import losses_ref as L  # noqa: E402
import relax_ref as X  # noqa: E402
import separation_ref as S  # noqa: E402

from robosat_amd import _lib, losses, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IG = X.IGNORE
MODES = {"CrossEntropy": ops.NLL_CROSS_ENTROPY, "Focal": ops.NLL_FOCAL}
RADII = [1, 2, 5, 11, 16]  # windows 3, 5, 11, 23, 33: 11 and 23 are no powers of two


def _dev(t):
    return None if t is None else t.to(DEV)


def _sets(labels, radius, ignore=None, classes=8):
    """The device's plane of int64 numpy / torch labels [N, H, W] as a CPU tensor."""

    t = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else labels
    out = ops.label_set_plane(_dev(t), radius, ignore=ignore, classes=classes).cpu()
    assert out.dtype == torch.uint8 and out.shape == t.shape
    return out


def _same(got, want):
    want = torch.from_numpy(want) if isinstance(want, np.ndarray) else want
    assert torch.equal(got, want), "{} of {} pixels differ".format(int((got != want).sum()), want.numel())


@functools.lru_cache(maxsize=None)
def _plane_case(h, w, radius, ignore):
    """(labels, reference sets) of one C = 8 raster per size, radius and ignore variant, made once."""

    t = X.blocks_raster(1, 8, h, w, seed=h * 131 + w, ignore=ignore)
    return t, X.sets_brute(t, radius, IG if ignore else None)


# ---- the set plane --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", [(65, 65), (64, 130), (130, 63)])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("ignore", [False, True], ids=["plain", "ignore"])
def test_the_plane_across_tile_borders(h, w, radius, ignore):
    """Sizes that cross any 64-wide tile, C = 8 with every bit used, bit 7 included."""

    t, want = _plane_case(h, w, radius, ignore)
    cen = X.census(t, want, IG if ignore else None)
    assert cen["bits"] == 255 and cen["more"] > 0 and (cen["ignored"] > 0) == ignore, cen
    assert (h > 64 or w > 64) and int((t == 7).sum()) > 0
    _same(_sets(t, radius, IG if ignore else None), want)


@pytest.mark.parametrize("h, w", [(1, 1), (1, 70), (70, 1), (5, 7)])
@pytest.mark.parametrize("radius", RADII)
def test_the_plane_of_rasters_smaller_than_the_reach(h, w, radius):
    assert min(h, w) < 2 * max(RADII) + 1 and (radius < 5 or min(h, w) < 2 * radius + 1)
    for ignore in (False, True):
        t, want = _plane_case(h, w, radius, ignore)
        _same(_sets(t, radius, IG if ignore else None), want)


@pytest.mark.parametrize("radius", [2, 11])
def test_three_images_are_three_single_calls(radius):
    """Images never see each other; one of them holds a single valid pixel enclosed by ignored ones, one is ignored altogether."""

    t = np.full((3, 40, 70), IG, dtype=np.int64)
    t[0] = X.blocks_raster(1, 8, 40, 70, seed=5, ignore=True)[0]
    t[1, 20, 33] = 6
    want = X.sets_brute(t, radius, IG)
    assert want[2].max() == 0 and int((want[1] != 0).sum()) == 1 and want[1, 20, 33] == 64 and X.census(t[:1], want[:1], IG)["more"] > 0
    got = _sets(t, radius, IG)
    _same(got, want)
    for i in range(3):
        _same(_sets(t[i:i + 1], radius, IG)[0], want[i])
    # without the ignore label the same call reads 255 as "not ignored": labels >= C are undefined, so only the labels < C are used here
    plain = np.where(t == IG, 0, t)
    _same(_sets(plain, radius), X.sets_brute(plain, radius))


@pytest.mark.parametrize("radius", RADII)
def test_a_single_pixel_lights_its_window_clipped_to_the_image(radius):
    """One pixel of class 5 on class 0 at each corner, at column 63 / 64 and at row 63 / 64: exactly its (2R+1)^2 window, clipped,
    holds bit 5."""

    h, w = 70, 130
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (30, 63), (30, 64), (63, 100), (64, 100), (63, 63), (64, 64)):
        t = np.zeros((1, h, w), dtype=np.int64)
        t[0, y, x] = 5
        want = np.ones((1, h, w), dtype=np.uint8)
        want[0, max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1] |= 32
        want[0, y, x] = 33 if radius >= 1 and (h > 1 or w > 1) else 32
        lit = int((want & 32 != 0).sum())
        assert lit == (min(h, y + radius + 1) - max(0, y - radius)) * (min(w, x + radius + 1) - max(0, x - radius))
        _same(_sets(t, radius), want)


def test_the_plane_is_the_same_bits_in_every_run():
    t, want = _plane_case(130, 63, 11, True)
    first = _sets(t, 11, IG)
    for _ in range(3):
        assert torch.equal(_sets(t, 11, IG), first)
    _same(first, want)


# ---- the losses against float64 -------------------------------------------------------------------------------------------------------
GOUT = 0.37
VARIANTS = {"plain": (False, False, False), "class-weights": (True, False, False), "pixel-weights": (False, True, False),
            "ignore": (False, False, True), "all": (True, True, True)}


def _run(name, x, t, w, plane, sets, ignore=None, gout=None):
    """(loss, gradient, stats) of the ``_rx`` calls as CPU tensors; ``sets=None`` makes the strict calls."""

    xd, td, wd, pd = _dev(x), _dev(t), _dev(w), _dev(plane)
    sd = None if sets is None else _dev(torch.from_numpy(sets) if isinstance(sets, np.ndarray) else sets)
    loss, stats = ops.nll_loss_fwd(xd, td, wd, MODES[name], 2.0, ignore=ignore, pixel_weight=pd, label_sets=sd)
    kept = stats.clone()
    grad = ops.nll_loss_bwd(xd, td, wd, stats, _dev(gout), MODES[name], 2.0, ignore=ignore, pixel_weight=pd, label_sets=sd)
    return loss.cpu(), grad.cpu(), kept.cpu()


def _assert_plus_zero(grad, where):
    at = grad.permute(0, 2, 3, 1)[where]
    assert int(torch.count_nonzero(at)) == 0 and not torch.signbit(at).any()


def _loss_case(name, c, shape_key, variant, scale):
    weighted, planed, ignored = VARIANTS[variant]
    t, sets = X.loss_case(c, shape_key, ignored)
    n, h, w = t.shape
    x, cw = X.logits_for((n, c, h, w), seed=c * 7 + len(shape_key), scale=scale)
    plane = X.pixel_weights(n, h, w, seed=c) if planed else None
    ig = IG if ignored else None
    return x, t, (cw if weighted else None), plane, sets, ig


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("c", [2, 3, 8])
@pytest.mark.parametrize("shape_key", ["wide", "small"])
@pytest.mark.parametrize("variant, scale", [(v, 2.0) for v in VARIANTS] + [("plain", 30.0), ("all", 30.0)])
def test_loss_and_gradient_against_float64(name, c, shape_key, variant, scale):
    """Shapes (3, C, 33, 65) and (1, C, 7, 9), logits of scale 2 and of scale 30 (lse_S far below lse), grad_out = 0.37."""

    x, t, cw, plane, sets, ig = _loss_case(name, c, shape_key, variant, scale)
    cen = X.census(t.numpy(), sets, ig)
    assert cen["one"] > 0 and cen["two"] > 0 and (c < 3 or cen["more"] > 0), cen
    want_loss, want_grad, want_den = X.loss64(name, x, t, sets, cw, plane, ig)
    strict = B.loss64(name, x, t, cw, torch.ones(t.shape) if plane is None else plane, ig)
    assert want_loss < strict[0] and want_den == strict[2]  # (the case relaxes something, and the normaliser is the strict one)
    if scale > 10:
        # some pixel's whole set lies far below the largest logit: log q << 0 there
        logq = torch.logsumexp(torch.where(torch.stack([torch.from_numpy((sets.astype(np.int64) >> k) & 1) for k in range(c)], 1).bool(),
                                           x.double(), torch.full_like(x.double(), float("-inf"))), 1) - torch.logsumexp(x.double(), 1)
        assert float(logq[t != IG].min()) < -30.0
    loss, grad, stats = _run(name, x, t, cw, plane, sets, ig, torch.tensor(GOUT))
    L.compare(name, loss, grad, want_loss, GOUT * want_grad, what="C={} {} {} scale {}".format(c, shape_key, variant, scale))
    assert abs(float(stats[0]) - float(loss)) == 0.0 and abs(float(stats[1]) - want_den) <= 1e-6 * want_den
    # stats[1] is today's denominator to the bit: the strict call with the same weights
    _, _, strict_stats = _run(name, x, t, cw, plane, None, ig, torch.tensor(GOUT))
    assert torch.equal(stats[1], strict_stats[1])
    if ig is not None:
        assert int((t == IG).sum()) > 0
        _assert_plus_zero(grad, t == IG)
    if plane is not None:
        assert int((plane == 0).sum()) > 0
        _assert_plus_zero(grad, plane == 0)


@pytest.mark.parametrize("name", list(MODES))
def test_an_image_without_a_valid_pixel(name):
    x, w = X.logits_for((2, 3, 9, 11), seed=3)
    t = torch.full((2, 9, 11), IG, dtype=torch.int64)
    sets = X.sets_brute(t.numpy(), 2, IG)
    assert sets.max() == 0 and X.loss64(name, x, t, sets, w, None, IG) [0] == 0.0
    loss, grad, stats = _run(name, x, t, w, None, sets, IG, torch.tensor(GOUT))
    assert float(loss) == 0.0 and float(stats[1]) == 0.0
    _assert_plus_zero(grad, t == IG)
    # one image ignored altogether beside one that is not: the valid one carries the loss alone
    t[1] = torch.from_numpy(X.blocks_raster(1, 3, 9, 11, seed=2)[0])
    sets = X.sets_brute(t.numpy(), 2, IG)
    want_loss, want_grad, _ = X.loss64(name, x, t, sets, w, None, IG)
    loss, grad, _ = _run(name, x, t, w, None, sets, IG, torch.tensor(GOUT))
    L.compare(name, loss, grad, want_loss, GOUT * want_grad, what="one image ignored")
    _assert_plus_zero(grad, t == IG)


@pytest.mark.parametrize("c", [2, 3, 8])
def test_a_set_of_all_classes_costs_nothing(c):
    """CrossEntropy: a pixel whose set is all C classes has loss 0 and a gradient of exactly 0."""

    t = X.noise_raster(2, c, 12, 14, seed=c)
    sets = X.sets_brute(t, 11)
    assert (sets == (1 << c) - 1).all()
    x, w = X.logits_for((2, c, 12, 14), seed=c, scale=8.0)
    assert X.loss64("CrossEntropy", x, torch.from_numpy(t), sets, w)[0] == 0.0
    loss, grad, stats = _run("CrossEntropy", x, torch.from_numpy(t), w, None, sets, None, torch.tensor(GOUT))
    assert float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0 and float(stats[1]) > 0
    _same(_sets(t, 11, classes=c), sets)


# ---- bit identity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("c", [2, 3, 8])
@pytest.mark.parametrize("kind", ["uniform", "bands"])
def test_singleton_sets_make_the_pw_calls_bit_for_bit(name, c, kind):
    """Every valid pixel's set is its own label alone (uniform images; bands of classes separated by ignored strips wider than R): loss,
    stats and gradient of the ``_rx`` calls are those of the ``_pw`` calls, with a pixel-weight plane and with none (a plane of 1.0f)."""

    radius, shape = 2, (3, 33, 65)
    if kind == "uniform":
        t = np.stack([np.full(shape[1:], k % c, dtype=np.int64) for k in range(shape[0])])
        ig = None
    else:
        t = X.singleton_raster(shape[0], c, shape[1], shape[2], radius, seed=c)
        ig = IG
    want = X.sets_brute(t, radius, ig)
    cen = X.census(t, want, ig)
    assert cen["one"] > 0 and cen["two"] == 0 and cen["more"] == 0 and (cen["ignored"] > 0) == (kind == "bands"), cen
    sets = _sets(t, radius, ig, classes=c)
    _same(sets, want)
    tt = torch.from_numpy(t)
    x, w = X.logits_for((shape[0], c) + shape[1:], seed=17 + c, scale=4.0)
    plane = X.pixel_weights(*shape, seed=23)
    gout = torch.tensor(GOUT)
    for pw_plane, rx_plane in ((plane, plane), (torch.ones(shape), None)):
        base = _run(name, x, tt, w, pw_plane, None, ig, gout)
        got = _run(name, x, tt, w, rx_plane, sets, ig, gout)
        for a, b, what in zip(got, base, ("loss", "gradient", "stats")):
            assert torch.equal(a, b), "{} differs from the _pw call's ({} plane)".format(what, "no" if rx_plane is None else "a")
        assert bool(torch.isfinite(got[1]).all()) and float(got[0]) > 0


@pytest.mark.parametrize("name", list(MODES))
def test_the_same_relaxed_input_gives_the_same_bits(name):
    x, t, cw, plane, sets, ig = _loss_case(name, 8, "wide", "all", 2.0)
    first = _run(name, x, t, cw, plane, sets, ig, torch.tensor(GOUT))
    for _ in range(2):
        again = _run(name, x, t, cw, plane, sets, ig, torch.tensor(GOUT))
        assert all(torch.equal(a, b) for a, b in zip(first, again))


# ---- the purpose, on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx, dy, within", [(2, 0, True), (-2, 2, True), (1, -2, True), (0, 1, True), (3, 0, False), (0, -3, False),
                                            (3, 3, False)])
def test_shifted_labels(dx, dy, within):
    """Confident logits that follow the true shape against labels moved by (dx, dy): below 1e-6 relaxed and above 0.1 strict while
    |dx|, |dy| <= R = 2; large again at R + 1."""

    radius = 2
    x, t = X.shifted_case(24, 28, radius, dx, dy)
    ref_sets = X.sets_brute(t.numpy(), radius)
    want = X.loss64("CrossEntropy", x, t, ref_sets)[0]
    strict = L.nll_family64("CrossEntropy", x, t)[0]
    assert strict > 0.1 and ((want < 1e-6) if within else (want > 0.1)), (want, strict)
    sets = _sets(t, radius, classes=2)
    _same(sets, ref_sets)
    for name in MODES:
        loss, grad, _ = _run(name, x, t, None, None, sets)
        assert (float(loss) < 1e-6) if within else (float(loss) > 0.1), (name, float(loss))
        assert bool(torch.isfinite(grad).all())
    loss, _, _ = _run("CrossEntropy", x, t, None, None, None)
    assert float(loss) > 0.1


# ---- the criteria -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def module_case():
    """Two images of 65 x 65 (the second ignores), logits, class weights, the REFERENCE sets at radius 2 and the REFERENCE weight planes."""

    t = torch.from_numpy(np.stack([S.standard_raster(65, 65), S.standard_raster(65, 65, ignore=True)[::-1].copy()]))
    x, w = B.logits_for(t, 3, seed=13)
    sets = X.sets_brute(t.numpy(), 2, IG)
    cen = X.census(t.numpy(), sets, IG)
    assert cen["one"] > 0 and cen["two"] > 0 and cen["ignored"] > 0, cen
    boundary = B.plane(t, 4.0, 3.0, IG)
    planes = {"relax": None, "relax+boundary": boundary, "relax+boundary+separation": S.plane(t, 10.0, 5, 3, IG, base=boundary)}
    return t, x, w, sets, planes


KW = {"relax": {}, "relax+boundary": {"boundary": (4.0, 3.0)}, "relax+boundary+separation": {"boundary": (4.0, 3.0), "separation": (10.0, 5)}}


def _cls(name):
    return losses.CrossEntropyLoss2d if name == "CrossEntropy" else losses.FocalLoss2d


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("variant", list(KW))
def test_the_criteria_relax_in_training_and_are_strict_in_eval(module_case, name, variant):
    """Training: float64 on the reference sets and the reference planes, which are made from the strict labels.  ``.eval()``: the bits
    of the criterion without ``relax``."""

    t, x, w, sets, planes = module_case
    crit = _cls(name)(weight=w, ignore_index=IG, relax=2, **KW[variant]).to(DEV)
    assert crit.training and crit.relax == 2
    td = _dev(t)
    xd = _dev(x).requires_grad_(True)
    loss = crit(xd, td)
    (loss * 0.5).backward()
    want_loss, want_grad, _ = X.loss64(name, x, t, sets, w, planes[variant], IG)
    L.compare(name, loss.detach().cpu(), xd.grad.cpu(), want_loss, 0.5 * want_grad, what=variant)
    _assert_plus_zero(xd.grad.cpu(), t == IG)

    strict = _cls(name)(weight=w, ignore_index=IG, **KW[variant]).to(DEV)
    xs = _dev(x).requires_grad_(True)
    strict_loss = strict(xs, td)
    strict_loss.backward()
    assert abs(float(strict_loss.detach()) - float(loss.detach())) > 1e-4  # (relaxation matters on this input)
    crit.eval()
    xe = _dev(x).requires_grad_(True)
    eval_loss = crit(xe, td)
    eval_loss.backward()
    assert torch.equal(eval_loss.detach(), strict_loss.detach()) and torch.equal(xe.grad, xs.grad)
    crit.train()
    assert torch.equal(crit(_dev(x), td).detach(), loss.detach())


@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("ignore", [False, True], ids=["plain", "ignore"])
def test_without_relax_the_criteria_make_the_calls_they_made(module_case, name, ignore):
    t, x, w, _, _ = module_case
    t = t if ignore else torch.where(t == IG, torch.zeros_like(t), t)
    ig = IG if ignore else None
    crit = _cls(name)(weight=w, ignore_index=ig, relax=None).to(DEV)
    xp = _dev(x).requires_grad_(True)
    got = crit(xp, _dev(t))
    got.backward()
    base_loss, base_stats = ops.nll_loss_fwd(_dev(x), _dev(t), _dev(w), MODES[name], 2.0, ignore=ig)
    base_grad = ops.nll_loss_bwd(_dev(x), _dev(t), _dev(w), base_stats, torch.ones((), device=DEV), MODES[name], 2.0, ignore=ig)
    assert torch.equal(got.detach(), base_loss) and torch.equal(xp.grad, base_grad)


def test_relax_with_hard_raises_and_cldice_wraps_a_relaxed_base(module_case):
    t, x, w, _, _ = module_case
    for cls in (losses.CrossEntropyLoss2d, losses.FocalLoss2d):
        with pytest.raises(ValueError, match="relax cannot be combined with hard"):
            cls(weight=w, relax=2, hard=0.25)
    crit = losses.ClDiceLoss2d(losses.CrossEntropyLoss2d(weight=w, ignore_index=IG, relax=2), 0.3, iters=3, ignore_index=IG).to(DEV)
    assert crit.relax == 2 and crit.hard is None
    xd = _dev(x).requires_grad_(True)
    loss = crit(xd, _dev(t))
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
    crit.eval()
    strict = losses.ClDiceLoss2d(losses.CrossEntropyLoss2d(weight=w, ignore_index=IG), 0.3, iters=3, ignore_index=IG).to(DEV)
    assert torch.equal(crit(_dev(x), _dev(t)).detach(), strict(_dev(x), _dev(t)).detach())


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    lib = _lib.lib()
    n, c, h, w = 2, 3, 6, 7
    t = torch.zeros(n, h, w, dtype=torch.int64, device=DEV)
    sets = torch.full((n, h, w), 99, dtype=torch.uint8, device=DEV)
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def make(n=n, c=c, h=h, w=w, r=2, ignore=-1, targets=ptr(t), out=ptr(sets)):
        return lib.rs_label_set_plane(targets, out, n, c, h, w, r, ignore, stream)

    for bad in ({"r": 0}, {"r": 17}, {"r": -1}, {"r": 1 << 20}, {"c": 0}, {"c": 9}, {"c": -1}, {"ignore": 0}, {"ignore": 2}, {"ignore": 256},
                {"ignore": -2}, {"n": 0}, {"h": 0}, {"w": 0}, {"n": -1}, {"h": -3}, {"w": -1}, {"n": 65536}, {"h": 4097}, {"w": 4097},
                {"targets": None}, {"out": None}):
        assert make(**bad) == _lib.RS_EINVAL, bad
    torch.cuda.synchronize()
    assert (sets == 99).all()  # (nothing was launched)
    assert make(r=1) == 0 and make(r=16) == 0 and make(ignore=255) == 0 and make(ignore=3) == 0 and make(c=1) == 0 and make(c=8) == 0
    torch.cuda.synchronize()
    assert (sets == 1).all()

    x = torch.zeros(n, c, h, w, device=DEV)
    loss, stats = torch.zeros((), device=DEV), torch.zeros(2, device=DEV)
    ws = torch.empty(lib.rs_nll_loss_workspace_bytes(), dtype=torch.uint8, device=DEV)
    dx = torch.zeros_like(x)

    def fwd(c=c, mode=0, ignore=-1, s=ptr(sets), xs=ptr(x)):
        return lib.rs_nll_loss_fwd_rx(xs, ptr(t), None, ptr(loss), ptr(stats), n, c, h, w, mode, ctypes.c_float(2.0), ptr(ws), stream,
                                      None, ignore, s)

    def bwd(c=c, mode=0, ignore=-1, s=ptr(sets), out=ptr(dx)):
        return lib.rs_nll_loss_bwd_rx(ptr(x), ptr(t), None, ptr(stats), None, out, n, c, h, w, mode, ctypes.c_float(2.0), stream, None,
                                      ignore, s)

    for call in (fwd, bwd):
        for bad in ({"s": None}, {"c": 9}, {"c": 0}, {"mode": 2}, {"ignore": 1}, {"ignore": 256}):
            assert call(**bad) == _lib.RS_EINVAL, (call.__name__, bad)
    assert fwd(xs=None) == _lib.RS_EINVAL and bwd(out=None) == _lib.RS_EINVAL
    assert fwd() == 0 and bwd() == 0  # (null class weights, pixel weights and grad_out are allowed)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(np.log(3.0))) < 1e-6 and float(stats[1]) == n * h * w

    for call in (lambda: ops.label_set_plane(t, 0), lambda: ops.label_set_plane(t, 17), lambda: ops.label_set_plane(t, True),
                 lambda: ops.label_set_plane(t, 2.0), lambda: ops.label_set_plane(t, 2, ignore=2, classes=3),
                 lambda: losses.CrossEntropyLoss2d(relax=0), lambda: losses.FocalLoss2d(relax=2.0), lambda: losses.FocalLoss2d(relax=True)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError):
        ops.label_set_plane(t.cpu(), 2)  # (no CPU path)
