"""The Lovasz hinge loss (reference robosat/losses.py:96-119) restated so that EVERY element of its gradient is defined, the
checker that holds a kernel to it exactly, and the input families of its tests (TEST INFRASTRUCTURE ONLY; plain numpy on the
CPU, nothing of the package under test).

The reference sorts an image's C*H*W hinge errors with ``torch.sort``, which is not stable on the CPU, so inside a group of equal
errors its gradient is the sort's choice (tests/lovasz_check.py compares group sums for that reason).  With a STABLE descending
sort -- equal errors in ascending flat index ``c*HW + hw`` -- the permutation is unique, every operand of the Jaccard curve is an
integer below 2^24 and hence exact in fp32, and each of the reference's fp32 operations (two subtractions, one addition, one
division, one difference of neighbours) has exactly one correctly rounded result.  The whole gradient is then one defined fp32
array, and a kernel that claims a stable sort and the reference's operations has to reproduce it value for value.

Per image, with ``m`` the one-hot mask and ``x`` the fp32 logits:

    err_i   = fp32(1 - (2 m_i - 1) x_i)
    order   = stable descending sort of err;  lab_r = m_order(r);  cs_r = labels among ranks 0 .. r (an integer, cast to fp32)
    jac_r   = fp32: 1 - (gts - cs_r) / (gts + ((r + 1) - cs_r)),  gts = H*W;   delta_0 = jac_0, delta_r = jac_r - jac_{r-1}
    loss_n  = sum_r float64(fp32(relu(err_order(r)) * delta_r));   loss = mean over the N images (float64)
    unit_i  = -(2 m_i - 1) [err_i > 0] delta_rank(i)              (d loss / d x_i = unit_i / N)

With an ignore label the same on the compaction: an image's ignored pixels are dropped, the rest packed in ``(c, hw)`` order,
``gts`` = the image's valid pixel count; the gradient goes back to its place, +0.0 at the ignored pixels; an image with no valid
pixel contributes 0 to the sum (and still counts in N)."""

import numpy as np
import torch

F32 = np.float32
SCAN_CHUNK = 1024  # (only to name a rank's scan chunk and sort tile in a failure report)
SORT_TILES = (8192, 4096)


def jaccard_deltas(cs, ranks1, gts):
    """fp32 Jaccard increments from the inclusive label counts ``cs`` and the 1-based ranks ``ranks1`` (integer arrays) and the
    foreground count ``gts``, with the reference's operations in the reference's order."""

    cs, r1, g = cs.astype(F32), ranks1.astype(F32), F32(gts)
    inter = g - cs
    union = g + (r1 - cs)  # the reference's cumsum(1 - lab): the integer r + 1 - cs_r
    jac = F32(1) - inter / union
    assert jac.dtype == F32
    return np.concatenate([jac[:1], jac[1:] - jac[:-1]]) if jac.size > 1 else jac


def _image(x, t, c, ignore):
    """One image: x fp32 [C, HW], t int64 [HW].  Returns (loss float64, unit fp32 [C, HW], err fp32 [C, HW] (nan where ignored),
    rank int64 [C, HW] (-1 where ignored))."""

    hw = t.size
    keep = np.ones(hw, dtype=bool) if ignore is None else t != ignore
    unit, err_full, rank_full = np.zeros((c, hw), F32), np.full((c, hw), np.nan, F32), np.full((c, hw), -1, np.int64)
    k = int(keep.sum())
    if k == 0:
        return 0.0, unit, err_full, rank_full
    m = (t[keep][None, :] == np.arange(c)[:, None]).reshape(-1)  # packed in (c, hw) order
    sign = np.where(m, F32(1), F32(-1))
    err = F32(1) - sign * x[:, keep].reshape(-1)
    assert err.dtype == F32 and bool(np.isfinite(err).all())
    order = np.argsort(-err, kind="stable")  # descending; equal errors in ascending packed index
    lab = m[order]
    delta = jaccard_deltas(np.cumsum(lab.astype(np.int64)), np.arange(1, err.size + 1, dtype=np.int64), k)
    e = err[order]
    prod = np.maximum(e, F32(0)) * delta
    assert prod.dtype == F32
    loss = float(np.sum(prod.astype(np.float64)))
    g = np.where(e > 0, delta, F32(0)) * -sign[order]
    packed_unit, packed_rank = np.empty(err.size, F32), np.empty(err.size, np.int64)
    packed_unit[order] = g
    packed_rank[order] = np.arange(err.size)
    unit[:, keep] = packed_unit.reshape(c, k)
    err_full[:, keep] = err.reshape(c, k)
    rank_full[:, keep] = packed_rank.reshape(c, k)
    return loss, unit, err_full, rank_full


class Detail:
    """What a failure report needs beyond the gradient: per element the fp32 error (nan where ignored), the rank in its image's
    stable order (-1 where ignored) and whether another element of the image has the same error; and the ignored pixels."""

    def __init__(self, err, rank, ignored):
        self.err, self.rank, self.ignored = err, rank, ignored  # [N, C, H, W], [N, C, H, W], bool [N, H, W]

    def tied(self, flat):
        n, rest = divmod(int(flat), self.err[0].size)
        e = self.err[n].reshape(-1)
        return bool(np.count_nonzero(e == e[rest]) > 1)


def hinge_exact(logits, targets, ignore=None, detail=False):
    """logits fp32 [N, C, H, W], targets int64 [N, H, W] (torch or numpy) -> (loss float64, unit_delta fp32 [N, C, H, W] numpy:
    N * d loss / d logits); with ``detail`` a ``Detail`` as the third."""

    x = np.ascontiguousarray(logits.numpy() if isinstance(logits, torch.Tensor) else logits)
    t = np.ascontiguousarray(targets.numpy() if isinstance(targets, torch.Tensor) else targets).astype(np.int64)
    assert x.dtype == F32 and x.ndim == 4 and t.shape == (x.shape[0],) + x.shape[2:]
    n, c, h, w = x.shape
    total, unit, err, rank = 0.0, np.empty(x.shape, F32), np.empty(x.shape, F32), np.empty(x.shape, np.int64)
    for i in range(n):
        li, ui, ei, ri = _image(x[i].reshape(c, -1), t[i].reshape(-1), c, ignore)
        total += li
        unit[i], err[i], rank[i] = ui.reshape(c, h, w), ei.reshape(c, h, w), ri.reshape(c, h, w)
    loss = total / n
    if detail:
        return loss, unit, Detail(err, rank, np.zeros(t.shape, bool) if ignore is None else t == ignore)
    return loss, unit


# ---- the checker ----------------------------------------------------------------------------------------------------------

def _ordered(a):
    """fp32 -> int64 that counts representable values in order (-0.0 and +0.0 both 0): differences are ulp distances."""

    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    return np.abs(_ordered(np.ascontiguousarray(a, F32)) - _ordered(np.ascontiguousarray(b, F32)))


def loss_bar(want_loss, keys):
    """1 ulp of fp32(want_loss) -- a kernel adds the same fp32 products in fp64 and rounds once, scaled by fp32(1 / N) -- plus
    ``keys * 2^-52 * |want_loss|`` for the order of the fp64 additions (all terms are >= 0: jac never decreases along the ranks,
    and a correctly rounded quotient keeps that)."""

    return float(np.spacing(F32(abs(want_loss)))) + keys * 2.0 ** -52 * abs(want_loss)


def assert_hinge_exact(got_loss, got_grad, want_loss, want_delta, n, detail=None, what="lovasz hinge"):
    """``got_grad`` (d loss / d logits, fp32) == fp32(want_delta / n) BY VALUE (-0.0 == 0.0): elementwise and exactly when n is a
    power of two, where the division and a product with fp32(1 / n) are the same exact scaling; otherwise at most 1 fp32 ulp
    apart (the product with the rounded reciprocal is within 1.5 ulp of the true quotient, the correctly rounded quotient within
    0.5, both on the fp32 grid).  The loss under ``loss_bar``.  With ``detail``: +0.0 by bit pattern at the ignored pixels, and a
    failure names the first wrong element's rank, sort tile, scan chunk and whether its error is tied."""

    got = np.ascontiguousarray(got_grad.detach().cpu().numpy() if isinstance(got_grad, torch.Tensor) else got_grad)
    assert got.dtype == F32 and got.shape == want_delta.shape and want_delta.dtype == F32, (what, got.dtype, got.shape)
    want = want_delta / F32(n)
    assert want.dtype == F32
    allowed = 0 if n & (n - 1) == 0 else 1
    bad = ~np.isfinite(got) | (ulp_distance(got, want) > allowed)
    if bad.any():
        flat = int(np.flatnonzero(bad.reshape(-1))[0])
        where = ""
        if detail is not None:
            r = int(detail.rank.reshape(-1)[flat])
            where = ", rank {} of its image (scan chunk {}, sort tile {} of 8192 / {} of 4096), error {!r} {}".format(
                r, r // SCAN_CHUNK, r // SORT_TILES[0], r // SORT_TILES[1], float(detail.err.reshape(-1)[flat]),
                "in a tie group" if detail.tied(flat) else "unique in its image")
        raise AssertionError("{}: {} of {} gradient entries differ by more than {} ulp; first at flat index {} (image {}): got {!r}, "
                             "want {!r}{}".format(what, int(bad.sum()), bad.size, allowed, flat, flat // want[0].size,
                                                  float(got.reshape(-1)[flat]), float(want.reshape(-1)[flat]), where))
    if detail is not None:
        at_ignored = np.broadcast_to(detail.ignored[:, None], got.shape)
        assert not np.signbit(got[at_ignored]).any() and not got[at_ignored].any(), what + ": not +0.0 at an ignored pixel"
        closed = ~at_ignored & ~(detail.err > 0)
        assert not got[closed].any(), what + ": a gradient where the error is not above 0"
    got_loss = float(got_loss)
    bar = loss_bar(want_loss, want_delta.size)
    assert abs(got_loss - want_loss) <= bar, "{}: loss {!r}, want {!r}: {:.3e} apart, bar {:.3e}".format(
        what, got_loss, want_loss, abs(got_loss - want_loss), bar)


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------

FAMILIES = ["const", "two", "four", "quant", "lowbyte", "exponent", "ramp", "gauss"]


def labels(shape, seed):
    """int64 [N, H, W], uniform over the classes, the last class rare in image 0 (absent from its upper half)."""

    n, c, h, w = shape
    g = torch.Generator().manual_seed(3000 + seed)
    y = torch.randint(0, c, (n, h, w), generator=g)
    top = y[0, : max(h // 2, 1)]
    top[top == c - 1] = 0
    return y


def family(name, shape, seed=0):
    """(logits fp32 [N, C, H, W], labels int64 [N, H, W]) of one input family; each asserts on the fp32 errors what it is for.

    const     all logits 0: ONE key.  Every pass puts whole tiles into one digit and the result is the stable order alone.
    two       +-3 from a hard prediction that is right at about 70 % of the pixels: the errors are -2 and 4, two huge tie groups,
              one on each side of the ``err > 0`` gate.
    four      the same prediction with magnitude 2 or 3 by a coin per element: errors -2, -1, 3 and 4, two on each side.
    quant     round(randn * 8) / 4: about 60 distinct errors, exactly 0 and negative ones among them.
    lowbyte   -(2m - 1)(1 + j 2^-23), j in [0, 256): errors in [2, 2 + 2^-15], whose keys differ in their low byte only -- pass 0
              alone orders them, passes 1 to 3 see one digit.
    exponent  +-2^k, k in [-20, 20], sign by a coin: at most 82 distinct errors 1 -+ 2^k, from 2^-20 below 1 to beyond +-10^6.
    ramp      errors strictly ascending in the flat index (a multiple of 2^-10 each, one of them 0): the sort reverses the image.
    gauss     randn * 3: the distribution of the older tests."""

    n, c, h, w = shape
    y = labels(shape, seed)
    g = torch.Generator().manual_seed(4000 + seed + FAMILIES.index(name))
    m = torch.nn.functional.one_hot(y, c).permute(0, 3, 1, 2)
    sign = (m * 2 - 1).float()
    p = c * h * w
    if name == "const":
        x = torch.zeros(shape)
    elif name in ("two", "four"):
        pred = torch.where(torch.rand(n, h, w, generator=g) < 0.7, y, torch.randint(0, c, (n, h, w), generator=g))
        x = torch.nn.functional.one_hot(pred, c).permute(0, 3, 1, 2).float() * 2 - 1
        x = x * (3.0 if name == "two" else torch.where(torch.rand(shape, generator=g) < 0.5, 3.0, 2.0))
    elif name == "quant":
        x = torch.round(torch.randn(shape, generator=g) * 8) / 4
    elif name == "lowbyte":
        j = torch.randint(0, 256, shape, generator=g)
        x = -sign * (1.0 + j.float() * 2.0 ** -23)
    elif name == "exponent":
        k = torch.randint(-20, 21, shape, generator=g)
        x = torch.where(torch.rand(shape, generator=g) < 0.5, 1.0, -1.0) * torch.pow(2.0, k.float())
    elif name == "ramp":
        err = (torch.arange(p).float() - float(p // 3)) * 2.0 ** -10
        x = sign * (1.0 - err.view(1, c, h, w))
    elif name == "gauss":
        x = torch.randn(shape, generator=g) * 3
    else:
        raise KeyError(name)
    x = x.float().contiguous()
    err = (1.0 - sign * x).reshape(n, -1)
    assert err.dtype == torch.float32
    distinct = [int(torch.unique(e).numel()) for e in err]
    if name == "const":
        assert distinct == [1] * n
    elif name == "two":
        assert sorted(torch.unique(err).tolist()) == [-2.0, 4.0]
    elif name == "four":
        assert sorted(torch.unique(err).tolist()) == [-2.0, -1.0, 3.0, 4.0]
    elif name == "quant":
        assert max(distinct) <= 100 and bool((err == 0).any()) and bool((err < 0).any())
    elif name == "lowbyte":
        bits = err.view(torch.int32)
        assert bool((bits >> 8 == bits.view(-1)[0] >> 8).all()) and max(distinct) > min(p, 128) // 4
    elif name == "exponent":
        assert max(distinct) <= 82 and bool((err < 0).any())
    elif name == "ramp":
        assert bool((err[:, 1:] > err[:, :-1]).all()) and bool((err == 0).any())
    return x, y


def ignored_mask(pattern, shape, seed=0):
    """bool [N, H, W]: ``none``; ``rows`` (a block of rows of every image); ``scattered`` (about 30 %); ``image`` (the last image
    wholly, the others scattered)."""

    n, _, h, w = shape
    g = torch.Generator().manual_seed(5000 + seed)
    m = torch.zeros(n, h, w, dtype=torch.bool)
    if pattern == "rows":
        m[:, h // 3: h // 3 + max(h // 4, 1)] = True
    elif pattern in ("scattered", "image"):
        m = torch.rand(n, h, w, generator=g) < 0.3
        assert 0.15 < float(m.float().mean()) < 0.45
        if pattern == "image":
            m[-1] = True
    elif pattern != "none":
        raise KeyError(pattern)
    assert bool(m.any()) == (pattern != "none") and not bool(m[0].all())
    return m
