"""Float64 references, seeded inputs and the one comparison of the streaming-kernel tests (TEST INFRASTRUCTURE ONLY).

The streaming kernels are the head (``self.final`` forward with its softmax / quantise / argmax epilogues, and its backward),
max-pool, the nearest-x2 upsample gradient with the ``torch.cat`` split, the stride-2 scatter and train-mode BatchNorm
(csrc/elementwise.hip, csrc/backward.hip, csrc/bn.hip).  Every reference here is the operation's definition (reference
unet.py, torch.nn.functional) evaluated in float64 on the CPU with plain tensor algebra -- none calls the project's code and
none follows a kernel's loop structure; tests/test_stream_ref_cpu.py checks each against torch's own float64 operators and
autograd.  Activations are NHWC ``[N,H,W,C]`` as the kernels take them, logits NCHW.

``compare`` differs from the max-norm ``close()`` of the older tests: every output ELEMENT is measured against its own scale,
the float64 sum of the absolute values of the terms that make it up (``max(|want|, tiny)`` for an elementwise operation), so
a wrong element of small magnitude cannot hide behind a large one elsewhere in the tensor, and an element that has to be
exactly 0 (a masked gradient) fails on any other value.  An output STORED as bf16 is compared with the float64 result
rounded to bf16, with one bf16 ulp of that element on top of the bar: a correct kernel rounds its fp32 value once, and that
value can lie on the other side of a rounding boundary from the float64 one."""

import numpy as np
import torch

BF16 = torch.bfloat16
TINY = 1e-30  # floor of a scale: below it fp32 has underflowed (1.2e-38 is the smallest normal) and 0 is as good an answer

# The bars, in units of the element's scale.  LIMITS are what the older tests use for the same quantities (1e-5 head logits /
# probabilities, 3e-4 head gradients and BatchNorm forward, 1e-5 running buffers, 1e-3 BatchNorm backward) and, for the two
# few-term sums, what the number format gives: <= 5 fp32 terms are 4 roundings of 2^-24 each, 2.4e-7 of the scale.  BARS are
# what ``compare`` asserts: a limit that the MI355X met with more than 100x to spare is replaced by about 10x the largest
# distance measured there (the figures are in the docstring of tests/test_gpu_streaming.py).  The head's logits and
# probabilities have 21x and 36x to spare and keep 1e-5 as their limit, but are asserted against ``head_bars(Cin)`` below it.
LIMITS = {
    "logits": 1e-5, "probs": 1e-5,
    "head dx": 3e-4, "head dW": 3e-4, "head db": 3e-4,
    "pool grad": 1e-6, "upsample grad": 1e-6,
    "bn mean": 3e-4, "bn invstd": 3e-4, "bn scale": 3e-4, "bn shift": 3e-4, "bn z": 3e-4,
    "running_mean": 1e-5, "running_var": 1e-5,
    "bn dy": 1e-3, "bn dgamma": 1e-3, "bn dbeta": 1e-3,
}
BARS = dict(LIMITS)
BARS.update({
    "head dx": 2e-6, "head dW": 1e-6, "head db": 5e-7,
    "bn mean": 6e-7, "bn invstd": 8e-7, "bn scale": 1e-6, "bn shift": 2e-6, "bn z": 1e-6,
    "bn dy": 1e-5, "bn dgamma": 2e-6, "bn dbeta": 6e-7,
})
assert all(BARS[k] <= LIMITS[k] for k in LIMITS)


def head_bars(cin):
    """(logit bar, probability bar) of a head with Cin input channels, from the number format: a logit is Cin fused multiply-adds
    and the bias add, Cin + 1 roundings of 2^-24 each relative to the sum of the absolute terms in ANY order of summation; a
    probability carries that (through ``prob_scale``) plus the rounding of the subtraction of the maximum, expf (1 ulp), a sum of
    <= 8 terms and a division (2.5 ulp): 12 more.  Cin <= 128: 7.7e-6 and 8.4e-6, below the limits of 1e-5."""

    u = 2.0 ** -24
    return (cin + 1) * u, (cin + 13) * u


def gen(seed):
    return torch.Generator().manual_seed(seed)


def q_bf16(t):
    """``t`` rounded to bf16 and back (what a bf16 kernel is given)."""

    return t.to(BF16).to(t.dtype)


def bf16_ulp(v):
    """One unit in the last place of bf16 (8 significant bits) at each element of float64 ``v``; 0 where v == 0."""

    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))  # |v| = m * 2^e, m in [0.5, 1)
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 8))


# ---- the comparison -------------------------------------------------------------------------------------------------------

def distance(got, want, scale, bf16=False):
    """Largest |got - want| / max(scale, TINY) over the elements (scale: a tensor like ``want`` or a number).  ``bf16``: want is
    rounded to bf16 first and one bf16 ulp of it is taken off the difference.  NaN if anything in ``got`` is NaN."""

    got, want = got.detach().double().cpu(), want.detach().double()
    assert tuple(got.shape) == tuple(want.shape), (got.shape, want.shape)
    if got.numel() == 0:
        return 0.0
    if bf16:
        want = want.float().to(BF16).double()
    err = (got - want).abs()
    err = torch.where(got == want, torch.zeros_like(err), err)  # (inf == inf)
    if bf16:
        err = (err - bf16_ulp(want)).clamp_min(0)
    if not torch.is_tensor(scale):
        scale = torch.full_like(want, float(scale))
    d = err / scale.double().clamp_min(TINY)
    return float("nan") if bool(torch.isnan(d).any()) else float(d.max())


def compare(quantity, got, want, scale, what="", record=None, bf16=False, bar=None):
    """Asserts distance(got, want, scale) <= the bar of ``quantity`` (``BARS``) and returns the distance.  NaN fails.  The
    distance is printed, and kept in ``record[quantity]`` as a running maximum when a dict is given."""

    bar = BARS[quantity] if bar is None else bar
    d = distance(got, want, scale, bf16)
    print("{} {}: distance {:.2e} (bar {:.0e}){}".format(quantity, what, d, bar, " [bf16 store]" if bf16 else ""))
    assert d == d, "{} {}: NaN".format(quantity, what)
    if record is not None:
        record[quantity] = max(record.get(quantity, 0.0), d)
    assert d <= bar, "{} {}: distance {:.3e} > {:.0e}".format(quantity, what, d, bar)
    return d


# ---- head forward ---------------------------------------------------------------------------------------------------------

def head_fwd(x, w, b):
    """self.final = Conv2d(Cin, C, 1) on NHWC x [N,H,W,Cin] with w [C,Cin], b [C], then softmax over the classes.  Returns a
    dict of float64 NCHW tensors: logits, logit_scale (sum_k |x_k w_ck| + |b_c|), probs, prob_scale and the argmax byte."""

    x64, w64, b64 = x.double(), w.double(), b.double()
    logits = (torch.einsum("nhwk,ck->nchw", x64, w64) + b64.view(1, -1, 1, 1)).contiguous()
    lscale = (torch.einsum("nhwk,ck->nchw", x64.abs(), w64.abs()) + b64.abs().view(1, -1, 1, 1)).contiguous()
    probs = torch.softmax(logits, dim=1)
    # d p_c = p_c (d l_c - sum_j p_j d l_j): an error of eps * L_j in logit j moves p_c by at most eps * p_c * (L_c + sum_j p_j L_j);
    # the exp and the division add a few eps * p_c
    pscale = probs * (1.0 + lscale + (probs * lscale).sum(1, keepdim=True))
    return {"logits": logits, "logit_scale": lscale, "probs": probs, "prob_scale": pscale,
            "argmax": torch.from_numpy(np.argmax(logits.numpy(), axis=1).astype(np.uint8))}


ANCHORS = np.linspace(0, 1, 256)


def head_quantize(probs, overlap):
    """tools/predict.py: np.digitize(p, np.linspace(0,1,256)).astype(np.uint8) of every non-background class of NCHW ``probs``
    after the crop of ``overlap``: [N,H',W'] for C = 2, [N,H',W',C-1] otherwise.  Returns (bytes, bins before the uint8 wrap,
    the cropped probabilities, the distance of each to the nearest anchor), the last three as [N,H',W',C-1]."""

    n, c, h, w = probs.shape
    p = probs[:, 1:, overlap:h - overlap, overlap:w - overlap].permute(0, 2, 3, 1).contiguous().numpy()
    bins = np.digitize(p, ANCHORS)
    q = bins.astype(np.uint8)
    near = np.abs(p[..., None] - ANCHORS).min(-1)
    return (q[..., 0] if c == 2 else q), bins, p, near


def quantize_check(got, probs, prob_scale, overlap, bar):
    """The issue's rule for the bytes of the device: a byte may differ from the float64 one by exactly one bin, and only where the
    float64 probability lies within ``bar`` * scale of an anchor.  Returns (bytes compared, bytes that differ, bytes that were
    allowed to).  ``got``: uint8 array in the layout of ``head_quantize``."""

    n, c, h, w = probs.shape
    want, bins, p, near = head_quantize(probs, overlap)
    s = prob_scale[:, 1:, overlap:h - overlap, overlap:w - overlap].permute(0, 2, 3, 1).numpy()
    got = np.asarray(got).reshape(bins.shape).astype(np.int64)
    assert got.shape == bins.shape
    gbin = np.where((got == 0) & (bins >= 255), 256, got)  # undo the uint8 wrap of bin 256 next to where it can occur
    diff = np.abs(gbin - bins)
    allowed = near <= bar * s  # (no floor: a probability of 1e-50 is bin 1 for any kernel that returns p >= 0)
    assert int(diff.max(initial=0)) <= 1, "a byte is {} bins off".format(int(diff.max()))
    assert not bool(((diff == 1) & ~allowed).any()), "a byte differs where the float64 probability is not within the bar of an anchor"
    return bins.size, int((diff == 1).sum()), int(allowed.sum())


def argmax_check(got, logits, logit_scale, bar):
    """The device's class byte may differ from the float64 argmax only where the two largest float64 logits are closer than
    ``bar`` * (their scales added).  Returns (pixels, pixels that differ, pixels that were allowed to)."""

    top = torch.topk(logits, 2, dim=1)
    gap = (top.values[:, 0] - top.values[:, 1]).numpy()
    s = torch.gather(logit_scale, 1, top.indices).sum(1).numpy()
    want = np.argmax(logits.numpy(), axis=1)
    got = np.asarray(got).astype(np.int64)
    assert got.shape == want.shape
    allowed = gap <= bar * s
    differ = got != want
    assert not bool((differ & ~allowed).any()), "argmax differs where the two largest float64 logits are further apart than the bar"
    # where it differs it must still be one of the two largest
    second = top.indices[:, 1].numpy()
    assert bool((~differ | (got == second)).all())
    return want.size, int(differ.sum()), int(allowed.sum())


# ---- head backward --------------------------------------------------------------------------------------------------------

def head_bwd(x, w, dl, relu_mask):
    """Gradients of logits = conv1x1(x) w.r.t. x (NHWC, times (x > 0) when ``relu_mask``: x is a ReLU output), w and b for
    the NCHW logit gradient ``dl``.  Returns float64 dx, dW, db and their scales (sums of absolute terms)."""

    x64, w64, d64 = x.double(), w.double(), dl.double()
    dx = torch.einsum("nchw,ck->nhwk", d64, w64)
    sdx = torch.einsum("nchw,ck->nhwk", d64.abs(), w64.abs())
    if relu_mask:
        keep = (x64 > 0).double()
        dx, sdx = dx * keep, sdx * keep
    dw = torch.einsum("nchw,nhwk->ck", d64, x64)
    sdw = torch.einsum("nchw,nhwk->ck", d64.abs(), x64.abs())
    return {"dx": dx, "dx_scale": sdx, "dW": dw, "dW_scale": sdw, "db": d64.sum((0, 2, 3)), "db_scale": d64.abs().sum((0, 2, 3))}


# ---- max-pool -------------------------------------------------------------------------------------------------------------

def pool_out(size, k, s, p):
    return (size + 2 * p - k) // s + 1


def _windows(x, k, s, p):
    """[k*k, N, Ho, Wo, C] float64 window taps of NHWC ``x`` in row-major tap order and the bool [k*k, Ho, Wo] of the taps that
    lie inside the image."""

    n, h, w, c = x.shape
    ho, wo = pool_out(h, k, s, p), pool_out(w, k, s, p)
    pad = torch.full((n, h + 2 * p + k, w + 2 * p + k, c), float("-inf"), dtype=torch.float64)
    pad[:, p:p + h, p:p + w] = x.double()
    inside = torch.zeros(h + 2 * p + k, w + 2 * p + k, dtype=torch.bool)
    inside[p:p + h, p:p + w] = True
    taps, valid = [], []
    for r in range(k):
        for t in range(k):
            taps.append(pad[:, r:r + (ho - 1) * s + 1:s, t:t + (wo - 1) * s + 1:s])
            valid.append(inside[r:r + (ho - 1) * s + 1:s, t:t + (wo - 1) * s + 1:s])
    return torch.stack(taps), torch.stack(valid)


def maxpool_fwd(x, k, s, p):
    """F.max_pool2d(x, k, s, p) on NHWC x: (value float64 [N,Ho,Wo,C], winning tap int64 r*k+t in window coordinates).  The
    winner is the FIRST maximum of the taps inside the image in row-major order; a NaN beats everything and the LAST NaN of
    the window is the one recorded (torch: ``val > maxval || isnan(val)`` tap after tap)."""

    taps, valid = _windows(x, k, s, p)
    t, n, ho, wo, c = taps.shape
    v = valid.view(t, 1, ho, wo, 1).expand_as(taps)
    isn = torch.isnan(taps) & v
    clean = torch.where(isn | ~v, torch.full_like(taps, float("-inf")), taps)
    best = clean.max(0).values
    order = torch.arange(t).view(t, 1, 1, 1, 1).expand_as(taps)
    first_max = torch.where((clean == best) & v, order, torch.full_like(order, t)).min(0).values
    last_nan = torch.where(isn, order, torch.full_like(order, -1)).max(0).values
    has_nan = last_nan >= 0
    value = torch.where(has_nan, torch.full_like(best, float("nan")), best)
    tap = torch.where(has_nan, last_nan, first_max)
    assert int(tap.max()) < t
    return value, tap


def maxpool_bwd(dy, tap, in_shape, k, s, p, base=None):
    """Gradient of the pooling input: each window's ``dy`` lands on its winning tap (plus ``base`` when given).  Returns
    (dx float64 NHWC, scale = sum of the absolute terms, number of windows that contribute to each element)."""

    n, h, w, c = in_shape
    _, ho, wo, _ = dy.shape
    d = dy.double().numpy()
    tp = tap.numpy()
    dx, sc, cnt = np.zeros(in_shape), np.zeros(in_shape), np.zeros(in_shape, dtype=np.int64)
    ni, oy, ox, ci = np.meshgrid(np.arange(n), np.arange(ho), np.arange(wo), np.arange(c), indexing="ij")
    iy, ix = oy * s - p + tp // k, ox * s - p + tp % k
    assert iy.min() >= 0 and iy.max() < h and ix.min() >= 0 and ix.max() < w
    np.add.at(dx, (ni, iy, ix, ci), d)
    np.add.at(sc, (ni, iy, ix, ci), np.abs(d))
    np.add.at(cnt, (ni, iy, ix, ci), 1)
    dx, sc = torch.from_numpy(dx), torch.from_numpy(sc)
    if base is not None:
        dx, sc = dx + base.double(), sc + base.double().abs()
    return dx, sc, torch.from_numpy(cnt)


# ---- upsample / split / scatter -------------------------------------------------------------------------------------------

def upsample_split_bwd(dup, c1, c2, mask1=None, mask2=None, base1=None, summed=True):
    """Gradient of torch.cat([a, b], C) -> F.interpolate(scale_factor=2, mode="nearest") for the NHWC gradient ``dup``
    [N,2H,2W,C1+C2] (``summed=False``: of the cat alone, ``dup`` [N,H,W,C1+C2]): every source element collects its 2x2 copies.
    ``mask1`` / ``mask2``: a and b are ReLU outputs, the gradient is zeroed where they are <= 0; ``base1`` is added to d1.
    Returns (d1, scale1, d2, scale2) in float64 (d2, scale2 None when C2 == 0)."""

    d = dup.double()
    if summed:
        n, h2, w2, ct = d.shape
        blocks = d.view(n, h2 // 2, 2, w2 // 2, 2, ct)
        g, sg = blocks.sum((2, 4)), blocks.abs().sum((2, 4))
    else:
        g, sg = d, d.abs()
    d1, s1 = g[..., :c1], sg[..., :c1]
    d2, s2 = (g[..., c1:], sg[..., c1:]) if c2 else (None, None)
    if mask1 is not None:
        keep = (mask1.double() > 0).double()
        d1, s1 = d1 * keep, s1 * keep
    if mask2 is not None and c2:
        keep = (mask2.double() > 0).double()
        d2, s2 = d2 * keep, s2 * keep
    if base1 is not None:
        d1, s1 = d1 + base1.double(), s1 + base1.double().abs()
    return d1.contiguous(), s1.contiguous(), (d2.contiguous() if c2 else None), (s2.contiguous() if c2 else None)


def scatter_add_stride2(t, out):
    """out[:, ::2, ::2] += t in float64 (a copy; ``out`` [N,Ho,Wo,C] with Ho in {2 Hs - 1, 2 Hs}) and the bool mask of the
    positions it touches."""

    o = out.double().clone()
    n, hs, ws, c = t.shape
    o[:, ::2, ::2][:, :hs, :ws] += t.double()
    touched = torch.zeros(out.shape, dtype=torch.bool)
    touched[:, ::2, ::2][:, :hs, :ws] = True
    return o, touched


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------

def bn_stats(y, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """Train-mode BatchNorm2d statistics of y viewed as [M, C] (two passes in float64 over the given values): mean, biased
    variance -> invstd, scale = gamma * invstd, shift = beta - mean * scale, and the running buffers after one step
    (unbiased variance, momentum).  Values and ``*_scale`` entries in one dict."""

    c = y.shape[-1]
    y64 = y.double().reshape(-1, c)
    m = y64.shape[0]
    mean = y64.mean(0)
    var = ((y64 - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    g64, b64 = gamma.double(), beta.double()
    scale = g64 * invstd
    out = {"mean": mean, "mean_scale": y64.abs().mean(0), "var": var, "invstd": invstd, "invstd_scale": invstd.abs(),
           "scale": scale, "scale_scale": scale.abs(), "shift": b64 - mean * scale, "shift_scale": b64.abs() + (mean * scale).abs()}
    if running_mean is not None:
        unbiased = var * (m / (m - 1.0)) if m > 1 else var
        rm, rv = running_mean.double(), running_var.double()
        out["running_mean"] = (1 - momentum) * rm + momentum * mean
        out["running_mean_scale"] = (1 - momentum) * rm.abs() + momentum * mean.abs()
        out["running_var"] = (1 - momentum) * rv + momentum * unbiased
        out["running_var_scale"] = (1 - momentum) * rv.abs() + momentum * unbiased
    return out


def bn_apply(y, scale, shift, residual=None, relu=False):
    """z = relu?(y * scale + shift (+ residual)) in float64 and the scale |y scale| + |shift| (+ |residual|)."""

    z = y.double() * scale.double() + shift.double()
    s = (y.double() * scale.double()).abs() + shift.double().abs()
    if residual is not None:
        z, s = z + residual.double(), s + residual.double().abs()
    return (torch.relu(z) if relu else z), s


def mask_bits(z):
    """uint8 [numel/8]: bit e of byte i is (element 8 i + e of ``z`` > 0)."""

    return torch.from_numpy(np.packbits((z.reshape(-1) > 0).numpy().astype(np.uint8), bitorder="little"))


def bn_bwd(dz, zmask, y, gamma, eps, mean=None, invstd=None):
    """Backward of train-mode BatchNorm (+ the ReLU behind it: g = dz * (zmask > 0) when ``zmask`` is given) in float64:
    dbeta = sum g, dgamma = sum g xhat, dy = gamma invstd (g - mean(g) - xhat mean(g xhat)); ``g`` is also the gradient of
    the residual branch.  ``mean`` / ``invstd``: the forward's saved statistics (default: of ``y`` itself, in float64)."""

    c = y.shape[-1]
    y64, g = y.double().reshape(-1, c), dz.double().reshape(-1, c)
    if zmask is not None:
        g = g * (zmask.double().reshape(-1, c) > 0).double()
    m = y64.shape[0]
    if mean is None:
        mean = y64.mean(0)
        invstd = 1.0 / torch.sqrt(((y64 - mean) ** 2).mean(0) + eps)
    mean, invstd = mean.double(), invstd.double()
    xhat = (y64 - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    k1 = gamma.double() * invstd
    dy = k1 * (g - dbeta / m - xhat * dgamma / m)
    sdy = k1.abs() * (g.abs() + dbeta.abs() / m + (xhat * dgamma / m).abs())
    return {"dy": dy.reshape(y.shape), "dy_scale": sdy.reshape(y.shape), "dgamma": dgamma, "dgamma_scale": (g * xhat).abs().sum(0),
            "dbeta": dbeta, "dbeta_scale": g.abs().sum(0), "dmasked": g.reshape(y.shape)}


# ---- seeded inputs --------------------------------------------------------------------------------------------------------

HEAD_SHAPES = [(3, 7, 9), (2, 17, 31)]  # P = 189: one partial block with both image borders in it; P = 1054 = 4 * 256 + 30
HEAD_BIG = (2, 257, 511)  # P = 262 654 = 1025 * 256 + 254: 1026 tiles over 1024 blocks, HW = 131 327 = 512 * 256 + 255


def head_case(n, h, w, cin, c, seed, bf16=False, relu=False, wscale=0.3, plant=0.0, plant_w=1.0, plant_last=True):
    """x [N,H,W,Cin] = randn (ReLU'd when ``relu``: exact zeros, as dec5's output), w [C,Cin] = randn * wscale, b [C] = randn;
    x rounded to bf16 when ``bf16``.  ``plant`` = A > 0: w[:, 0] = (0, 1, .., C-1) * plant_w and two pixels next to the centre of
    the first image are 0 except channel 0 = +A / plant_w (the last class leads every other by about A or more) and -A / plant_w
    (class 0 leads); the same with A * 2/3 in the last image when ``plant_last``."""

    g = gen(seed)
    x = torch.randn(n, h, w, cin, generator=g)
    if relu:
        x = torch.relu(x)
    wt = torch.randn(c, cin, generator=g) * wscale
    b = torch.randn(c, generator=g)
    if plant:
        wt[:, 0] = torch.arange(c, dtype=torch.float32) * plant_w
        for img, a in ((0, plant / plant_w), (n - 1, plant * 2 / 3 / plant_w))[:2 if plant_last else 1]:
            x[img, h // 2, w // 2] = 0
            x[img, h // 2, w // 2, 0] = a
            x[img, h // 2, w // 2 - 1] = 0
            x[img, h // 2, w // 2 - 1, 0] = -a
    if bf16:
        x = q_bf16(x)
    return x, wt, b


QUANT_CLASSES = (2, 3, 5)
QUANT_CIN = (32, 8)


def max_overlap(h, w):
    """The largest overlap that leaves a crop one pixel wide (H, W odd)."""

    return (min(h, w) - 1) // 2


def quantize_cases(cin, bf16):
    """The (x, w, b, overlap) of the quantise tests for one input width and type: C in {2, 3, 5}, both head shapes (H != W),
    overlap 0 / 1 / the largest, weights * 0.05 and a planted column * 2^-4 (logit scales of a few units, so that few
    probabilities lie within the bar of an anchor) and, in the first image, planted pixels with a lead of 120: probability exactly 1.0
    (bin 256 -> byte 0) and exp(-120) (fp32: 0, byte 1) -- in float64 too."""

    for c in QUANT_CLASSES:
        for n, h, w in HEAD_SHAPES:
            x, wt, b = head_case(n, h, w, cin, c, seed=300 + 10 * c + cin, bf16=bf16, wscale=0.05, plant=120.0, plant_w=0.0625, plant_last=False)
            for ov in (0, 1, max_overlap(h, w)):
                yield x, wt, b, ov


ARGMAX_CLASSES = (2, 3, 5, 8)


def argmax_cases(cin, bf16):
    for c in ARGMAX_CLASSES:
        for n, h, w in HEAD_SHAPES:
            yield head_case(n, h, w, cin, c, seed=400 + 10 * c + cin, bf16=bf16)


def tie_case(n, h, w, cin, c, seed, bf16=False):
    """Rows 1 and 2 of w (rows 0 and 1 for C = 2) are identical with equal biases 1 above the others': the two classes tie
    exactly on every pixel and lead on many.  Returns (x, w, b, lower index of the pair)."""

    x, wt, b = head_case(n, h, w, cin, c, seed, bf16=bf16)
    lo = 0 if c == 2 else 1
    wt[lo + 1] = wt[lo]
    b[lo] = b[lo + 1] = float(b.max()) + 1.0
    return x, wt, b, lo


def probe_pixels(n, h, w):
    """Flat pixel indices a head-backward probe visits: the first, the last (of the ragged tile), the two either side of the
    first image border, and -- where there is one -- the first pixel of the first tile a block takes on its second trip."""

    hw, p = h * w, n * h * w
    out = [0, hw - 1, hw, p - 1]
    if p > 1024 * 256:
        out.append(1024 * 256)
    return out


POOL_PARAMS = [(3, 2, 1), (2, 2, 0)]
POOL_SHAPES = [(17, 23), (1, 1), (2, 3)]


def pool_input(n, h, w, c, seed, special=True):
    """ReLU'd randn on a 0.25 grid (exact ties and zeros everywhere; bf16-exact) with, when there is room, an all-equal
    window, -inf entries (a whole 3x3 neighbourhood of them too) and NaNs at the first, a middle and the last tap of windows."""

    g = gen(seed)
    x = torch.round(torch.relu(torch.randn(n, h, w, c, generator=g)) * 4) / 4
    if special and h >= 13 and w >= 18:
        x[0, 0:4, 0:4, :] = 1.5  # all-equal windows
        x[0, 5:10, 5:10, 0] = float("-inf")  # windows of -inf alone
        x[0, 2, 9, 1] = float("-inf")
        # for k = 3, s = 2, p = 1 the window of output (oy, ox) covers rows 2 oy - 1 .. 2 oy + 1: (3, 11) is the first tap of
        # output (2, 6), (6, 14) its middle tap of output (3, 7), (11, 17) the last tap of output (5, 8); for k = 2, s = 2, p = 0
        # they are tap 3 of (1, 5), tap 0 of (3, 7) and tap 3 of (5, 8)
        for (yy, xx) in ((3, 11), (6, 14), (11, 17)):
            x[-1, yy, xx, :] = float("nan")
        x[-1, 12, 2, 0] = float("nan")  # two NaNs in one window: the last one is recorded
        x[-1, 12, 3, 0] = float("nan")
    return x


def bn_input(m, c, seed, offset=0.0, spread=1.0, bf16=False):
    g = gen(seed)
    y = offset + spread * torch.randn(m, c, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    return (q_bf16(y) if bf16 else y), gamma, beta, rm, rv
