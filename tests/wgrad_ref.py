"""Reference, generators, launch-plan restatements and the case tables of the weight-gradient edge tests
(tests/test_gpu_wgrad_edges.py on the MI355X, tests/test_wgrad_ref_cpu.py without one).

Reference.  The filter gradient is autograd's, in float64, on the reference formulation: ``F.conv2d(x, w, stride, padding)`` for a
plain layer, ``F.conv2d(F.interpolate(cat[a, b], scale_factor=2, mode="nearest"), w, padding=1)`` for DecoderBlock; returned KRSC.
``wgrad_loops`` is a second restatement (an explicit loop over taps with index arithmetic instead of conv2d / interpolate) that the
CPU test holds against it on tiny shapes, and ``pulse_window`` a third (one window of the gathered input).

Exactness.  ``x`` and ``dy`` are integers in [-2, 2] (bf16 values).  A kernel that multiplies operand pairs and adds them in fp32
-- the tap-per-block, phase and thin kernels, the split reduction and the phase combine -- forms only integers bounded by
S = sum |dy| |x|, and ``magnitude`` computes S by the same autograd on absolute values: S < 2^24 is asserted per case, so any summation
order, MFMA shape or split gives the reference's bits.  The two Winograd-domain kernels add transformed operands; read from their code:

  conv_wgrad_wino_f32 (DecoderBlock, F(2x2, 2x2)): Z = A dY A^T with A = [1 0; 1 1; 0 1] is computed as sums of at most four dz values,
      V = B^T d B with B^T = [1 -1 0; 0 1 0; 0 -1 1] as differences of at most four source values (T = d - d, then V = T - T): all
      integers, |Z| <= 4 D, |V| <= 4 X.  dU = sum over the tiles of Z V: integers, |dU| <= 16 D X T for T tiles.  The finish kernel adds
      four dU per parity (G = [1 0; 1 1; 0 1]: no fractions) and four parities per tap: |.| <= 256 D X T.
  conv_wgrad_wino33_f32 (stride-1 3x3, F(2x2, 3x3)): Z = A dY A^T (A^T = [1 1 1 0; 0 1 -1 -1] restricted to the tile's 2x2 dy) and
      V = B^T d B (two non-zeros per row of B^T) are sums of at most four values each, computed rows first, then columns: integers,
      |dU| <= 16 D X T.  The finish kernel applies G^T . G with G's halves as h = 0.5 u (exact: a power of two), t = u0 + (h1 + h2),
      h1 - h2, (h1 + h2) + u3 -- multiples of 1/2 bounded by 2 |u| -- and the same again on the columns: multiples of 1/4 bounded by
      4 |u|, that is 16 |u| <= 256 D X T quarter-units.

So for both, ``wino_bound`` = 256 D X T < 2^24 (units of 1/4 for wino33) makes every intermediate a dyadic number that fp32 holds
exactly: with D = X = 2 and at most a few hundred tiles the cases here stay below 2^21.  No step of either kernel is inexact on such
data, so both are held to torch.equal like the rest.

Plans.  ``bf16_plan``, ``thin_plan``, ``f32_plan`` (with ``w33_plan`` / ``ww_plan``) and ``reduce_plan`` restate plan() of
conv_wgrad_bf16.hip, rs_wgrad_thin_plan, plan() of conv_wgrad.hip (and of the two Winograd files) and rs_reduce_splits under a given
knob setting.  A case states what it aims at (``aim``); the CPU test compares aim, restatement and library, so that after a change
of launch policy a case says that it no longer aims at anything."""

import collections
import functools

import torch
import torch.nn.functional as F

EXACT = float(1 << 24)

# the shipped knob settings the restatements start from (csrc/common.h: RsKnobs)
DEFAULT_KNOBS = dict(wgrad_blocks=96, wgrad_blocks_phase=1536, wgrad_phase4=1, wgrad_blocks_phase4=256, wgrad_ring=3,
                     wgrad_f32_phase=1, wgrad_f32_dma=-1, wgrad_f32_blocks=2048, wgrad_f32_wino=1, wgrad_f32_wino_blocks=1024,
                     wgrad_f32_wino33=1, wgrad_f32_wino33_blocks=256)


class Case(collections.namedtuple("Case", "name n h w c1 c2 cout k stride pad ups")):
    """One layer: source [n, c1 (+ c2), h, w], read through the nearest-x2 upsample when ``ups``; k x k filter."""

    __slots__ = ()

    @property
    def ho(self):
        return ((2 * self.h if self.ups else self.h) + 2 * self.pad - self.k) // self.stride + 1

    @property
    def wo(self):
        return ((2 * self.w if self.ups else self.w) + 2 * self.pad - self.k) // self.stride + 1

    @property
    def m(self):
        return self.n * self.ho * self.wo

    @property
    def cin(self):
        return self.c1 + self.c2

    def desc(self):
        """The fields of rs_conv_desc, in order."""
        return (self.n, self.h, self.w, self.c1, self.c2, self.ups, self.k, self.k, self.stride, self.pad, self.ho, self.wo, self.cout, 0, 0)


def plain(name, n, h, w, c1, cout, k=3, stride=1, pad=None, c2=0):
    return Case(name, n, h, w, c1, c2, cout, k, stride, k // 2 if pad is None else pad, 0)


def decoder(name, n, h, w, c1, c2, cout):
    return Case(name, n, h, w, c1, c2, cout, 3, 1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# generators and the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).double()


def randn(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed), dtype=torch.float64)


def round_bf16(t):
    return t.float().to(torch.bfloat16).double()


def operands(case, kind="int", seed=0):
    """(a, b, dy) NCHW float64 on the host; b is None for one source.  kind: "int" [-2, 2], "randn" (fp32 values) or "randn_bf16"."""
    shapes = ((case.n, case.c1, case.h, case.w), (case.n, case.c2, case.h, case.w), (case.n, case.cout, case.ho, case.wo))
    if kind == "int":
        a, b, dy = (ints(-2, 2, *s, seed=seed + i) for i, s in enumerate(shapes))
    else:
        a, b, dy = (randn(*s, seed=seed + i).float().double() for i, s in enumerate(shapes))
        if kind == "randn_bf16":
            a, b, dy = round_bf16(a), round_bf16(b), round_bf16(dy)
    return a, (b if case.c2 else None), dy


def forward(case, a, b, w):
    x = a if b is None else torch.cat([a, b], 1)
    if case.ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, w, stride=case.stride, padding=case.pad)


def wgrad(case, a, b, dy):
    """KRSC filter gradient by autograd, in the dtype of the operands."""
    w = torch.zeros(case.cout, case.cin, case.k, case.k, dtype=a.dtype, requires_grad=True)
    forward(case, a, b, w).backward(dy)
    return w.grad.permute(0, 2, 3, 1).contiguous()


def magnitude(case, a, b, dy):
    """S = sum |dy| |x| per element: the same autograd on absolute values."""
    return wgrad(case, a.abs(), None if b is None else b.abs(), dy.abs())


def gathered(case, a, b):
    """The convolution's input as the kernels gather it: concat, upsample by index arithmetic, zero padding.  [n, C, Hv + 2 pad, Wv + 2 pad]."""
    x = a if b is None else torch.cat([a, b], 1)
    if case.ups:
        iy, ix = torch.arange(2 * case.h) // 2, torch.arange(2 * case.w) // 2
        x = x[:, :, iy][:, :, :, ix]
    out = torch.zeros(x.shape[0], x.shape[1], x.shape[2] + 2 * case.pad, x.shape[3] + 2 * case.pad, dtype=x.dtype)
    out[:, :, case.pad:case.pad + x.shape[2], case.pad:case.pad + x.shape[3]] = x
    return out


def wgrad_loops(case, a, b, dy):
    """The second restatement: dW[co][ky][kx][ci] = sum_m dy[m][co] * in[n][oy * stride - pad + ky][ox * stride - pad + kx][ci], tap by tap."""
    xin = gathered(case, a, b)
    dw = torch.zeros(case.cout, case.k, case.k, case.cin, dtype=a.dtype)
    for ky in range(case.k):
        for kx in range(case.k):
            for oy in range(case.ho):
                for ox in range(case.wo):
                    col = xin[:, :, oy * case.stride + ky, ox * case.stride + kx]  # [n, cin]
                    dw[:, ky, kx, :] += dy[:, :, oy, ox].t() @ col
    return dw


def pulse_window(case, a, b, pos):
    """[k, k, cin]: the window of the gathered input under output pixel pos = (n, oy, ox), zeros outside the image."""
    n, oy, ox = pos
    xin = gathered(case, a, b)
    return xin[n, :, oy * case.stride:oy * case.stride + case.k, ox * case.stride:ox * case.stride + case.k].permute(1, 2, 0).contiguous()


def wino_tiles(case):
    """2x2 tiles the Winograd-domain kernels reduce over (of output pixels for wino33, of source positions for DecoderBlock)."""
    return case.n * ((case.h + 1) // 2) * ((case.w + 1) // 2)


def wino_bound(case, dmax, xmax):
    """256 D X T (see the module docstring): must stay below 2^24."""
    return 256.0 * dmax * xmax * wino_tiles(case)


@functools.lru_cache(maxsize=None)
def exact_problem(case):
    """(a, b, dy, ref KRSC, S) on integer data; computed once per case and shared: do not modify."""
    a, b, dy = operands(case, "int", seed=1000)
    return a, b, dy, wgrad(case, a, b, dy), magnitude(case, a, b, dy)


# ---------------------------------------------------------------------------------------------------------------------------------
# launch plans
# ---------------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def largest_tile(c):
    return 128 if c % 128 == 0 else 64 if c % 64 == 0 else 32


def is_decoder(c):
    return c.ups == 1 and c.k == 3 and c.stride == 1 and c.pad == 1  # (Ho = 2 Hs follows)


def reduce_plan(n, splits):
    """rs_reduce_splits: one level up to 8 splits, else L lanes per column, then their sum.  (levels, L, scratch floats)"""
    if splits <= 8:
        return dict(levels=1, L=1, scratch=0)
    return dict(levels=2, L=max(2, min(32, 131072 // (n // 4), splits // 2)), scratch=32 * n)


def _split(chunks, tiles, target, min_chunks, fits, refuse=False):
    """(chunks per split, splits): s = ceil(target / tiles) splits of at least ``min_chunks`` chunks each, then twice as many until a
    split's 32-bit byte offsets fit.  At one chunk per split the tap-per-block plans go ahead; the Winograd plans refuse (None)."""
    s = max(1, min(cdiv(target, tiles), cdiv(chunks, min_chunks)))
    while True:
        cps = cdiv(chunks, s)
        if fits(cps) or (cps == 1 and not refuse):
            return cps, cdiv(chunks, cps)
        if cps == 1:
            return None
        s *= 2


def thin_plan(c):
    """rs_wgrad_thin_plan: None, or the all-taps kernel's launch."""
    if c.c2 or c.k != 3 or c.stride != 1 or c.pad != 1 or c.cout % 32 or (c.c1 not in (32, 64) and c.c1 % 128) or c.ho % 8 or c.wo % 8:
        return None
    if c.m * c.cout * 2 >= 1 << 31 or c.n * c.h * c.w * c.c1 * 2 >= 1 << 31:
        return None
    patches = c.n * (c.ho // 8) * (c.wo // 8)
    slab = min(c.c1, 128)
    groups = (c.cout // 32) * (c.c1 // slab)
    if groups == 1:
        nb = min(patches, 512)
    else:
        if c.ups:
            return None
        nb = max(1, 256 // groups)
        if patches // nb < 8:
            return None
    ppb = cdiv(patches, nb)
    nb = cdiv(patches, ppb)
    n = c.cout * 9 * c.c1
    slices = nb * (4 // (slab // 32))
    red = reduce_plan(n, slices)
    return dict(form=1, kind="thin", name="conv_wgrad_thin_bf16<{}{}>".format(slab, ",ups" if c.ups else ""), tile=0, groups=groups,
                patches=patches, chunks=patches, cps=ppb, splits=nb, last=patches - (nb - 1) * ppb, slices=slices, n=n, reduce=red,
                workspace=(slices * n + red["scratch"]) * 4)


def bf16_plan(c, knobs=None):
    """rs_conv2d_wgrad_bf16: the thin kernel where rs_wgrad_thin_plan admits the layer, else plan() of conv_wgrad_bf16.hip."""
    kn = dict(DEFAULT_KNOBS, **(knobs or {}))
    thin = thin_plan(c)
    if thin:
        return thin
    phase = is_decoder(c)
    m = c.n * c.h * c.w if phase else c.m
    bmo, bno, bno2 = largest_tile(c.cout), largest_tile(c.c1), 0
    if c.c2:
        b2 = largest_tile(c.c2)
        if b2 != bno and b2 >= 64 and bno >= 64 and bmo >= 64:
            bno2 = b2  # one launch per source
        elif b2 < bno:
            bno = b2
    if bno == 32:
        bmo = 32
    if bmo == 32 and bno == 64:
        bno = 32
    if not phase and not bno2 and (bmo, bno) == (128, 128) and c.cout % 256 == 0:
        bmo = 256
    taps = 16 if phase else c.k * c.k
    tiles_ci = (c.c1 if bno2 else c.cin) // bno
    tiles_ci2 = c.c2 // bno2 if bno2 else 0
    tiles_co = c.cout // bmo
    phase4 = bool(phase and (bmo, bno) == (128, 128) and kn["wgrad_phase4"])
    tiles = tiles_co * 4 * tiles_ci if phase4 else tiles_co * taps * (tiles_ci + tiles_ci2)
    chunks = cdiv(m, 64)
    target = kn["wgrad_blocks_phase4"] if phase4 else kn["wgrad_blocks_phase"] if phase else kn["wgrad_blocks"]
    howo = c.h * c.w if phase else c.ho * c.wo
    img, dimg = c.h * c.w * max(c.c1, c.c2) * 2, c.ho * c.wo * c.cout * 2

    def fits(cps):
        px = (cps + 2) * 64
        span_dy = (px // howo + 2) * dimg if phase else px * c.cout * 2
        return span_dy < 1 << 31 and (px // howo + 2) * img < 1 << 31

    cps, splits = _split(chunks, tiles, target, 8, fits)
    n = c.cout * taps * c.cin
    red = reduce_plan(n, splits)
    tile = "{}x{}".format(bmo, bno) + ("+{}x{}".format(bmo, bno2) if bno2 else "")
    name = "conv_wgrad_bf16<{}{}>".format(("phase4," if phase4 else "phase,") if phase else "", tile)
    # RING 3 exists for the 64- and 128-wide tap-per-block tiles; the 32-cout tiles and the phase form keep two buffers
    ring = 3 if kn["wgrad_ring"] == 3 and not phase and bmo >= 64 else 2
    return dict(form=2 if phase else 0, kind="src" if phase else "pix", pk=64, name=name, tile=(bmo << 16) | (bno2 << 8) | bno, tile_name=tile,
                chunks=chunks, cps=cps, splits=splits, n=n, reduce=red, ring=3 if phase4 else ring, launches=2 if bno2 else 1,
                workspace=(splits * n + red["scratch"] + (n if phase else 0)) * 4)


def w33_plan(c, kn):
    """w33_plan of conv_wgrad_wino33_f32.hip (geometry only: the knob wgrad_f32_wino33 is applied by f32_plan)."""
    if c.ups or c.k != 3 or c.stride != 1 or c.pad != 1 or c.c2 or c.h < 2 or c.w < 2 or c.cout % 32 or c.c1 % 32:
        return None
    wide = c.cout % 64 == 0 and c.c1 % 64 == 0
    b = 64 if wide else 32
    tiles = (c.cout // b) * (c.c1 // b)
    ty, cx = (c.h + 1) // 2, cdiv((c.w + 1) // 2, 8)
    chunks = c.n * ty * cx
    target = kn["wgrad_f32_wino33_blocks"] * (1 if wide else 3)
    cmax = max(c.c1, c.cout)
    got = _split(chunks, tiles, target, 8, lambda cps: ((cps + 1) // (ty * cx) + 2) * c.h * c.w * cmax * 4 < 1 << 31, refuse=True)
    if got is None:
        return None
    n = 16 * c.cout * c.c1
    red = reduce_plan(n, got[1])
    return dict(kind="w33", ty=ty, cx=cx, chunks=chunks, cps=got[0], splits=got[1], n=n, reduce=red, wide=wide,
                floats=got[1] * n + red["scratch"] + n)


def ww_plan(c, kn):
    """ww_plan of conv_wgrad_wino_f32.hip (geometry only)."""
    if not is_decoder(c) or c.h < 2 or c.w < 2 or c.cout % 32 or c.c1 % 64 or c.c2 % 64:
        return None
    wgm = 2 if c.cout % 64 == 0 else 1
    tiles = 4 * (c.cout // (32 * wgm)) * (c.cin // 64)
    ty, tx = (c.h + 1) // 2, (c.w + 1) // 2
    nt = c.n * ty * tx
    chunks = cdiv(nt, 8)
    cmax = max(c.c1, c.c2)

    def fits(cps):
        imgs = (cps + 1) * 8 // (ty * tx) + 2
        return imgs * 4 * c.h * c.w * c.cout * 4 < 1 << 31 and imgs * c.h * c.w * cmax * 4 < 1 << 31

    got = _split(chunks, tiles, kn["wgrad_f32_wino_blocks"], 16, fits, refuse=True)
    if got is None:
        return None
    n = 36 * c.cout * c.cin
    red = reduce_plan(n, got[1])
    return dict(kind="ww", ty=ty, tx=tx, ntiles=nt, chunks=chunks, cps=got[0], splits=got[1], n=n, reduce=red, wgm=wgm,
                floats=got[1] * n + red["scratch"] + n)


def f32_plan(c, knobs=None):
    """rs_conv2d_wgrad (non-stem): which kernel, its chunks and splits, and the workspace -- the larger of the tap-per-block / phase
    plan's and the Winograd plan's, whichever the knobs pick at launch time."""
    kn = dict(DEFAULT_KNOBS, **(knobs or {}))
    phase = is_decoder(c) and kn["wgrad_f32_phase"] != 0
    dma = kn["wgrad_f32_dma"] != 0
    m = c.n * c.h * c.w if phase else c.m
    bmo, bno = largest_tile(c.cout), largest_tile(c.c1)
    if c.c2:
        bno = min(bno, largest_tile(c.c2))
    if bno == 32:
        bmo = 32
    if bmo == 32 and bno == 64:
        bno = 32
    taps = 16 if phase else c.k * c.k
    tiles = (c.cout // bmo) * taps * (c.cin // bno)
    chunks = cdiv(m, 32)
    howo = c.h * c.w if phase else c.ho * c.wo
    img = c.h * c.w * max(c.c1, c.c2) * 4

    def fits(cps):
        px = (cps + 1) * 32
        span_dy = (px // howo + 2) * c.ho * c.wo * c.cout * 4 if phase else px * c.cout * 4
        return span_dy < 1 << 31 and (px // howo + 2) * img < 1 << 31

    cps, splits = _split(chunks, tiles, kn["wgrad_f32_blocks"], 8, fits)
    n = c.cout * taps * c.cin
    red = reduce_plan(n, splits)
    floats = splits * n + red["scratch"] + (n if phase else 0)
    wino = ww_plan(c, kn) if phase else w33_plan(c, kn)
    workspace = max(floats, wino["floats"] if wino else 0) * 4
    use_wino = bool(wino) and dma and kn["wgrad_f32_wino" if phase else "wgrad_f32_wino33"] != 0
    if use_wino:
        return dict(wino, form=3 if phase else 4, name="conv_wgrad_wino_f32" if phase else "conv_wgrad_wino33_f32", workspace=workspace)
    return dict(form=2 if phase else 0, kind="src" if phase else "pix", pk=32, name="conv_wgrad_f32_dma" if dma else "conv_wgrad_f32",
                tile_name="{}x{}".format(bmo, bno), chunks=chunks, cps=cps, splits=splits, n=n, reduce=red, workspace=workspace)


def plan(case, dtype, knobs=None):
    return (bf16_plan if dtype == "bf16" else f32_plan)(case, knobs)


# ---------------------------------------------------------------------------------------------------------------------------------
# where a plan's chunks and splits lie in the image: the pulse probes' positions
# ---------------------------------------------------------------------------------------------------------------------------------
def _parities(c, pos):
    n, a, b = pos
    return [(n, 2 * a + py, 2 * b + px) for py in (0, 1) for px in (0, 1)]


def chunk_ends(c, pl, chunk):
    """(outputs of the first reduction unit, outputs of the last) of a chunk, as output pixels (n, oy, ox).  A unit is an output
    pixel, or -- for the forms that reduce over SOURCE pixels -- a source pixel with its four output parities."""
    kind = pl["kind"]
    if kind in ("pix", "src"):
        hw = (c.h, c.w) if kind == "src" else (c.ho, c.wo)
        total = c.n * hw[0] * hw[1]
        ends = []
        for m in (chunk * pl["pk"], min(total, (chunk + 1) * pl["pk"]) - 1):
            pos = (m // (hw[0] * hw[1]), m % (hw[0] * hw[1]) // hw[1], m % hw[1])
            ends.append(_parities(c, pos) if kind == "src" else [pos])
        return tuple(ends)
    if kind == "w33":  # eight 2x2 tiles of one tile row
        n, rem = divmod(chunk, pl["ty"] * pl["cx"])
        ty, cx = divmod(rem, pl["cx"])
        return [(n, 2 * ty, 16 * cx)], [(n, min(2 * ty + 1, c.h - 1), min(16 * cx + 15, c.w - 1))]
    if kind == "ww":  # eight 2x2 tiles of source positions
        ends = []
        for t, last in ((chunk * 8, 0), (min(pl["ntiles"], chunk * 8 + 8) - 1, 1)):
            n, rem = divmod(t, pl["ty"] * pl["tx"])
            ty, tx = divmod(rem, pl["tx"])
            ends.append(_parities(c, (n, min(2 * ty + last, c.h - 1), min(2 * tx + last, c.w - 1))))
        return tuple(ends)
    assert kind == "thin"  # an 8x8 patch of output pixels
    ppr, ppi = c.wo // 8, (c.ho // 8) * (c.wo // 8)
    n, rem = divmod(chunk, ppi)
    pr, pc = divmod(rem, ppr)
    return [(n, 8 * pr, 8 * pc)], [(n, 8 * pr + 7, 8 * pc + 7)]


def pulse_positions(c, pl):
    """Output pixels worth a pulse under plan ``pl``, without repeats: corners and an edge midpoint of the first and last image; the
    first and last unit of the first, a middle and the last chunk; both sides of every split boundary; the last pixel of all."""
    out = []
    for n in (0, c.n - 1):
        out += [(n, 0, 0), (n, 0, c.wo - 1), (n, c.ho - 1, 0), (n, c.ho - 1, c.wo - 1), (n, 0, c.wo // 2)]
    for chunk in (0, pl["chunks"] // 2, pl["chunks"] - 1):
        first, last = chunk_ends(c, pl, chunk)
        out += first + last
    for s in range(1, pl["splits"]):
        out += chunk_ends(c, pl, s * pl["cps"] - 1)[1] + chunk_ends(c, pl, s * pl["cps"])[0]
    out.append((c.n - 1, c.ho - 1, c.wo - 1))
    seen, uniq = set(), []
    for p in out:
        assert 0 <= p[0] < c.n and 0 <= p[1] < c.ho and 0 <= p[2] < c.wo, (p, c)
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases.  aim: what the shape was chosen for, as figures of the restated plans at the shipped knobs --
#   bf16 / f32: (kernel name or tile, chunks, chunks per split, splits) of the bf16 launch / of the fp32 tap-per-block (or phase) launch
#   w33 / ww:   (chunks, chunks per split, splits) of the Winograd-domain launch
# ---------------------------------------------------------------------------------------------------------------------------------
def _tile_cases():
    out = []
    for tile, cout, cin in (("256x128", 256, 128), ("128x128", 128, 128), ("128x64", 128, 64), ("64x128", 64, 128), ("64x64", 64, 64),
                            ("32x128", 32, 128), ("32x32", 32, 32)):
        f32 = "128x128" if tile == "256x128" else tile
        # M = 126: two 64-pixel chunks, the second ragged (62); four 32-pixel chunks, the last with 30; wino33: 5 chunks per image, one split each
        out.append((plain("tile_{}_two_chunks".format(tile), 2, 9, 7, cin, cout), dict(bf16=(tile, 2, 2, 1), f32=(f32, 4, 4, 1), w33=(10, 5, 2))))
        # M = 646, images of 323 pixels: bf16 splits at pixel 384, fp32 at 224 and 448 -- all inside an image; ragged tails; wino33: 18 chunks
        # per image in splits of 8 (ceil(36 / 8) = 5 splits, the last of 4)
        out.append((plain("tile_{}_splits".format(tile), 2, 17, 19, cin, cout), dict(bf16=(tile, 11, 6, 2), f32=(f32, 21, 7, 3), w33=(36, 8, 5))))
    return out


TAP_CASES = _tile_cases() + [
    # M around the chunk sizes (64 -> 64 channels keeps the 3x3 off the thin kernel even where Ho, Wo are multiples of 8)
    (plain("m63", 1, 7, 9, 64, 64), dict(bf16=("64x64", 1, 1, 1), f32=("64x64", 2, 2, 1), w33=(4, 4, 1))),       # one ragged chunk
    (plain("m64", 1, 4, 16, 64, 64), dict(bf16=("64x64", 1, 1, 1), f32=("64x64", 2, 2, 1), w33=(2, 2, 1))),     # one whole chunk
    (plain("m65", 1, 5, 13, 64, 64), dict(bf16=("64x64", 2, 2, 1), f32=("64x64", 3, 3, 1), w33=(3, 3, 1))),     # a one-pixel chunk
    (plain("m192", 3, 8, 8, 64, 64), dict(bf16=("64x64", 3, 3, 1), f32=("64x64", 6, 6, 1), w33=(12, 6, 2))),   # image seams on chunk borders
    (plain("m257", 1, 1, 257, 64, 64), dict(bf16=("64x64", 5, 5, 1), f32=("64x64", 9, 5, 2))),                   # one row; a one-pixel chunk
    # more than 8 splits: reduce.hip's two levels, the last split short (3 of 8 chunks; fp32 6 of 8; wino33 8 of 8 but 24 splits)
    (plain("two_level_1x1", 2, 48, 50, 32, 32, k=1), dict(bf16=("32x32", 75, 8, 10), f32=("32x32", 150, 8, 19), L=dict(bf16=5, f32=9))),
    (plain("two_level_3x3", 2, 48, 50, 32, 32), dict(bf16=("32x32", 75, 8, 10), f32=("32x32", 150, 8, 19), w33=(192, 8, 24),
                                                     L=dict(bf16=5, f32=9, w33=12))),
    (plain("s2_3x3_odd", 2, 11, 13, 64, 64, stride=2), dict(bf16=("64x64", 2, 2, 1), f32=("64x64", 3, 3, 1))),  # 6 x 7 outputs of odd inputs
    (plain("s2_1x1", 2, 11, 13, 64, 128, k=1, stride=2), dict(bf16=("128x64", 2, 2, 1), f32=("128x64", 3, 3, 1))),
    (plain("image_2x2", 3, 2, 2, 64, 64), dict(bf16=("64x64", 1, 1, 1), f32=("64x64", 1, 1, 1), w33=(3, 3, 1))),  # smaller than the window
    (plain("image_1x3", 3, 1, 3, 64, 64), dict(bf16=("64x64", 1, 1, 1), f32=("64x64", 1, 1, 1))),
    # two sources without the upsample: the Cin tile walks from src1 into src2
    (plain("two_sources_64+64", 2, 9, 7, 64, 64, c2=64), dict(bf16=("64x64", 2, 2, 1), f32=("64x64", 4, 4, 1))),
    (plain("two_sources_128+64", 2, 9, 7, 128, 128, c2=64), dict(bf16=("128x128+128x64", 2, 2, 1), f32=("128x64", 4, 4, 1))),  # per-source launches, ci_base
    (plain("two_sources_64+32", 2, 9, 7, 64, 64, c2=32), dict(bf16=("32x32", 2, 2, 1), f32=("32x32", 4, 4, 1))),  # a 32-channel source: 32-wide tiles
]

DEC_CASES = [
    # every tile of the phase form on an odd 5 x 7 source grid (M = 70 source pixels: two chunks, the second of 6 pixels; fp32 three)
    (decoder("phase_128x128", 2, 5, 7, 128, 0, 128), dict(bf16=("phase4,128x128", 2, 2, 1), f32=("128x128", 3, 3, 1), ww=(3, 3, 1))),
    (decoder("phase_128x64", 2, 5, 7, 64, 0, 128), dict(bf16=("phase,128x64", 2, 2, 1), f32=("128x64", 3, 3, 1), ww=(3, 3, 1))),
    (decoder("phase_64x128", 2, 5, 7, 128, 0, 64), dict(bf16=("phase,64x128", 2, 2, 1), f32=("64x128", 3, 3, 1), ww=(3, 3, 1))),
    (decoder("phase_64x64", 2, 5, 7, 64, 0, 64), dict(bf16=("phase,64x64", 2, 2, 1), f32=("64x64", 3, 3, 1), ww=(3, 3, 1))),
    (decoder("phase_32x128", 2, 5, 7, 128, 0, 32), dict(bf16=("phase,32x128", 2, 2, 1), f32=("32x128", 3, 3, 1), ww=(3, 3, 1))),
    (decoder("phase_32x32", 2, 5, 7, 32, 0, 32), dict(bf16=("phase,32x32", 2, 2, 1), f32=("32x32", 3, 3, 1))),
    (decoder("phase_64x128+64x64", 2, 5, 7, 128, 64, 64), dict(bf16=("phase,64x128+64x64", 2, 2, 1), f32=("64x64", 3, 3, 1), ww=(3, 3, 1))),
    (decoder("phase_128x128+128x64", 2, 5, 7, 128, 64, 128), dict(bf16=("phase4,128x128+128x64", 2, 2, 1), f32=("128x64", 3, 3, 1), ww=(3, 3, 1))),
    # source grids
    (decoder("grid_1x1", 3, 1, 1, 64, 64, 64), dict(bf16=("phase,64x64", 1, 1, 1), f32=("64x64", 1, 1, 1))),   # every neighbour is padding
    (decoder("grid_2x2", 1, 2, 2, 64, 0, 64), dict(bf16=("phase,64x64", 1, 1, 1), f32=("64x64", 1, 1, 1), ww=(1, 1, 1))),  # one Winograd tile
    (decoder("grid_5x13", 1, 5, 13, 64, 0, 64), dict(bf16=("phase,64x64", 2, 2, 1), f32=("64x64", 3, 3, 1), ww=(3, 3, 1))),  # M = 65: a one-source-pixel chunk
    (decoder("tiles_9", 1, 6, 6, 64, 64, 32), dict(bf16=("phase,32x32", 1, 1, 1), f32=("32x32", 2, 2, 1), ww=(2, 2, 1))),   # 9 tiles: 8 + 1
    (decoder("tiles_15", 1, 6, 10, 64, 0, 64), dict(bf16=("phase,64x64", 1, 1, 1), f32=("64x64", 2, 2, 1), ww=(2, 2, 1))),  # 15 tiles: 8 + 7
    # M = 585 source pixels in images of 195: bf16 splits at source pixel 320 (inside image 1), fp32 at 224 and 448
    (decoder("straddle_64+64", 3, 13, 15, 64, 64, 64), dict(bf16=("phase,64x64", 10, 5, 2), f32=("64x64", 19, 7, 3), ww=(21, 11, 2))),
    (decoder("straddle_128", 3, 13, 15, 128, 0, 128), dict(bf16=("phase4,128x128", 10, 5, 2), f32=("128x128", 19, 7, 3), ww=(21, 11, 2))),
]

# the 3 x 3 source grid of the combine probe (see test_phase_combine_taps)
COMBINE_CASES = [decoder("combine_64", 1, 3, 3, 64, 0, 64), decoder("combine_128", 1, 3, 3, 128, 0, 128)]

THIN_CASES = [
    # name, case, (patches, patches per block, blocks, patches of the last block, slices)
    (plain("thin32_one_patch", 1, 8, 8, 32, 32), (1, 1, 1, 1, 4)),        # every halo side is padding
    (plain("thin64_one_patch", 1, 8, 8, 64, 32), (1, 1, 1, 1, 2)),
    (plain("thin128_one_patch", 1, 8, 8, 128, 32), (1, 1, 1, 1, 1)),
    (decoder("thin32ups_one_patch", 1, 4, 4, 32, 0, 32), (1, 1, 1, 1, 4)),
    (decoder("thin64ups_one_patch", 1, 4, 4, 64, 0, 32), (1, 1, 1, 1, 2)),
    (decoder("thin128ups_one_patch", 1, 4, 4, 128, 0, 32), (1, 1, 1, 1, 1)),
    # 3 x 19 x 9 = 513 patches on 257 blocks: runs of two that cross output rows (9 per row) and images (171 per image), one in the last block
    (plain("thin32_runs", 3, 152, 72, 32, 32), (513, 2, 257, 1, 1028)),
    (plain("thin64_runs", 3, 152, 72, 64, 32), (513, 2, 257, 1, 514)),
    (decoder("thin128ups_runs", 3, 76, 36, 128, 0, 32), (513, 2, 257, 1, 257)),
    (decoder("thin32ups_runs", 3, 76, 36, 32, 0, 32), (513, 2, 257, 1, 1028)),
    # two (cout tile, cin slab) groups: the plan wants 8 patches per block on 256 / 2 blocks -- 1024 patches is the smallest it admits
    (plain("thin32_groups", 1, 256, 256, 32, 64), (1024, 8, 128, 8, 512)),
]
THIN_TOO_SMALL = plain("thin32_groups_1023", 1, 248, 264, 32, 64)  # 31 x 33 = 1023 patches: one fewer, not admitted

THIN_PULSE_CASES = [plain("thin32_pulse", 2, 16, 24, 32, 32), decoder("thin64ups_pulse", 2, 8, 12, 64, 0, 32)]  # 12 patches, one per block


def variants(case, dtype):
    """[(label, knobs)]: the knob settings a case runs under for ``dtype``; the first is the shipped one."""
    if dtype == "bf16":
        pl = bf16_plan(case)
        if pl["form"] == 1:
            return [("thin", {})]
        if pl["form"] == 2:
            return [("phase4", {}), ("phase", {"wgrad_phase4": 0})] if "phase4" in pl["name"] else [("phase", {})]
        return [("ring3", {}), ("ring2", {"wgrad_ring": 2})]
    if is_decoder(case):
        out = [("wino", {})] if f32_plan(case)["form"] == 3 else []
        return out + [("phase", {"wgrad_f32_wino": 0}), ("direct", {"wgrad_f32_phase": 0}), ("staged", {"wgrad_f32_dma": 0})]
    out = [("wino33", {})] if f32_plan(case)["form"] == 4 else []
    return out + [("dma", {"wgrad_f32_wino33": 0}), ("staged", {"wgrad_f32_dma": 0})]


def expected_name(case, dtype, label):
    """The kernel a (case, dtype, variant) aims at, spelled out (not taken from the restatement)."""
    if dtype == "f32":
        return {"wino": "conv_wgrad_wino_f32", "wino33": "conv_wgrad_wino33_f32", "staged": "conv_wgrad_f32"}.get(label, "conv_wgrad_f32_dma")
    for table in (TAP_CASES, DEC_CASES):
        for c, aim in table:
            if c == case:
                tile = aim["bf16"][0]
                return "conv_wgrad_bf16<{}>".format(tile.replace("phase4,", "phase,") if label == "phase" else tile)
    raise KeyError(case)


def all_launches():
    """Every (case, dtype, label, knobs) of the exact tests over TAP_CASES and DEC_CASES."""
    out = []
    for table in (TAP_CASES, DEC_CASES):
        for case, _ in table:
            for dtype in ("bf16", "f32"):
                out += [(case, dtype, label, knobs) for label, knobs in variants(case, dtype)]
    return out


def launch_id(launch):
    return "{}-{}-{}".format(launch[0].name, launch[1], launch[2])


# pulse probes: one case per form and dtype (the variants of each are all run)
PULSE_CASES = [c for c, _ in TAP_CASES if c.name in ("tile_64x64_splits", "s2_3x3_odd", "two_sources_128+64")] + \
              [c for c, _ in DEC_CASES if c.name in ("straddle_64+64", "straddle_128")]

# Gaussian data, one shape per kernel
GAUSS_CASES = [c for c, _ in TAP_CASES if c.name in ("tile_64x64_splits", "tile_256x128_splits", "tile_32x32_splits")] + \
              [c for c, _ in DEC_CASES if c.name in ("straddle_64+64", "straddle_128")] + THIN_PULSE_CASES
