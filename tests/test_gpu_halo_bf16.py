"""The halo-once forms of the bf16 LDS-DMA implicit GEMM (HALO_33, HALO_PHASE, HALO_DG4 in csrc/conv_igemm_dma_kernel.h; the
``halo_mode()`` branch of csrc/conv_igemm_dma.hip) at the places where their main loop and epilogue can go wrong: one patch with every
side on the border, several patches per row and per image, an interior patch, 1 / 2 / 3 / 5 K-groups (both halo buffers, a wrap of the
four-slot weight ring; the single group has no next halo), two concat sources, the four parity planes of the 4x4 / stride-2 data
gradient, N tiles of 64 and 128 with a ragged last one, two destinations, the statistics and the into-BatchNorm epilogues.

Unforced the dispatcher takes these kernels only from ``conv_halo_min`` blocks upward, so every launch here forces them with
``ops.tuning(tile="halo", rowb=64 | 128)`` (the 512-pixel patch of 16 x 32 with 32-channel chunks | the 256-pixel patch of 8 x 32 with
64-channel chunks) and asserts the full name the dispatcher reports against ``expected_name()``, which restates ``halo_mode()``.

Exact checks: x / dz in [-2, 2], 3x3 weights in [-1, 1] (the phase and 4x4 packs sum at most four of them: integers of magnitude <= 4,
exact in bf16), scale in [1, 3], shift in [-4, 4], residual in [-9, 9], mask in [-1, 1].  Every partial sum is an integer bounded by
sum |x||w| < 2^24 (asserted per problem), so the fp32 accumulators are exact in any order, and the device result must be ``torch.equal``
to the float64 host convolution of the UNPACKED 3x3 weights + the epilogue, rounded once to bf16 (round to nearest even on both sides).
One Gaussian check per form and patch size against float64 with a derived per-element bound, and image 0 alone against image 0 of a
batch of three, bit for bit."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
EXACT = float(1 << 24)


def ints(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F64)


def nhwc(t, dtype=BF):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).to(dtype)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu().to(F64)


def krsc_f32(w):
    return w.permute(0, 2, 3, 1).contiguous().to(DEV).float()


def v(t):
    return t.view(1, -1, 1, 1)


def cdiv(a, b):
    return -(-a // b)


def n_tile(cout):
    """The N tile of ``halo_mode()``: 128 where the tiles are whole or at most 1/5 of a ragged tiling is padding, else 64, else none."""
    if cout % 128 == 0 or (cout > 128 and cdiv(cout, 128) * 128 * 4 <= cout * 5):
        return 128
    return 64 if cout % 64 == 0 else 0


def expected_name(form, rowb, n, gh, gw, c1, c2, cout):
    """What the dispatcher reports under ``tuning(tile="halo", rowb=rowb)``: the rules of ``halo_mode()`` restated.  The 512-pixel patch
    needs the N tile of 128 and a grid height that is a multiple of 16; where it cannot run, or with rowb = 128, the 256-pixel patch runs if
    both sources are multiples of 64 channels; else the dispatcher's own implicit-GEMM tile (these grids are far below its 512 blocks)."""
    bn = n_tile(cout)
    big = rowb == 64 and bn == 128 and gh % 16 == 0
    c64 = c1 % 64 == 0 and c2 % 64 == 0
    if bn and (big or c64) and gh % (16 if big else 8) == 0 and gw % 32 == 0 and not (form == "dgrad4x4" and c2):
        return "conv_halo_bf16<{},{}x{}>".format(form, 512 if big else 256, bn)
    m = n * gh * gw * (4 if form == "phase" else 1)
    assert cdiv(m, 128) * cdiv(cout, 64) < 512 and cout % 256 != 0, "a grid this large is the heuristics' business, not this file's"
    return "conv_igemm_bf16<{}{},r{}>".format("phase," if form == "phase" else "", "64x64" if cout % 64 == 0 else "128x32", 128 if rowb == 128 and c64 else 64)


def conv_ref(form, x, wt, gh, gw):
    """float64 host reference from the unpacked OIHW 3x3 weights.  3x3: x [n, c, gh, gw]; phase: x on the source grid; dgrad4x4: x = dz
    [n, c, 2gh, 2gw] and ``wt`` [c, cout, 3, 3] the FORWARD weights -- the autograd gradient of the phase-form expression wrt its input."""
    if form == "3x3":
        return F.conv2d(x, wt, padding=1)
    if form == "phase":
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, padding=1)
    a = torch.zeros(x.shape[0], wt.shape[1], gh, gw, dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(F.interpolate(a, scale_factor=2, mode="nearest"), wt, padding=1), a, x)
    return g


def operands(form, x, wt, c1, unit=1.0, wmax=1.0):
    """Device operands of one launch: sources (NHWC bf16, split at c1) and the weights in the layout the form takes."""
    from robosat_amd import ops

    xd = nhwc(x)
    s1, s2 = (xd, None) if c1 == x.shape[1] else (xd[..., :c1].contiguous(), xd[..., c1:].contiguous())
    wk = krsc_f32(wt)
    wd = wk.to(BF) if form == "3x3" else (ops.pack_phase_weight(wk, BF) if form == "phase" else ops.pack_dgrad_phase_weight(wk, BF))
    if form != "3x3":  # the packs sum at most four taps: multiples of `unit` up to 4 wmax, within bf16's 8 significant bits
        assert 4 * wmax / unit <= 256 and float(wd.float().abs().max()) <= 4 * wmax and torch.equal(wd.float() / unit, (wd.float() / unit).round())
    return s1, s2, wd


def launch(form, s1, s2, wd, gh, gw, **opts):
    from robosat_amd import ops

    if form == "3x3":
        return ops.conv2d(s1, wd, src2=s2, pad=1, **opts)
    if form == "phase":
        return ops.conv2d_phase(s1, wd, src2=s2, **opts)
    assert s2 is None
    return ops.conv2d(s1, wd, stride=2, pad=1, out_hw=(gh, gw), **opts)


def reported_name(form, s1, s2, wd, gh, gw, cout):
    from robosat_amd import _lib, ops

    if form == "3x3":
        d = ops.conv_desc(s1, wd, s2, 0, 1, 1)
    elif form == "phase":
        d = _lib.ConvDesc(s1.shape[0], gh, gw, s1.shape[3], 0 if s2 is None else s2.shape[3], 1, 3, 3, 1, 1, 2 * gh, 2 * gw, cout, 0, 0)
    else:
        d = ops.conv_desc(s1, wd, stride=2, pad=1, out_hw=(gh, gw))
    return ops.conv_tile_name(d, True, phase=form == "phase")


@functools.lru_cache(maxsize=None)
def problem(form, n, gh, gw, c1, c2, cout, xmax=2):
    """Integer operands (host, NCHW / OIHW, float64) and the raw convolution, shared by every kind and test; left unchanged."""
    c = c1 + c2
    seed = 100000 * ("3x3", "phase", "dgrad4x4").index(form) + 1000 * c + 10 * cout + n + 7 * gh + gw + xmax
    up = 2 if form == "dgrad4x4" else 1
    x = ints(-xmax, xmax, n, c, up * gh, up * gw, seed=seed)
    wt = ints(-1, 1, c, cout, 3, 3, seed=seed + 1) if form == "dgrad4x4" else ints(-1, 1, cout, c, 3, 3, seed=seed + 1)
    base = conv_ref(form, x, wt, gh, gw)
    sc, sh = ints(1, 3, cout, seed=seed + 2), ints(-4, 4, cout, seed=seed + 3)
    res, mask = ints(-9, 9, *base.shape, seed=seed + 4), ints(-1, 1, *base.shape, seed=seed + 5)
    # precondition: a result sums <= 9 c products of the unpacked taps (dgrad4x4: 36 c, nine taps at each of four upsampled pixels), each
    # <= xmax * 1, so every partial sum, in whatever order and however the packs group the taps, and every epilogue value is an integer
    # below 2^24: exact in fp32
    terms = (36 if form == "dgrad4x4" else 9) * c
    assert float(base.abs().max()) <= terms * xmax and terms * xmax * 3.0 + 4.0 + 9.0 < EXACT
    assert float((base.abs() < 256).double().mean()) > 0.9  # most results exact in bf16 themselves: an error of one is seen
    return x, wt, base, sc, sh, res, mask


def bf16_round(t):
    return t.to(BF).to(F64)


def kinds(base, sc, sh, res, mask):
    """(name, launch options without the device tensors, float64 expectation): the table of ``run_kinds()`` in the fp32 file."""
    zero = torch.zeros((), dtype=F64)
    return [
        ("none", (), base),
        ("scale+shift", ("scale", "shift"), base * v(sc) + v(sh)),
        ("scale+shift+relu", ("scale", "shift", "relu"), F.relu(base * v(sc) + v(sh))),
        ("scale+shift+res+relu", ("scale", "shift", "residual", "relu"), F.relu(base * v(sc) + v(sh) + res)),
        ("res", ("residual",), base + res),
        ("mask", ("relu_mask",), torch.where(mask > 0, base, zero)),
        ("res+mask", ("residual", "relu_mask"), torch.where(mask > 0, base + res, zero)),
    ]


# (rowb, n, gh, gw, c1, c2, cout); the grid is the output grid (phase: the source grid; dgrad4x4: dz is twice as large).  Large channel
# counts go with small grids and the other way round.
CASES_33_PHASE = [
    # 512-pixel patch: 32-channel chunks
    (64, 1, 16, 32, 32, 0, 128),     # one patch, every side on the border, ONE K-group: no next halo (phase: 4 steps = the 4 ring slots)
    (64, 3, 16, 32, 64, 0, 256),     # two groups, two N tiles, the descriptors restart per image
    (64, 1, 16, 64, 96, 0, 224),     # three groups, two patches per grid row, ragged last N tile of 96
    (64, 1, 16, 32, 160, 0, 320),    # five groups: both halo buffers twice, the weight ring wraps; ragged last N tile of 64
    (64, 1, 48, 96, 32, 32, 128),    # 3 x 3 patches: an interior one; two sources of one chunk each
    (64, 3, 16, 64, 64, 32, 128),    # two sources, the second no multiple of 64
    (64, 1, 16, 32, 64, 64, 256),
    (64, 3, 16, 32, 128, 64, 128),   # six groups over two sources
    # ... that cannot run: the 256-pixel patch where the sources are multiples of 64, else the generic tile
    (64, 1, 16, 32, 64, 0, 64),      # N tile of 64
    (64, 1, 16, 32, 128, 0, 192),    # N tile of 64, three of them
    (64, 3, 8, 32, 64, 0, 128),      # grid height 8
    (64, 1, 16, 32, 96, 0, 192),     # N tile of 64 and 96 channels: generic
    (64, 1, 8, 32, 32, 0, 128),      # grid height 8 and 32 channels: generic
    # 256-pixel patch: 64-channel chunks
    (128, 1, 8, 32, 64, 0, 64),      # one patch, every side on the border, ONE K-group, N tile of 64
    (128, 3, 8, 32, 128, 0, 192),    # two groups, three N tiles of 64
    (128, 1, 16, 32, 192, 0, 128),   # three groups, two patches per image
    (128, 1, 8, 32, 320, 0, 320),    # five groups, ragged last N tile of 64
    (128, 1, 32, 96, 64, 64, 128),   # 4 x 3 patches: interior ones; two sources
    (128, 3, 16, 64, 128, 64, 64),   # more than one patch per grid row, two sources
    (128, 1, 16, 32, 64, 0, 224),    # ragged last N tile of 96
    (128, 1, 16, 64, 64, 0, 256),
    (128, 1, 8, 32, 96, 0, 128),     # 96 channels: generic
]
CASES_DG4 = [  # one source; K-groups = 4 parity planes x chunks: 1 and 3 chunks per plane
    (64, 1, 16, 32, 32, 0, 128),
    (64, 3, 16, 64, 96, 0, 256),
    (64, 1, 48, 96, 32, 0, 224),
    (64, 3, 16, 32, 96, 0, 320),
    (64, 1, 16, 32, 64, 0, 192),     # N tile of 64: the 256-pixel patch
    (64, 1, 16, 32, 32, 0, 64),      # N tile of 64 and 32 channels: generic
    (64, 3, 8, 32, 64, 0, 128),      # grid height 8: the 256-pixel patch
    (128, 1, 8, 32, 64, 0, 64),
    (128, 3, 8, 32, 192, 0, 192),
    (128, 1, 16, 32, 64, 0, 128),
    (128, 1, 32, 96, 64, 0, 128),
    (128, 3, 16, 64, 64, 0, 256),
    (128, 1, 16, 64, 192, 0, 320),
    (128, 1, 8, 32, 64, 0, 224),
]
CASES = [("3x3",) + c for c in CASES_33_PHASE] + [("phase",) + c for c in CASES_33_PHASE] + [("dgrad4x4",) + c for c in CASES_DG4]


def case_id(c):
    return "{}-r{}-n{}-{}x{}-c{}+{}-k{}".format(*c)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_epilogue_kind_is_exact(case):
    from robosat_amd import ops

    form, rowb, n, gh, gw, c1, c2, cout = case
    x, wt, base, sc, sh, res, mask = problem(form, n, gh, gw, c1, c2, cout)
    s1, s2, wd = operands(form, x, wt, c1)
    dev = dict(scale=sc.float().to(DEV), shift=sh.float().to(DEV), residual=nhwc(res), relu_mask=nhwc(mask), relu=True)
    want_name = expected_name(form, rowb, n, gh, gw, c1, c2, cout)
    for what, keys, want in kinds(base, sc, sh, res, mask):
        assert float(want.abs().max()) < EXACT
        with ops.tuning(tile="halo", rowb=rowb):
            name = reported_name(form, s1, s2, wd, gh, gw, cout)
            assert name == want_name, (name, want_name)
            got = launch(form, s1, s2, wd, gh, gw, **{k: dev[k] for k in keys})
            torch.cuda.synchronize()
        assert torch.equal(nchw(got), bf16_round(want)), "{} {}: {} elements differ".format(what, name, int((nchw(got) != bf16_round(want)).sum()))


SPLITS = [  # (form, rowb, n, gh, gw, c, cout, csplit): csplit a multiple of the N tile
    ("3x3", 64, 1, 16, 64, 32, 256, 128),
    ("3x3", 128, 1, 16, 32, 64, 256, 128),
    ("3x3", 128, 3, 8, 32, 64, 192, 64),
    ("3x3", 128, 3, 8, 32, 64, 192, 128),
    ("dgrad4x4", 64, 1, 16, 64, 32, 256, 128),
    ("dgrad4x4", 128, 1, 16, 32, 64, 256, 128),
    ("dgrad4x4", 128, 3, 8, 32, 64, 192, 64),
    ("dgrad4x4", 128, 3, 8, 32, 64, 192, 128),
]


@pytest.mark.parametrize("case", SPLITS, ids=lambda c: "{}-r{}-n{}-{}x{}-c{}-k{}-s{}".format(*c))
def test_two_destinations_with_a_mask_on_one_side(case):
    from robosat_amd import ops

    form, rowb, n, gh, gw, c, cout, cs = case
    x, wt, base, _, _, _, mask = problem(form, n, gh, gw, c, 0, cout)
    s1, _, wd = operands(form, x, wt, c)
    kw = dict(pad=1) if form == "3x3" else dict(stride=2, pad=1, out_hw=(gh, gw))
    m1, m2 = mask[:, :cs].contiguous(), mask[:, cs:].contiguous()
    zero = torch.zeros((), dtype=F64)
    for side in (1, 2):
        with ops.tuning(tile="halo", rowb=rowb):
            name = reported_name(form, s1, None, wd, gh, gw, cout)
            assert name == expected_name(form, rowb, n, gh, gw, c, 0, cout) and name.startswith("conv_halo") and cs % n_tile(cout) == 0
            o1, o2 = ops.conv2d_split(s1, wd, cs, mask1=nhwc(m1) if side == 1 else None, mask2=nhwc(m2) if side == 2 else None, **kw)
            torch.cuda.synchronize()
        w1 = torch.where(m1 > 0, base[:, :cs], zero) if side == 1 else base[:, :cs]
        w2 = torch.where(m2 > 0, base[:, cs:], zero) if side == 2 else base[:, cs:]
        assert torch.equal(nchw(o1), bf16_round(w1)), "out1, mask on side {}".format(side)
        assert torch.equal(nchw(o2), bf16_round(w2)), "out2, mask on side {}".format(side)


def patch_sums(t, ph):
    """[n, c, h, w] -> [patches, c]: sums over the ph x 32 patches in the kernel's order -- M tile mt = (image, patch row, patch column),
    as the kernel decodes it (hn = mt / tpi, ty = rem / tpx)."""
    n, c, h, w = t.shape
    return t.reshape(n, c, h // ph, ph, w // 32, 32).sum((3, 5)).permute(0, 2, 3, 1).reshape(-1, c)


STATS = [  # (rowb, n, h, w, c1, c2, cout)
    (64, 3, 16, 64, 64, 0, 128),
    (64, 1, 48, 96, 32, 32, 224),
    (128, 3, 16, 64, 64, 64, 192),
    (128, 1, 8, 32, 320, 0, 320),
    (64, 1, 16, 32, 64, 0, 64),      # the forced 512-pixel patch gives way to the 256-pixel one: two rows
]


@pytest.mark.parametrize("case", STATS, ids=lambda c: "r{}-n{}-{}x{}-c{}+{}-k{}".format(*c))
def test_statistics_epilogue_rows_are_exact(case):
    """``conv2d_bnstats`` on HALO_33: the raw output, and one partial row per patch = sum y, sum y^2 over the bf16 values AS STORED."""
    from robosat_amd import ops

    rowb, n, h, w, c1, c2, cout = case
    x, wt, base, _, _, _, _ = problem("3x3", n, h, w, c1, c2, cout, xmax=1)
    s1, s2, wd = operands("3x3", x, wt, c1)
    name = expected_name("3x3", rowb, n, h, w, c1, c2, cout)
    ph = 16 if ",512x" in name else 8
    yb = bf16_round(base)
    s0, s1_ = patch_sums(yb, ph), patch_sums(yb * yb, ph)
    assert float(s1_.max()) < EXACT  # every term a non-negative integer: the sums are exact in any order
    with ops.tuning(tile="halo", rowb=rowb):
        assert reported_name("3x3", s1, s2, wd, h, w, cout) == name and name.startswith("conv_halo")
        y, partial = ops.conv2d_bnstats(s1, wd, src2=s2, pad=1)
        torch.cuda.synchronize()
    assert partial.shape[0] == n * (h // ph) * (w // 32)  # one row per patch: the generic tiles count 128 or 64 pixels a row
    assert torch.equal(nchw(y), yb)
    p = partial.cpu().to(F64)
    assert torch.equal(p[:, 0], s0), "sum y: rows {}".format((p[:, 0] != s0).any(1).nonzero().flatten().tolist())
    assert torch.equal(p[:, 1], s1_), "sum y^2: rows {}".format((p[:, 1] != s1_).any(1).nonzero().flatten().tolist())


BWD = [  # (rowb, n, h, w, c = channels of dy, cout = channels of the gradient)
    (64, 1, 32, 64, 32, 128),
    (128, 3, 16, 32, 64, 128),
    (128, 1, 8, 32, 128, 64),
    (64, 3, 16, 32, 96, 224),
]


@pytest.mark.parametrize("case", BWD, ids=lambda c: "r{}-n{}-{}x{}-c{}-k{}".format(*c))
def test_into_batchnorm_epilogue_is_exact(case):
    """``conv2d_dgrad_bnstats`` on HALO_33 (the data gradient of a 3x3 convolution, weights from ``pack_dgrad_weight``) with a ReLU mask, the
    same mask as bits, and a residual: g, and per patch sum g and sum g (y - mean) invstd over g as stored.  y and mean are small integers
    and invstd a power of two, so every term is a multiple of 1/2 and the sums are exact below 2^23."""
    from robosat_amd import ops

    rowb, n, h, w, c, cout = case
    seed = 7000 + 10 * c + cout + n
    dy, wt = ints(-2, 2, n, c, h, w, seed=seed), ints(-1, 1, c, cout, 3, 3, seed=seed + 1)  # wt: the forward weights, OIHW
    x0 = torch.zeros(n, cout, h, w, dtype=F64, requires_grad=True)
    (base,) = torch.autograd.grad(F.conv2d(x0, wt, padding=1), x0, dy)
    assert 9 * c * 2 * 1.0 + 9.0 < EXACT and float(base.abs().max()) <= 9 * c * 2
    res, mask = ints(-9, 9, *base.shape, seed=seed + 2), ints(-1, 1, *base.shape, seed=seed + 3)
    bn_y, mean = ints(-4, 4, *base.shape, seed=seed + 4), ints(-2, 2, cout, seed=seed + 5)
    invstd = 2.0 ** ints(-1, 1, cout, seed=seed + 6)
    xhat = (bn_y - v(mean)) * v(invstd)
    dyd, wd = nhwc(dy), ops.pack_dgrad_weight(krsc_f32(wt), BF)
    z = nhwc(mask)
    bits = ((z.reshape(-1, 8) > 0).to(torch.int32) << torch.arange(8, device=DEV, dtype=torch.int32)).sum(1).to(torch.uint8)  # as test_relu_mask_as_bits
    name = expected_name("3x3", rowb, n, h, w, c, 0, cout)
    ph = 16 if ",512x" in name else 8
    masked = torch.where(mask > 0, base, torch.zeros((), dtype=F64))
    for what, opts, want in (("mask", dict(relu_mask=z), masked), ("bits", dict(relu_mask_bits=bits), masked), ("residual", dict(residual=nhwc(res)), base + res)):
        gb = bf16_round(want)
        assert float(patch_sums((gb * xhat).abs(), ph).max()) < EXACT / 2 and float(patch_sums(gb.abs(), ph).max()) < EXACT
        with ops.tuning(tile="halo", rowb=rowb):
            assert reported_name("3x3", dyd, None, wd, h, w, cout) == name and name.startswith("conv_halo")
            g, partial = ops.conv2d_dgrad_bnstats(dyd, wd, (h, w), nhwc(bn_y), mean.float().to(DEV), invstd.float().to(DEV), pad=1, **opts)
            torch.cuda.synchronize()
        assert partial.shape[0] == n * (h // ph) * (w // 32)
        assert torch.equal(nchw(g), gb), what
        p = partial.cpu().to(F64)
        assert torch.equal(p[:, 0], patch_sums(gb, ph)), "{}: sum g".format(what)
        assert torch.equal(p[:, 1], patch_sums(gb * xhat, ph)), "{}: sum g xhat".format(what)


RANDOM = [  # (form, rowb, gh, gw, c1, c2, cout), n = 3
    ("3x3", 64, 16, 32, 64, 32, 128),
    ("3x3", 128, 16, 32, 64, 64, 192),
    ("phase", 64, 16, 32, 64, 32, 128),
    ("phase", 128, 8, 32, 128, 64, 64),
    ("dgrad4x4", 64, 16, 32, 96, 0, 128),
    ("dgrad4x4", 128, 8, 32, 192, 0, 320),
]


@pytest.mark.parametrize("case", RANDOM, ids=lambda c: "{}-r{}-{}x{}-c{}+{}-k{}".format(*c))
def test_gaussian_operands_against_float64_and_across_batch_sizes(case):
    """Gaussian operands rounded to bf16, scale + shift + residual + ReLU, against float64: per element
    |got - want| <= 2^-8 |want| + 2 K 2^-24 scale (|x| conv |w|) + 2 * 2 * 2^-24 (scale (|x| conv |w|) + |shift| + |residual|) -- twice the
    half-ulp of the one bf16 rounding, plus twice the textbook bound of K fp32 additions (K = the products the kernel sums: 9 c, phase 4 c,
    dgrad4x4 16 c) on the convolution of absolute values, scaled as the epilogue scales it, plus the same for the two fp32 operations of the
    epilogue on their operands.  Derived, not measured.  The 3x3 weights are
    multiples of 1/8 below 3 in magnitude, so that the phase and 4x4 packs (sums of up to four) are exact in bf16 and the reference is the
    unpacked expression.  And image 0 alone equals image 0 inside the batch of three, bit for bit."""
    from robosat_amd import ops

    form, rowb, gh, gw, c1, c2, cout = case
    n, c = 3, c1 + c2
    g = torch.Generator().manual_seed(11 + c + cout)
    up = 2 if form == "dgrad4x4" else 1
    x = torch.randn(n, c, up * gh, up * gw, generator=g).to(BF).to(F64)
    wt = ((torch.randn(*((c, cout) if form == "dgrad4x4" else (cout, c)), 3, 3, generator=g) * 8).round() / 8).clamp(-3, 3).to(F64)
    sc, sh = (torch.rand(cout, generator=g) + 0.5).to(F64), torch.randn(cout, generator=g).to(F64)
    conv, absconv = conv_ref(form, x, wt, gh, gw), conv_ref(form, x.abs(), wt.abs(), gh, gw)
    res = torch.randn(*conv.shape, generator=g).to(BF).to(F64)
    want = F.relu(conv * v(sc) + v(sh) + res)
    k = {"3x3": 9, "phase": 4, "dgrad4x4": 16}[form] * c
    bound = 2.0 ** -8 * want.abs() + 2 * k * 2.0 ** -24 * absconv * v(sc) + 2 * 2 * 2.0 ** -24 * (absconv * v(sc) + v(sh).abs() + res.abs())
    s1, s2, wd = operands(form, x, wt, c1, unit=0.125, wmax=3.0)
    opts = dict(scale=sc.float().to(DEV), shift=sh.float().to(DEV), relu=True)
    resd = nhwc(res)
    with ops.tuning(tile="halo", rowb=rowb):
        name = reported_name(form, s1, s2, wd, gh, gw, cout)
        assert name == expected_name(form, rowb, n, gh, gw, c1, c2, cout) and name.startswith("conv_halo")
        got = launch(form, s1, s2, wd, gh, gw, residual=resd, **opts)
        one = launch(form, s1[:1].contiguous(), None if s2 is None else s2[:1].contiguous(), wd, gh, gw, residual=resd[:1].contiguous(), **opts)
        torch.cuda.synchronize()
    ratio = float(((nchw(got) - want).abs() / bound).max())
    print("{} r{}: largest error / bound = {:.4f}".format(name, rowb, ratio))
    assert ratio <= 1.0, ratio
    assert torch.equal(one[0], got[0]), "image 0 depends on the batch it travels in"
