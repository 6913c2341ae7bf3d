"""``conv_thin_bf16`` (csrc/conv_thin_bf16.hip: 3x3 32 -> 32, phase form 128 -> 32, 4x4 / stride-2 data gradient 32 -> 128) where a
persistent block's patch walk can go wrong: ragged last patch rows and columns, one patch with every side padding, an interior patch, the
descriptors across images -- and the ring: the kernel takes at most 256 blocks, each walks its patches through three halo slots and stages
its output in the slot it has just consumed, so only past 768 patches does a block reuse a slot that held staged output.  The kernel is
reached unforced (the name is asserted).

Exact checks as in test_gpu_halo_bf16.py: x / dz in [-2, 2], 3x3 weights in [-1, 1] (the packs sum at most four: exact in bf16), mask in
[-1, 1]; every partial sum is an integer bounded by sum |x||w| < 2^24 (asserted), so the device result must be ``torch.equal`` to the
float64 host convolution of the unpacked 3x3 weights + ReLU / ReLU mask, rounded once to bf16.  The phase kernel has no ReLU-mask input:
the dispatcher must hand a phase launch WITH a mask to the generic kernel, and the name and the exact result say so."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
EXACT = float(1 << 24)
MODES = ["3x3", "phase", "dgrad4x4"]
PATCH = {"3x3": (16, 32), "phase": (8, 16), "dgrad4x4": (8, 16)}   # on the base grid: output | source | output grid
CHANNELS = {"3x3": (32, 32), "phase": (128, 32), "dgrad4x4": (32, 128)}  # (in, out) of the launch
PHASE_MASK_NAME = "conv_igemm_bf16<phase,128x32,r128>"  # 32 couts: the 128x32 tile; four taps x 128 channels = 8 rows of 128 bytes


def ints(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).to(F64)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).to(BF)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu().to(F64)


def cdiv(a, b):
    return -(-a // b)


def patches(mode, n, bh, bw):
    return n * cdiv(bh, PATCH[mode][0]) * cdiv(bw, PATCH[mode][1])


def conv_ref(mode, x, wt, bh, bw):
    """float64 host reference from the unpacked OIHW 3x3 weights; dgrad4x4: x = dz [n, 32, 2bh, 2bw], ``wt`` [32, 128, 3, 3] the FORWARD
    weights -- the autograd gradient of the phase-form expression with respect to its input."""
    if mode == "3x3":
        return F.conv2d(x, wt, padding=1)
    if mode == "phase":
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, padding=1)
    a = torch.zeros(x.shape[0], wt.shape[1], bh, bw, dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(F.interpolate(a, scale_factor=2, mode="nearest"), wt, padding=1), a, x)
    return g


def problem(mode, n, bh, bw):
    """Integer operands (host, float64) and the raw convolution, shared by every kind of one case; left unchanged."""
    cin, cout = CHANNELS[mode]
    seed = 50000 * MODES.index(mode) + 1000 * n + 10 * bh + bw
    up = 2 if mode == "dgrad4x4" else 1
    x = ints(-2, 2, n, cin, up * bh, up * bw, seed=seed)
    wt = ints(-1, 1, *((cin, cout) if mode == "dgrad4x4" else (cout, cin)), 3, 3, seed=seed + 1)
    base = conv_ref(mode, x, wt, bh, bw)
    mask = ints(-1, 1, *base.shape, seed=seed + 2)
    # precondition: a result sums <= 9 cin products of the unpacked taps (dgrad4x4: 36 cin, nine taps at each of four upsampled pixels),
    # each <= 2: every partial sum, however the packs group the taps, is an integer below 2^24 and exact in fp32
    terms = (36 if mode == "dgrad4x4" else 9) * cin
    assert float(base.abs().max()) <= 2 * terms and 2.0 * terms < EXACT
    assert float((base.abs() < 256).double().mean()) > 0.9  # most results exact in bf16 themselves: an error of one is seen
    return x, wt, base, mask


def operands(mode, x, wt, unit=1.0, wmax=1.0):
    from robosat_amd import ops

    wk = wt.permute(0, 2, 3, 1).contiguous().to(DEV).float()
    wd = wk.to(BF) if mode == "3x3" else (ops.pack_phase_weight(wk, BF) if mode == "phase" else ops.pack_dgrad_phase_weight(wk, BF))
    if mode != "3x3":  # the packs sum at most four taps: multiples of `unit` up to 4 wmax, within bf16's 8 significant bits
        assert 4 * wmax / unit <= 256 and float(wd.float().abs().max()) <= 4 * wmax and torch.equal(wd.float() / unit, (wd.float() / unit).round())
    return nhwc(x), wd


def launch(mode, xd, wd, bh, bw, **opts):
    from robosat_amd import ops

    if mode == "3x3":
        return ops.conv2d(xd, wd, pad=1, **opts)
    if mode == "phase":
        return ops.conv2d_phase(xd, wd, **opts)
    return ops.conv2d(xd, wd, stride=2, pad=1, out_hw=(bh, bw), **opts)


def reported_name(mode, xd, wd, bh, bw, masked):
    from robosat_amd import _lib, ops

    if mode == "3x3":
        d = ops.conv_desc(xd, wd, pad=1)
    elif mode == "phase":
        d = _lib.ConvDesc(xd.shape[0], bh, bw, 128, 0, 1, 3, 3, 1, 1, 2 * bh, 2 * bw, 32, 0, 0)
    else:
        d = ops.conv_desc(xd, wd, stride=2, pad=1, out_hw=(bh, bw))
    return ops.conv_tile_name(d, True, phase=mode == "phase", plain=not masked)


def run_kinds(mode, n, bh, bw):
    """none, ReLU, ReLU mask: each ``torch.equal`` to the host, each launch with its kernel's name asserted."""
    x, wt, base, mask = problem(mode, n, bh, bw)
    xd, wd = operands(mode, x, wt)
    zero = torch.zeros((), dtype=F64)
    for what, opts, want in (("none", {}, base), ("relu", dict(relu=True), F.relu(base)), ("mask", dict(relu_mask=nhwc(mask)), torch.where(mask > 0, base, zero))):
        name = reported_name(mode, xd, wd, bh, bw, what == "mask")
        if mode == "phase" and what == "mask":  # (the thin phase kernel takes no mask: the generic kernel)
            assert name == PHASE_MASK_NAME, name
        else:
            assert name == "conv_thin_bf16<{}>".format(mode), name
        got = launch(mode, xd, wd, bh, bw, **opts)
        torch.cuda.synchronize()
        want = want.to(BF).to(F64)
        assert torch.equal(nchw(got), want), "{} {} n{} {}x{}: {} elements differ".format(what, name, n, bh, bw, int((nchw(got) != want).sum()))


# base grids (output grid; phase: source grid; dz of dgrad4x4 is twice as large) -> patches, the ragged part
GRIDS = {
    "3x3": [(17, 33),    # 2 x 2 patches: the last row and column of patches hold 1 row / 1 pixel
            (16, 32),    # one patch: every side is padding
            (40, 70)],   # 3 x 3 patches: an interior one; W no multiple of 8
    "phase": [(9, 17), (8, 16), (20, 35)],
    "dgrad4x4": [(9, 17), (8, 16), (20, 35)],
}
EDGES = [(mode, n, bh, bw) for mode in MODES for (bh, bw) in GRIDS[mode] for n in (1, 3)]


@pytest.mark.parametrize("mode,n,bh,bw", EDGES)
def test_ragged_edges_and_a_few_patches_are_exact(mode, n, bh, bw):
    assert patches(mode, n, bh, bw) == n * {0: 4, 1: 1, 2: 9}[GRIDS[mode].index((bh, bw))]
    run_kinds(mode, n, bh, bw)


RING = {"3x3": (7, 170, 310), "phase": (7, 85, 155), "dgrad4x4": (7, 85, 155)}  # 11 x 10 patches x 7 images = 770


@pytest.mark.parametrize("mode", MODES)
def test_the_ring_turns_and_reuses_a_staged_slot(mode):
    """More than 3 x 256 patches: the first blocks walk four, so their fourth halo lands in the slot that held the first patch's staged
    output (and, with a mask, its mask patch was fetched four times into the one mask buffer)."""
    n, bh, bw = RING[mode]
    assert patches(mode, n, bh, bw) > 768
    run_kinds(mode, n, bh, bw)


@pytest.mark.parametrize("mode", MODES)
def test_gaussian_operands_against_float64_and_across_batch_sizes(mode):
    """Gaussian operands rounded to bf16, ReLU, against float64: per element |got - want| <= 2^-8 |want| + 2 K 2^-24 (|x| conv |w|) -- twice
    the half-ulp of the one bf16 rounding plus twice the textbook bound of K fp32 additions (K = the products the kernel sums: 9 x 32,
    4 x 128, 16 x 32) on the convolution of absolute values.  Derived, not measured.  The 3x3 weights are multiples of 1/8 below 3 in
    magnitude, so that the packs (sums of up to four) are exact in bf16 and the reference is the unpacked expression.  And image 0 alone
    equals image 0 inside the batch of three, bit for bit (2 x 2 ragged patches per image: 4 against 12 blocks)."""
    n, (bh, bw) = 3, GRIDS[mode][0]
    cin, cout = CHANNELS[mode]
    g = torch.Generator().manual_seed(3 + MODES.index(mode))
    up = 2 if mode == "dgrad4x4" else 1
    x = torch.randn(n, cin, up * bh, up * bw, generator=g).to(BF).to(F64)
    wt = ((torch.randn(*((cin, cout) if mode == "dgrad4x4" else (cout, cin)), 3, 3, generator=g) * 8).round() / 8).clamp(-3, 3).to(F64)
    want, absconv = F.relu(conv_ref(mode, x, wt, bh, bw)), conv_ref(mode, x.abs(), wt.abs(), bh, bw)
    k = {"3x3": 9, "phase": 4, "dgrad4x4": 16}[mode] * cin
    bound = 2.0 ** -8 * want.abs() + 2 * k * 2.0 ** -24 * absconv
    xd, wd = operands(mode, x, wt, unit=0.125, wmax=3.0)
    name = reported_name(mode, xd, wd, bh, bw, False)
    assert name == "conv_thin_bf16<{}>".format(mode), name
    got = launch(mode, xd, wd, bh, bw, relu=True)
    one = launch(mode, xd[:1].contiguous(), wd, bh, bw, relu=True)
    torch.cuda.synchronize()
    err = (nchw(got) - want).abs()
    assert bool((err[bound == 0] == 0).all())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("{}: largest error / bound = {:.4f}".format(name, ratio))
    assert ratio <= 1.0, ratio
    assert torch.equal(one[0], got[0]), "image 0 depends on the batch it travels in"
