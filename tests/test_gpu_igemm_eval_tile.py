"""The fp32 direct-form EPI_EVAL launches of the LDS-DMA implicit GEMM (csrc/conv_igemm_dma_kernel.h) at the places where their per-tile
code can go wrong: the epilogue kinds fixed at compile time (scale + shift, + ReLU, + residual + ReLU) with a whole pass's residual pieces
in flight, the table-free prologue of the plain 1x1 launches (FAST1), and everything that must keep the gather table and the run-time
epilogue (strided 1x1, 3x3, two concat sources, no scale, ReLU mask, two destinations, a scale that is not 16-byte aligned).

Exact checks: inputs, weights, scale, shift and residual are small integers, so every fp32 sum is exact whatever its order (the bound is
asserted) and the result must be ``torch.equal`` to ``F.conv2d`` + the epilogue on the host.  One randomised check per tile against
float64 at the suite's fp32 bar (2e-4 of the output scale).

Shapes: M = 81 (< BM) and M = 3 * 11 * 13 = 429 (a ragged last tile, tiles straddling two images); Cin 32 / 64 / 96 = 2 / 4 / 6 chunks
at 64-byte rows and 1 / 2 / 3 at 128 (nk = 1 runs only the chunk without a fetch); Cout 32 / 96 / 160 (a ragged last N tile at
BN = 128; where the forced tile cannot run a Cout the dispatcher answers as it always did, and the name says so) plus 64 / 128, the
whole N tiles of the 64-wide forms."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILES = ["128x128", "128x64", "128x32", "64x64"]
ROWS = [64, 128]
SHAPES = [(1, 9, 9), (3, 11, 13)]
CINS = [32, 64, 96]
COUTS = [32, 96, 160, 64, 128]
EXACT = float(1 << 24)


def ints(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def krsc(w):
    return w.permute(0, 2, 3, 1).contiguous().to(DEV)


def expected_name(tile, rowb, cout):
    """What the dispatcher reports under a forced (tile, rowb) at these small M: the forced tile where its N tiles are whole (128x128:
    also ragged behind 128 couts), else its own choice -- 64x64 for whole 64-cout tiles, 128x32 otherwise."""
    bn = int(tile.split("x")[1])
    if not (cout % bn == 0 or (tile == "128x128" and cout > 128)):
        tile = "64x64" if cout % 64 == 0 else "128x32"
    return "conv_igemm_f32<{},r{}>".format(tile, rowb)


@functools.lru_cache(maxsize=None)
def problem(n, h, w, cin, cout, k=1, stride=1, pad=0):
    """Integer operands (host, NCHW / OIHW) and the raw convolution, shared by every tile and kind; left unchanged."""
    seed = 1000 * cin + 10 * cout + n + 7 * k + stride
    x, wt = ints(-2, 2, n, cin, h, w, seed=seed), ints(-1, 1, cout, cin, k, k, seed=seed + 1)
    base = F.conv2d(x, wt, stride=stride, padding=pad)
    sc, sh = ints(1, 3, cout, seed=seed + 2), ints(-4, 4, cout, seed=seed + 3)
    res, mask = ints(-9, 9, *base.shape, seed=seed + 4), ints(-1, 1, *base.shape, seed=seed + 5)
    # precondition: every partial sum and every epilogue value is an integer below 2^24, hence exact in fp32 in any order
    assert 2.0 * cin * k * k * 3.0 + 4.0 + 9.0 < EXACT and float(base.abs().max()) * 3 + 13 < EXACT
    return x, wt, base, sc, sh, res, mask


def run_kinds(tile, rowb, n, h, w, cin, cout, k=1, stride=1, pad=0, two_sources=False):
    """Every epilogue kind of one launch shape, each ``torch.equal`` to the host; the reported name is the parent's."""
    from robosat_amd import ops

    x, wt, base, sc, sh, res, mask = problem(n, h, w, cin, cout, k, stride, pad)
    xd, wd = nhwc(x), krsc(wt)
    scd, shd, resd, maskd = sc.to(DEV), sh.to(DEV), nhwc(res), nhwc(mask)
    kw = dict(stride=stride, pad=pad)
    if two_sources:  # torch.cat fused into the gather: the first 32 channels are source 1
        src = dict(src1=xd[..., :32].contiguous(), src2=xd[..., 32:].contiguous())
    else:
        src = dict(src1=xd)
    v = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    off = torch.zeros(cout + 1, device=DEV)  # scale at a 4-byte offset: not a 16-byte piece, the run-time path
    off[1:] = scd
    cases = [
        ("none", {}, base),
        ("scale+shift", dict(scale=scd, shift=shd), base * v(sc) + v(sh)),
        ("scale+shift+relu", dict(scale=scd, shift=shd, relu=True), F.relu(base * v(sc) + v(sh))),
        ("scale+shift+res+relu", dict(scale=scd, shift=shd, residual=resd, relu=True), F.relu(base * v(sc) + v(sh) + res)),
        ("scale+shift+res", dict(scale=scd, shift=shd, residual=resd), base * v(sc) + v(sh) + res),
        ("res", dict(residual=resd), base + res),
        ("res+relu", dict(residual=resd, relu=True), F.relu(base + res)),
        ("mask", dict(relu_mask=maskd), torch.where(mask > 0, base, torch.zeros(()))),
        ("res+mask", dict(residual=resd, relu_mask=maskd), torch.where(mask > 0, base + res, torch.zeros(()))),
        ("unaligned scale", dict(scale=off[1:], shift=shd, residual=resd, relu=True), F.relu(base * v(sc) + v(sh) + res)),
    ]
    with ops.tuning(tile=tile, rowb=rowb):
        d = ops.conv_desc(src["src1"], wd, src.get("src2"), 0, stride, pad)
        name = ops.conv_tile_name(d)
        assert name == expected_name(tile, rowb, cout), (name, tile, rowb, cout)
        for what, opts, want in cases:
            got = ops.conv2d(weight=wd, **src, **kw, **opts)
            torch.cuda.synchronize()
            assert torch.equal(nchw(got), want), "{} {} r{} {}x{}x{} {}->{} k{} s{}".format(what, tile, rowb, n, h, w, cin, cout, k, stride)


@pytest.mark.parametrize("rowb", ROWS)
@pytest.mark.parametrize("tile", TILES)
def test_plain_1x1_every_kind_is_exact(tile, rowb):
    """The launches that take the table-free prologue: M < BM and M ragged over two images, 1 .. 6 K-chunks, ragged N."""
    for n, h, w in SHAPES:
        for cin in CINS:
            for cout in COUTS:
                run_kinds(tile, rowb, n, h, w, cin, cout)


@pytest.mark.parametrize("rowb", ROWS)
@pytest.mark.parametrize("tile", TILES)
def test_launches_that_keep_the_gather_table_are_exact(tile, rowb):
    """1x1 stride 2, 3x3 pad 1 at stride 1 and 2, 1x1 over two concat sources: same tiles, same kinds, the table prologue."""
    for cout in (96, 160, 64):
        run_kinds(tile, rowb, 3, 11, 13, 64, cout, k=1, stride=2)
        run_kinds(tile, rowb, 3, 11, 13, 32, cout, k=3, stride=1, pad=1)
        run_kinds(tile, rowb, 3, 11, 13, 32, cout, k=3, stride=2, pad=1)
        run_kinds(tile, rowb, 3, 11, 13, 96, cout, two_sources=True)


SPLIT = {"128x128": (160, 128), "128x64": (128, 64), "128x32": (96, 32), "64x64": (128, 64)}  # (Cout, csplit): csplit % BN == 0


@pytest.mark.parametrize("rowb", ROWS)
@pytest.mark.parametrize("tile", TILES)
def test_two_destinations_with_a_mask_on_one_side(tile, rowb):
    from robosat_amd import ops

    cout, c1 = SPLIT[tile]
    for n, h, w in SHAPES:
        x, wt, base, _, _, _, mask = problem(n, h, w, 64, cout)
        m2 = mask[:, c1:].contiguous()
        with ops.tuning(tile=tile, rowb=rowb):
            o1, o2 = ops.conv2d_split(nhwc(x), krsc(wt), c1, mask2=nhwc(m2))
            torch.cuda.synchronize()
        assert torch.equal(nchw(o1), base[:, :c1])
        assert torch.equal(nchw(o2), torch.where(m2 > 0, base[:, c1:], torch.zeros(())))


@pytest.mark.parametrize("rowb", ROWS)
@pytest.mark.parametrize("tile", TILES)
def test_random_operands_against_float64_and_across_batch_sizes(tile, rowb):
    """Gaussian operands, scale + shift + residual + ReLU and scale + shift alone: within 2e-4 of the output scale of float64; image 0
    alone equals image 0 inside a batch of three bit for bit (M = 143 per image: tiles straddle images in the batch)."""
    from robosat_amd import ops

    g = torch.Generator().manual_seed(5)
    n, h, w, cin = 3, 11, 13, 96
    cout = 160 if tile == "128x128" else (96 if tile == "128x32" else 128)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    res = torch.randn(n, cout, h, w, generator=g)
    base = F.conv2d(x.double(), wt.double()) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    xd, wd, scd, shd, resd = nhwc(x), krsc(wt), sc.to(DEV), sh.to(DEV), nhwc(res)
    with ops.tuning(tile=tile, rowb=rowb):
        assert ops.conv_tile_name(ops.conv_desc(xd, wd)) == expected_name(tile, rowb, cout)
        for opts, want in ((dict(residual=resd, relu=True), F.relu(base + res.double())), ({}, base)):
            got = ops.conv2d(xd, wd, scale=scd, shift=shd, **opts)
            one = ops.conv2d(xd[:1].contiguous(), wd, scale=scd, shift=shd, **({k: (v[:1].contiguous() if k == "residual" else v) for k, v in opts.items()}))
            torch.cuda.synchronize()
            err, scale = float((nchw(got).double() - want).abs().max()), float(want.abs().max())
            print("{} r{} {}: max abs err {:.3e} of scale {:.3e}".format(tile, rowb, sorted(opts), err, scale))
            assert err <= 2e-4 * scale, (err, scale)
            assert torch.equal(one[0], got[0]), "image 0 depends on the batch it travels in"
