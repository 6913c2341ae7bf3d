"""The pixel form of the fp32 Winograd DecoderBlock forward (conv_wino_f32.hip, PIX = true): GEMM rows are source pixels, a sub-block is
an 8 x 8 patch of pixels with a 10 x 10 halo, a work item is (m block, cout block) without a parity, and filter position (r, c) comes
from slab [2 (r == 2) + (c == 2)][3 r + c] of the packed filters.  The smallest shapes that reach each mechanism, each against the float64
conv2d(interpolate) reference with the project's bound (2e-5 of the reference's largest element), and the first and the last image alone
bit for bit against the batch.  The block shape is asserted through rs_conv2d_phase_wino_name, never assumed.  Every launch says
`upsampled=True` (the DecoderBlock's contract, which the pixel form needs); the last test pins that a launch without it -- four free
parity filter sets, as the stride-2 data gradient passes them -- still computes the general four 2x2 convolutions.

Sub-blocks are 8 x 8 PIXELS here: 16 x 16 sources hold four per image (nsub is even at every n), so the cases that need an odd number
of sub-blocks -- a dead second sub-block, an item whose two sub-blocks lie in two images -- use 18 x 22 sources (3 x 3 = 9 per image)
with an odd n."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W64, W128X64, W128X32 = "conv_wino_f32<phase,p8,64x64>", "conv_wino_f32<phase,p8,128x64>", "conv_wino_f32<phase,p8,128x32>"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _name(n, h, w, c1, c2, cout):
    import ctypes

    from robosat_amd import _lib, ops

    d = ops._phase_desc(n, h, w, c1, c2, cout)
    return _lib.lib().rs_conv2d_phase_wino_name(ctypes.byref(d)).decode()


def _wide_n(regions_per_image, odd=False):
    """Smallest n at which the wide rule holds for Cout 64: (n regions + 1) // 2 * 4 >= 2 CUs."""
    n = 1
    while (n * regions_per_image + 1) // 2 * 4 < 2 * _cus() or (odd and n % 2 == 0):
        n += 1
    return n


def _forward(n, h, w, c1, c2, cout, name, seed, relu=True, borders=False):
    from robosat_amd import ops

    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(n, h, w, c1, device=DEV, generator=g)
    b = torch.randn(n, h, w, c2, device=DEV, generator=g) if c2 else None
    wk = torch.randn(cout, 3, 3, c1 + c2, device=DEV, generator=g) * (2.0 / (9 * (c1 + c2))) ** 0.5
    assert ops.wino_ok(a, b, cout, force=True)
    assert _name(n, h, w, c1, c2, cout) == name
    u = ops.pack_wino_phase_weight(ops.pack_phase_weight(wk))
    got = ops.conv2d_phase_wino(a, u, src2=b, relu=relu, upsampled=True)
    x64 = (a if b is None else torch.cat([a, b], 3)).double().cpu().permute(0, 3, 1, 2)
    ref = F.conv2d(F.interpolate(x64, scale_factor=2, mode="nearest"), wk.double().cpu().permute(0, 3, 1, 2), padding=1)
    ref = F.relu(ref) if relu else ref
    gotc = got.permute(0, 3, 1, 2).double().cpu()
    bound = 2e-5 * max(1.0, float(ref.abs().max()))
    err = float((gotc - ref).abs().max())
    assert err <= bound, (name, err, bound)
    if borders:  # the four borders of each of the four parities, named: a masked or misplaced ragged row shows here first
        for u_ in (0, 1):
            for v_ in (0, 1):
                gp, rp = gotc[:, :, u_::2, v_::2], ref[:, :, u_::2, v_::2]
                for what, sl in (("top", (slice(0, 1), slice(None))), ("bottom", (slice(-1, None), slice(None))),
                                 ("left", (slice(None), slice(0, 1))), ("right", (slice(None), slice(-1, None)))):
                    e = float((gp[:, :, sl[0], sl[1]] - rp[:, :, sl[0], sl[1]]).abs().max())
                    assert e <= bound, (name, "parity", u_, v_, what, e, bound)
    for i in (0, n - 1):  # batch independence
        alone = ops.conv2d_phase_wino(a[i:i + 1], u, src2=None if b is None else b[i:i + 1], relu=relu, upsampled=True)
        assert torch.equal(alone[0], got[i]), (name, i)


@pytest.mark.parametrize("cout,name", [(64, W64), (32, W128X32)])
@pytest.mark.parametrize("relu", [True, False])
def test_smallest_qualifying_layer(cout, name, relu):
    """16 x 16 sources, C = 32 (nk = 2: the next item's table is built in an item's first chunk and read in its last)."""
    _forward(2, 16, 16, 32, 0, cout, name, 101, relu=relu)


def test_wide_block():
    """The 128 x 64 block at 16 x 16, Cout 64, with as many images as the wide rule needs at this CU count; the images alone run on the
    64 x 64 block and must give the same bits."""
    _forward(_wide_n(1), 16, 16, 32, 0, 64, W128X64, 102)


def test_wide_block_dead_second_sub_block():
    """18 x 22 sources are four regions of 16 x 16 and nine 8 x 8 sub-blocks per image: an odd n makes nsub odd, the last item's second
    sub-block is dead (its halo rows arrive as zeros, its waves store nothing)."""
    _forward(_wide_n(4, odd=True), 18, 22, 16, 16, 64, W128X64, 103)


@pytest.mark.parametrize("h,w", [(18, 22), (15, 17)])
@pytest.mark.parametrize("cout,name", [(64, W64), (32, W128X32)])
def test_partial_patches_and_odd_sizes(h, w, cout, name):
    """Ragged 8 x 8 patches: pixels past Hs / Ws are masked per pixel (the tile form padded whole tiles).  n = 3 at 18 x 22: 27
    sub-blocks, so on the 32-cout block every other item's two sub-blocks lie in two images and the last one's second is dead."""
    _forward(3, h, w, 32, 0, cout, name, 104, borders=True)


@pytest.mark.parametrize("c1,c2", [(16, 16), (48, 16)])
@pytest.mark.parametrize("cout,name", [(64, W64), (32, W128X32)])
def test_two_sources(c1, c2, cout, name):
    """The C1 -> C2 switch on an item's second chunk of two, and on the last of four."""
    _forward(2, 16, 16, c1, c2, cout, name, 105)


def test_sub_blocks_across_images():
    """n = 5 at 18 x 22 on the 32-cout block: 45 sub-blocks, two per item -- items 4, 13 and 22 span two images, the last is half dead."""
    _forward(5, 18, 22, 16, 16, 32, W128X32, 106, relu=False)


@pytest.mark.parametrize("extra", [0, 1, 3])
def test_blocks_walk_three_and_four_items(extra):
    """16 x 16 sources, Cout 64: 4 n items on the 64 x 64 block; 3 CUs + {0, 4, 12} of them: every block walks three items, some a
    fourth -- the two-deep item state is overwritten while its predecessor is in use."""
    _forward((3 * _cus() + 3) // 4 + extra, 16, 16, 32, 0, 64, W64, 107 + extra)


@pytest.mark.parametrize("cout,name", [(96, W128X32), (128, W64)])
def test_slab_offset_with_a_cout_block(cout, name):
    """Cout 96 = three cout blocks of 32, Cout 128 = two of 64: the position's slab offset and the item's cout block add up."""
    _forward(2, 16, 16, 32, 0, cout, name, 110)


def test_free_parity_filters_keep_the_tile_form():
    """`conv2d_phase_wino` without `upsampled` takes ANY phase pack: four unrelated 2x2 filter sets, against four 2x2 correlations in
    float64 (parity (py, px) of the output reads source rows y - 1 + py + r, columns x - 1 + px + s)."""
    from robosat_amd import ops

    g = torch.Generator(device=DEV).manual_seed(111)
    n, h, w, c, cout = 2, 16, 18, 32, 64
    a = torch.randn(n, h, w, c, device=DEV, generator=g)
    pack = torch.randn(4, cout, 2, 2, c, device=DEV, generator=g) * (2.0 / (4 * c)) ** 0.5
    got = ops.conv2d_phase_wino(a, ops.pack_wino_phase_weight(pack)).permute(0, 3, 1, 2).double().cpu()
    x64 = F.pad(a.double().cpu().permute(0, 3, 1, 2), (1, 1, 1, 1))
    ref = torch.zeros(n, cout, 2 * h, 2 * w, dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            k = pack[2 * py + px].double().cpu().permute(0, 3, 1, 2)  # [Cout, C, 2, 2]
            ref[:, :, py::2, px::2] = F.conv2d(x64[:, :, py:py + h + 1, px:px + w + 1], k)
    err, bound = float((got - ref).abs().max()), 2e-5 * max(1.0, float(ref.abs().max()))
    assert err <= bound, (err, bound)


def test_pixel_forms_beside_an_lds_user():
    """The three pixel blocks twice on the same data, each time with LDS-DMA traffic of a neighbour on four side streams: bit for bit (the
    screen of tests/test_gpu_wino_pipeline.py, whose launches say nothing about their filters and therefore keep the tile form; the
    positive control that shows such a neighbour exposes a missing wait is tests/test_gpu_race_screen.py's)."""
    from robosat_amd import ops

    g = torch.Generator(device=DEV).manual_seed(112)
    sides = [torch.cuda.Stream() for _ in range(4)]
    nx = torch.randn(32, 64, 64, 256, device=DEV, generator=g).to(torch.bfloat16)
    nw = (torch.randn(64, 1, 1, 256, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    no = [torch.empty(32, 64, 64, 64, device=DEV, dtype=torch.bfloat16) for _ in range(4)]

    def neighbour():
        for side, o in zip(sides, no):
            with torch.cuda.stream(side):
                for _ in range(6):
                    ops.conv2d(nx, nw, out=o)

    nwide = -(-_wide_n(16) // 4) * 4
    a = torch.randn(nwide, 64, 64, 16, device=DEV, generator=g)
    b = torch.randn(nwide, 64, 64, 16, device=DEV, generator=g)
    u64 = ops.pack_wino_phase_weight(ops.pack_phase_weight(torch.randn(64, 3, 3, 32, device=DEV, generator=g) * 0.08))
    u32 = ops.pack_wino_phase_weight(ops.pack_phase_weight(torch.randn(32, 3, 3, 32, device=DEV, generator=g) * 0.08))
    assert _name(nwide, 64, 64, 16, 16, 64) == W128X64 and _name(4, 64, 64, 16, 16, 64) == W64 and _name(4, 64, 64, 16, 16, 32) == W128X32
    runs = [lambda: ops.conv2d_phase_wino(a, u64, src2=b, relu=True, upsampled=True),
            lambda: ops.conv2d_phase_wino(a[:4], u64, src2=b[:4], relu=True, upsampled=True),
            lambda: ops.conv2d_phase_wino(a[:4], u32, src2=b[:4], relu=True, upsampled=True)]
    bad = []
    for r in range(10):
        for i, fn in enumerate(runs):
            torch.cuda.synchronize()
            neighbour()
            one = fn()
            neighbour()
            two = fn()
            if not torch.equal(one, two):
                bad.append((r, i))
    torch.cuda.synchronize()
    assert not bad, bad
