"""The fp32 Winograd DecoderBlock kernel's per-item state (conv_wino_f32.hip): an item's parity, cout block and sub-blocks are decoded once
and carried from item to item (no division by the item index), kept two deep -- the table builder and the fetch side run one item ahead of
the accumulators --, and the epilogue reads what was decoded.  These shapes aim at that state: blocks that walk three and four items (the
two-deep state wraps), the 128 x 64 block with several items per block, the 32-cout block with a dead second sub-block and with its two
sub-blocks in different images, the DG form with two output items (eight units) per block.  Each against a float64 reference with the
bound of tests/test_gpu_wino_pipeline.py (2e-5 of the reference's largest element); each forward case also bit for bit against its first
and its last image alone (batch independence)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _close(got, want, what, rel=2e-5):
    """fp32 kernel vs float64 reference: within `rel` of the reference's largest element."""
    err = float((got.double().cpu() - want).abs().max())
    bound = rel * max(1.0, float(want.abs().max()))
    assert err <= bound, (what, err, bound)


def _up_conv64(x, w):  # x [N,H,W,C] fp32 gpu, w [Cout,3,3,Cin] -> conv3x3(upsample x2(x)) in float64 NCHW on the CPU
    x64 = x.double().cpu().permute(0, 3, 1, 2)
    return F.conv2d(F.interpolate(x64, scale_factor=2, mode="nearest"), w.double().cpu().permute(0, 3, 1, 2), padding=1)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _forward(n, h, w, c1, c2, cout, name, seed, relu=True):
    from robosat_amd import ops

    g = _gen(seed)
    a = torch.randn(n, h, w, c1, device=DEV, generator=g)
    b = torch.randn(n, h, w, c2, device=DEV, generator=g) if c2 else None
    wk = torch.randn(cout, 3, 3, c1 + c2, device=DEV, generator=g) * (2.0 / (9 * (c1 + c2))) ** 0.5
    assert ops.wino_ok(a, b, cout, force=True)
    u = ops.pack_wino_phase_weight(ops.pack_phase_weight(wk))
    got = ops.conv2d_phase_wino(a, u, src2=b, relu=relu)
    ref = _up_conv64(a if b is None else torch.cat([a, b], 3), wk)
    _close(got.permute(0, 3, 1, 2), F.relu(ref) if relu else ref, name)
    # batch independence: the first and the last image alone are the same bits as inside the batch
    for i in (0, n - 1):
        alone = ops.conv2d_phase_wino(a[i:i + 1], u, src2=None if b is None else b[i:i + 1], relu=relu)
        assert torch.equal(alone[0], got[i]), (name, i)


@pytest.mark.parametrize("extra", [0, 1, 3])
def test_wino_blocks_walk_three_and_four_items(extra):
    """16 x 16 sources = one 8x8 patch per image, Cout 64: 4 n items on the 64 x 64 block, 3 CUs + {0, 4, 12} of them (rounded up to whole
    images): every block walks three items, some a fourth -- the two-deep item state is overwritten while its predecessor is in use."""
    n = (3 * _cus() + 3) // 4 + extra
    _forward(n, 16, 16, 32, 0, 64, "conv_wino_f32<phase,p8,64x64>", 81 + extra)


def test_wino_wide_block_several_items_per_block():
    """The 128 x 64 block runs where (nsub + 1) / 2 * (Cout / 64) * 4 >= 2 CUs: n = CUs + 3 images of one patch each at Cout 64 give
    4 ceil(n / 2) items of two sub-blocks (2 CUs + 8 at 256 CUs; n odd at an even CU count: the last m block's second sub-block is
    dead), two or three per block;
    C1 = 16, C2 = 16: nk = 2, the source switch on every item's second chunk."""
    n = _cus() + 3
    _forward(n, 16, 16, 16, 16, 64, "conv_wino_f32<phase,p8,128x64>", 84)


def test_wino_32_cout_block_dead_second_sub_block():
    """The 32-cout block holds two patches.  n = 3 at 18 x 22 (9 x 11 tiles: 2 x 2 ragged patches per image, 12 sub-blocks) and n = 3 at
    16 x 16 (one patch per image: 3 sub-blocks, the second item's second sub-block is dead), C = 32: nk = 2."""
    _forward(3, 18, 22, 32, 0, 32, "conv_wino_f32<phase,p8,128x32>", 85)
    _forward(3, 16, 16, 32, 0, 32, "conv_wino_f32<phase,p8,128x32>", 86)


def test_wino_sub_blocks_in_different_images():
    """n = 5 at 16 x 16 on the 32-cout block: every item's two sub-blocks are two images; the last item's second one is dead."""
    _forward(5, 16, 16, 16, 16, 32, "conv_wino_f32<phase,p8,128x32>", 87, relu=False)


def _dgrad(n, c1, c2, cout, hs, seed, masked=True):
    from robosat_amd import ops

    assert ops.wino_dgrad_ok(n, hs, hs, c1, c2, cout)
    g = _gen(seed)
    wk = torch.randn(cout, 3, 3, c1 + c2, device=DEV, generator=g) * 0.05
    dz = torch.randn(n, 2 * hs, 2 * hs, cout, device=DEV, generator=g)
    mask = torch.randn(n, hs, hs, c1 + c2, device=DEV, generator=g)
    u = ops.pack_wino_dgrad_weight(ops.pack_dgrad_phase_weight(wk))
    got, _ = ops.conv2d_dgrad_phase_wino(dz, u, c1, c2, mask1=mask if masked else None)
    x = torch.zeros(n, c1 + c2, hs, hs, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wk.double().cpu().permute(0, 3, 1, 2), padding=1)
    (y * dz.double().cpu().permute(0, 3, 1, 2)).sum().backward()
    ref = x.grad * (mask.cpu().permute(0, 3, 1, 2) > 0) if masked else x.grad
    _close(got.permute(0, 3, 1, 2), ref, "wino dgrad")
    return got, dz, u, mask


@pytest.mark.parametrize("n,c1,c2,cout,hs", [(2, 32, 32, 64, 16), (3, 64, 0, 32, 18)])
def test_wino_dgrad_items_vs_float64(n, c1, c2, cout, hs):
    _dgrad(n, c1, c2, cout, hs, 88)


def test_wino_dgrad_two_output_items_per_block():
    """One patch per image, 64 output channels = one cout block: n output items of four units each; n = CUs + 5 gives some blocks two
    output items (eight units: the plane-only decode of units 1 .. 3 twice, the full decode in between).  The first and the last image
    alone give the same bits."""
    from robosat_amd import ops

    n = _cus() + 5
    got, dz, u, mask = _dgrad(n, 64, 0, 32, 16, 89)
    for i in (0, n - 1):
        alone, _ = ops.conv2d_dgrad_phase_wino(dz[i:i + 1], u, 64, 0, mask1=mask[i:i + 1])
        assert torch.equal(alone[0], got[i]), i
