"""The 7x7 / stride-2 stem (resnet.conv1) on its four kernels -- stem_conv_f32<3|4> (stem_f32.hip), conv_wgrad_f32<64,32,..,FORM=1>
(conv_wgrad.hip), stem_fwd_bf16_kernel and stem_wgrad_bf16_kernel (stem_bf16.hip) -- at the shapes where their state can go wrong:
odd borders, a one-pixel second tile, images smaller than the window, persistent blocks that run several tiles / patches across
output rows and images with a dead last prefetch, ragged chunks and short splits of the fp32 weight gradient.

Two checks per kernel:
  exact   inputs drawn from small integers: every product and partial sum is an integer below 2^24 (below 256 for a bf16 output), so
          any summation order, MFMA or split reduction gives the reference's bits: torch.equal.  A dropped, doubled or misplaced pixel
          cannot hide in a relative bound here.  That the reference stays inside the range is asserted as a precondition.
  float   Gaussian data against float64 on the host: 2e-5 of the reference's largest element for the fp32 forward (the bar of
          tests/test_gpu_wino_pipeline.py); |err| <= 1e-5 * S per element for both weight gradients, S = sum |dy| |x| in float64 (the
          same autograd on absolute values); |err| <= 2^-8 |ref| + 1e-5 max |ref| per element for the bf16 forward on bf16-rounded
          operands (one bf16 rounding, a factor 2 for ties after the fp32 accumulation).

The counts a shape aims at (tiles per block, patches per block, chunks per split) are asserted next to it: after a change of launch
policy the test says that it no longer aims at anything."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
EXACT = float(1 << 24)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).double()


def _randn(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed), dtype=torch.float64)


def _q(t):  # round to bf16, keep float64 storage
    return t.float().to(BF).double()


def _krsc(w):  # OIHW host -> KRSC fp32 device
    return w.float().permute(0, 2, 3, 1).contiguous().to(DEV)


def _nchw(t):  # NHWC device -> NCHW float64 host
    return t.double().permute(0, 3, 1, 2).cpu()


def _conv(x, w):
    return F.conv2d(x, w, stride=2, padding=3)


def _epilogue(y, sc, sh):
    return torch.relu(y * sc.to(y.dtype).view(1, -1, 1, 1) + sh.to(y.dtype).view(1, -1, 1, 1))


def _int_epilogue(seed):
    """Per-channel scale from {0.5, 1, 2} and an integer shift: exact on integer sums."""
    sc = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (64,), generator=_gen(seed))]
    return sc, _ints(-3, 3, 64, seed=seed + 1)


def _wgrad_ref(x, dy):
    """Gradient of the stem filter [64, Cin, 7, 7] by autograd, in the dtype of x and dy."""
    w = torch.zeros(64, x.shape[1], 7, 7, dtype=x.dtype, requires_grad=True)
    _conv(x, w).backward(dy)
    return w.grad


def _check_wgrad_float(got, x, dy, what):
    """|got - ref| <= 1e-5 * S per element; ref and S = sum |dy| |x| in float64."""
    ref, s = _wgrad_ref(x, dy), _wgrad_ref(x.abs(), dy.abs())
    excess = (got - ref).abs() - 1e-5 * s
    assert float(excess.max()) <= 0.0, (what, float(((got - ref).abs() / s.clamp_min(1e-300)).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 forward: stem_conv_f32<3> (RGB: the 4th band is skipped) and stem_conv_f32<4>
# ---------------------------------------------------------------------------------------------------------------------------------
def _many_tiles_shape():
    """3 x 199 x 300 at 256 CUs: 600 tiles of 128 pixels (two per output row, the second ragged) on one block per CU (four bands) --
    runs of two and three tiles that cross output rows and images, the odd bottom row in mid-run.  H grows with the CU count."""
    ho = max(100, _cus() // 3 + 1)  # 3 images x ho rows x 2 tiles > 2 CUs
    return 3, 2 * ho - 1, 300


F32_FWD = {
    "odd_37x45": (2, 37, 45),     # odd bottom and right borders, Wo = 23
    "wo128": (1, 9, 256),         # one full tile per row
    "wo129": (1, 9, 257),         # a one-pixel second tile
    "tiny_3x5": (2, 3, 5),        # smaller than the 7x7 window
    "tiny_1x1": (1, 1, 1),
    "many_tiles": None,           # _many_tiles_shape()
}


def _f32_fwd_case(name):
    n, h, w = F32_FWD[name] or _many_tiles_shape()
    ho, wo = (h + 1) // 2, (w + 1) // 2
    tpr = (wo + 127) // 128
    ntile = n * ho * tpr
    if name == "wo128":
        assert (wo, tpr) == (128, 1)
    if name == "wo129":
        assert (wo, tpr) == (129, 2)
    if name == "many_tiles":
        # the grid is one block per CU (four bands) or two (RGB): every four-band block runs 2+ tiles, RGB blocks one or two
        assert h % 2 == 1 and tpr == 2 and ntile > 2 * _cus(), (n, h, w, ntile, _cus())
    return n, h, w, ho, wo


def _run_f32_fwd(x, wt, bands, sc=None, sh=None):
    """x NCHW float64 host, wt OIHW float64 host -> NHWC fp32 device output of the stem kernel (raw, or scale / shift / ReLU)."""
    from robosat_amd import ops

    x4 = ops.nchw_to_nhwc4(x.float().to(DEV))
    if bands == 3:
        x4[..., 3] = 1e30  # the RGB form is told to skip the 4th band, and must
    packed = ops.pack_stem_weight(_krsc(wt))
    kw = {} if sc is None else dict(scale=sc.float().to(DEV), shift=sh.float().to(DEV), relu=True)
    out = ops.conv2d(x4, packed, stride=2, pad=3, stem=7, bands=bands, **kw)
    # batch independence, bit for bit: the first and the last image alone
    for i in {0, x.shape[0] - 1} if x.shape[0] > 1 else ():
        alone = ops.conv2d(x4[i:i + 1].contiguous(), packed, stride=2, pad=3, stem=7, bands=bands, **kw)
        assert torch.equal(alone[0], out[i]), ("image alone != in the batch", i)
    return out


@pytest.mark.parametrize("bands", [3, 4])
@pytest.mark.parametrize("name", list(F32_FWD))
def test_stem_f32_forward_exact(name, bands):
    """x, w in {-3..3}: |y| <= 196 * 9, every partial sum an integer: the kernel's bits are F.conv2d's."""
    n, h, w, ho, wo = _f32_fwd_case(name)
    x, wt = _ints(-3, 3, n, bands, h, w, seed=101), _ints(-3, 3, 64, bands, 7, 7, seed=102)
    ref = _conv(x, wt)
    assert tuple(ref.shape) == (n, 64, ho, wo) and float(ref.abs().max()) <= 196 * 9 < EXACT
    assert torch.equal(_nchw(_run_f32_fwd(x, wt, bands)), ref), "raw"
    sc, sh = _int_epilogue(103)
    want = _epilogue(ref, sc, sh)
    assert float(want.abs().max()) < EXACT
    assert torch.equal(_nchw(_run_f32_fwd(x, wt, bands, sc, sh)), want), "scale / shift / ReLU"


@pytest.mark.parametrize("bands", [3, 4])
@pytest.mark.parametrize("name", list(F32_FWD))
def test_stem_f32_forward_float64(name, bands):
    """Gaussian data: within 2e-5 of the float64 reference's largest element, raw and with the epilogue."""
    n, h, w, _, _ = _f32_fwd_case(name)
    x, wt = _randn(n, bands, h, w, seed=111).float().double(), (_randn(64, bands, 7, 7, seed=112) * 0.1).float().double()
    sc, sh = _randn(64, seed=113).float().double(), _randn(64, seed=114).float().double()
    ref = _conv(x, wt)
    for what, got, want in (("raw", _run_f32_fwd(x, wt, bands), ref),
                            ("epilogue", _run_f32_fwd(x, wt, bands, sc, sh), _epilogue(ref, sc, sh))):
        err, bound = float((_nchw(got) - want).abs().max()), 2e-5 * float(want.abs().max())
        assert err <= bound, (what, err, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 weight gradient: conv_wgrad_f32<64, 32, 2, 1, FORM = 1> through conv2d_wgrad(stem=7)
# ---------------------------------------------------------------------------------------------------------------------------------
F32_WGRAD = {
    # name: (N, H, W), (chunks of 32 pixels, chunks per split, splits)
    "ragged_3x37x45": ((3, 37, 45), (41, 7, 6)),   # M = 1311: the last split has 6 chunks, its last chunk 31 pixels
    "many_images_20x9x11": ((20, 9, 11), (19, 7, 3)),  # M = 600: splits of 224 pixels over 7+ images of 30 pixels (the last has 5 chunks)
    "control_1x64x96": ((1, 64, 96), (48, 8, 6)),  # M = 1536: one image, even sizes, equal splits
}


def _f32_wgrad_case(name):
    from robosat_amd import _lib, ops

    (n, h, w), (chunks, cps, splits) = F32_WGRAD[name]
    ho, wo = (h + 1) // 2, (w + 1) // 2
    m = n * ho * wo
    # conv_wgrad.hip's plan(): 7 tiles (one per filter row); as many splits as reach the block target, of at least 8 chunks each
    tot = (m + 31) // 32
    s = max(1, min((ops.get_knob("wgrad_f32_blocks") + 6) // 7, (tot + 7) // 8))
    per = (tot + s - 1) // s
    assert (tot, per, (tot + per - 1) // per) == (chunks, cps, splits), (name, tot, per)
    # ... and the library's own count: the workspace is [splits][64][224] floats (no reduction scratch up to 8 splits)
    d = ops.ConvDesc(n, h, w, 4, 0, 0, 7, 7, 2, 3, ho, wo, 64, 0, 1)
    assert _lib.lib().rs_conv2d_wgrad_workspace_bytes(ctypes.byref(d)) == splits * 64 * 224 * 4
    if name.startswith("ragged"):
        assert chunks - (splits - 1) * cps == 6 and m - 32 * (chunks - 1) == 31
    if name.startswith("many_images"):
        assert cps * 32 // (ho * wo) >= 7
    return n, h, w, ho, wo


def _run_f32_wgrad(x, dy, bands):
    """x NCHW, dy NCHW (float64 host) -> KRSC gradient [64, 7, 7, bands] as OIHW float64 on the host.  The packed gradient holds a
    tap 7 (real products of the pixel one to the right of the window) and, for RGB, a band 3: neither may reach the unpacked filter."""
    from robosat_amd import ops

    x4 = ops.nchw_to_nhwc4(x.float().to(DEV))
    dwp = ops.conv2d_wgrad(dy.float().permute(0, 2, 3, 1).contiguous().to(DEV), x4, 7, 7, stride=2, pad=3, stem=7)
    assert tuple(dwp.shape) == (64, 7, 8, 4)
    dw = ops.unpack_stem_weight(dwp, 7, bands)
    assert torch.equal(dw, dwp[:, :, :7, :bands]), "unpack_stem_weight"
    if bands == 3:
        assert float(dwp[:, :, :7, 3].abs().max()) == 0.0, "gradient of the zero band"
    return _nchw(dw)


@pytest.mark.parametrize("bands", [3, 4])
@pytest.mark.parametrize("name", list(F32_WGRAD))
def test_stem_f32_wgrad_exact(name, bands):
    """x, dy in {-3..3}: |dW| <= 9 M < 2^24, every partial tile and their sum exact."""
    n, h, w, ho, wo = _f32_wgrad_case(name)
    x, dy = _ints(-3, 3, n, bands, h, w, seed=121), _ints(-3, 3, n, 64, ho, wo, seed=122)
    ref = _wgrad_ref(x, dy)
    assert 9 * n * ho * wo < EXACT and float(ref.abs().max()) < EXACT
    assert torch.equal(_run_f32_wgrad(x, dy, bands), ref)


@pytest.mark.parametrize("bands", [3, 4])
@pytest.mark.parametrize("name", list(F32_WGRAD))
def test_stem_f32_wgrad_float64(name, bands):
    """Gaussian data: |err| <= 1e-5 * S per element against float64."""
    n, h, w, ho, wo = _f32_wgrad_case(name)
    x, dy = _randn(n, bands, h, w, seed=131).float().double(), _randn(n, 64, ho, wo, seed=132).float().double()
    _check_wgrad_float(_run_f32_wgrad(x, dy, bands), x, dy, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16 forward: stem_fwd_bf16_kernel (patches of 8 x 16 outputs, at most 2048 blocks)
# ---------------------------------------------------------------------------------------------------------------------------------
def _bf16_fwd_counts(n, h, w):
    """rs_stem_conv_fwd_bf16's launch: (patches, patches per block, blocks, patches of the last block, patches per image)."""
    ppi = (h // 16) * (w // 32)
    total = n * ppi
    per = -(-total // min(total, 2048))
    blocks = -(-total // per)
    return total, per, blocks, total - (blocks - 1) * per, ppi


def _run_bf16_fwd(x, wt, sc=None, sh=None):
    """x NCHW, wt OIHW (host, bf16-representable) -> NHWC bf16 device output."""
    from robosat_amd import ops

    x4 = ops.nchw_to_nhwc4(x.float().to(DEV), BF)
    wp = ops.pack_stem_weight(_krsc(wt), BF)
    if sc is None:
        return ops.stem_conv_bf16(x4, wp)
    return ops.stem_conv_bf16(x4, wp, scale=sc.float().to(DEV), shift=sh.float().to(DEV), relu=True)


def _equal_nhwc(got, want_nchw):
    """got NHWC on the device == want NCHW on the host (compared on the device: the big case is 71 M elements)."""
    return torch.equal(got.float(), want_nchw.float().permute(0, 2, 3, 1).contiguous().to(DEV))


@pytest.mark.parametrize("n,bands,counts", [(9, 3, (2304, 2, 1152, 2, 256)), (17, 4, (4352, 3, 1451, 2, 256))])
def test_stem_bf16_forward_exact(n, bands, counts):
    """x, w in {-1, 0, 1}: |y| <= 196 < 256, so the fp32 sums and their bf16 roundings are exact.  9 images: two patches per block.
    17 images: three per block, two in the last (the dead prefetch follows a short run); 256 patches per image is no multiple of
    three, so runs cross images.  float32 on the host is exact here too."""
    h, w = 256, 512
    assert _bf16_fwd_counts(n, h, w) == counts
    if n == 17:
        assert counts[4] % counts[1] != 0, "runs must cross images"
    x, wt = _ints(-1, 1, n, bands, h, w, seed=141).float(), _ints(-1, 1, 64, bands, 7, 7, seed=142).float()
    ref = _conv(x, wt)
    assert float(ref.abs().max()) <= 196 < 256
    assert _equal_nhwc(_run_bf16_fwd(x, wt), ref), "raw"
    sc, sh = _int_epilogue(143)
    want = _epilogue(ref, sc, sh)
    assert float(want.abs().max()) < 256 and torch.equal(want.to(BF).float(), want), "the reference must be bf16 values"
    assert _equal_nhwc(_run_bf16_fwd(x, wt, sc, sh), want), "scale / shift / ReLU"


def test_stem_bf16_forward_float64():
    """9 x 256 x 512 (two patches per block), Gaussian operands rounded to bf16: |got - ref| <= 2^-8 |ref| + 1e-5 max |ref|."""
    n, h, w = 9, 256, 512
    assert _bf16_fwd_counts(n, h, w)[:3] == (2304, 2, 1152)
    x, wt = _q(_randn(n, 3, h, w, seed=151)), _q(_randn(64, 3, 7, 7, seed=152) * 0.1)
    sc, sh = _randn(64, seed=153).float().double(), _randn(64, seed=154).float().double()
    ref = _conv(x, wt)
    for what, got, want in (("raw", _run_bf16_fwd(x, wt), ref), ("epilogue", _run_bf16_fwd(x, wt, sc, sh), _epilogue(ref, sc, sh))):
        excess = (_nchw(got) - want).abs() - (want.abs() / 256 + 1e-5 * float(want.abs().max()))
        assert float(excess.max()) <= 0.0, (what, float(excess.max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16 weight gradient: stem_wgrad_bf16_kernel (patches of 8 x 8 outputs, at most 512 blocks, accumulators carried across a block's
# patches) + rs_reduce_splits over the blocks in use
# ---------------------------------------------------------------------------------------------------------------------------------
BF16_WGRAD = [
    # N, bands, H, W, (patches, patches per block, blocks in use, patches of the last block)
    (5, 4, 256, 256, (1280, 3, 427, 2)),   # 256 patches per image: runs cross images
    (3, 3, 224, 224, (588, 2, 294, 2)),
    (2, 4, 64, 96, (48, 1, 48, 1)),        # control: one patch per block
]


def _bf16_wgrad_case(n, h, w, counts):
    from robosat_amd import _lib

    total = n * (h // 16) * (w // 16)
    blocks = min(total, 512)
    per = -(-total // blocks)
    used = -(-total // per)
    assert (total, per, used, total - (used - 1) * per) == counts
    # the library's own block count: workspace = [blocks][64][224] floats + 32 tiles of reduction scratch above 8 blocks
    tile = 64 * 224 * 4
    assert _lib.lib().rs_stem_conv_wgrad_bf16_workspace_bytes(n, h, w) == (blocks + (32 if blocks > 8 else 0)) * tile


def _run_bf16_wgrad(x, dy, bands):
    from robosat_amd import ops

    x4 = ops.nchw_to_nhwc4(x.float().to(DEV), BF)
    dwp = ops.stem_conv_wgrad_bf16(dy.float().permute(0, 2, 3, 1).contiguous().to(DEV).to(BF), x4)
    assert tuple(dwp.shape) == (64, 7, 8, 4) and dwp.dtype == torch.float32
    dw = ops.unpack_stem_weight(dwp, 7, bands)
    assert torch.equal(dw, dwp[:, :, :7, :bands]), "unpack_stem_weight"
    if bands == 3:
        assert float(dwp[:, :, :7, 3].abs().max()) == 0.0, "gradient of the zero band"
    return _nchw(dw)


@pytest.mark.parametrize("n,bands,h,w,counts", BF16_WGRAD)
def test_stem_bf16_wgrad_exact(n, bands, h, w, counts):
    """x, dy in {-3..3} (bf16 values): |dW| <= 9 M < 2^24, so the fp32 accumulators, the partial tiles and their sum are exact."""
    _bf16_wgrad_case(n, h, w, counts)
    x, dy = _ints(-3, 3, n, bands, h, w, seed=161), _ints(-3, 3, n, 64, h // 2, w // 2, seed=162)
    ref = _wgrad_ref(x, dy)
    assert 9 * n * (h // 2) * (w // 2) < EXACT and float(ref.abs().max()) < EXACT
    assert torch.equal(_run_bf16_wgrad(x, dy, bands), ref)


@pytest.mark.parametrize("n,bands,h,w,counts", BF16_WGRAD)
def test_stem_bf16_wgrad_float64(n, bands, h, w, counts):
    """bf16-rounded Gaussian operands: the products are exact and the sums fp32, so the fp32 gradient's bound holds."""
    _bf16_wgrad_case(n, h, w, counts)
    x, dy = _q(_randn(n, bands, h, w, seed=171)), _q(_randn(n, 64, h // 2, w // 2, seed=172))
    _check_wgrad_float(_run_bf16_wgrad(x, dy, bands), x, dy, (n, h, w))


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(48, 64), (64, 48), (33, 64)])
def test_stem_bf16_refuses_sizes_that_are_no_multiple_of_32(h, w):
    from robosat_amd import ops

    x4 = torch.zeros(1, h, w, 4, device=DEV, dtype=BF)
    wp = torch.zeros(64, 7, 8, 4, device=DEV, dtype=BF)
    with pytest.raises(ValueError):
        ops.stem_conv_bf16(x4, wp)
    with pytest.raises(ValueError):
        ops.stem_conv_wgrad_bf16(torch.zeros(1, h // 2, w // 2, 64, device=DEV, dtype=BF), x4)


@pytest.mark.parametrize("out_hw", [(18, 23), (19, 22), (20, 23)])
def test_stem_f32_refuses_an_output_size_that_is_not_half_the_input(out_hw):
    from robosat_amd import ops

    x4 = torch.zeros(1, 37, 45, 4, device=DEV)  # (H + 1) / 2 = 19, (W + 1) / 2 = 23
    with pytest.raises(ValueError):
        ops.conv2d(x4, torch.zeros(64, 7, 8, 4, device=DEV), stride=2, pad=3, stem=7, out_hw=out_hw)
