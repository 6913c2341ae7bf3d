"""Per-item state of the fp32 Winograd 3x3 kernels (conv_wino33_f32.hip): an item's (cout block, image, patch origin) is decoded once and
kept two deep (the fetch side runs an item ahead of the MFMAs), each thread's table rows and filter offsets once per block, the fused
head carries (image, row, column) and class loops of 2 / 4 / 8.  The shapes are the smallest at which that state can go wrong: three and
more items per block, the 128-tile block with its two sub-blocks in different images and a dead one at the end, ragged patches, every
class bucket and its boundary.  Each against F.conv2d in float64 on the CPU at the suite's fp32 bar (2e-5 of the reference's largest
element, as tests/test_gpu_wino_pipeline.py), against the generic kernel / the two-launch head where those can run, and against itself
on the first tile alone (bit for bit)."""

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
    print("{}: max err {:.3e} (bound {:.3e})".format(what, err, bound))
    assert err <= bound, (what, err, bound)


def _conv64(x, w):  # x [N,H,W,C], w [Cout,3,3,Cin] on the GPU -> float64 NCHW on the CPU
    return F.conv2d(x.double().cpu().permute(0, 3, 1, 2), w.double().cpu().permute(0, 3, 1, 2), padding=1)


def _layer(n, h, w, cin, cout, seed):
    g = _gen(seed)
    x = torch.randn(n, h, w, cin, device=DEV, generator=g)
    wk = torch.randn(cout, 3, 3, cin, device=DEV, generator=g) * (2.0 / (9 * cin)) ** 0.5
    return x, wk


# (n, h, w, cin, cout)
PLAIN = [
    (6, 64, 64, 32, 256),  # 768 items of two chunks on one block per CU: three per block, the two-deep state wraps
    (3, 16, 16, 32, 48),   # the 128 x 16 block: one patch per image, so an item's two sub-blocks lie in different images; the last one is dead
    (2, 17, 31, 48, 64),   # ragged patches (9 x 16 tiles), odd sizes: the last tile row / column hangs over the border; three chunks
    (2, 40, 24, 48, 64),   # ragged the other way (20 x 12 tiles)
]


@pytest.mark.parametrize("n,h,w,cin,cout", PLAIN)
def test_wino33_items_plain_vs_float64(n, h, w, cin, cout):
    from robosat_amd import ops

    x, wk = _layer(n, h, w, cin, cout, 81)
    assert ops.wino33_ok(x, cout)
    u = ops.pack_wino33_weight(wk)
    got = ops.conv2d_wino33(x, u)
    ref = _conv64(x, wk)
    _close(got.permute(0, 3, 1, 2), ref, "wino33 plain")
    if cin % 32 == 0 and cout % 32 == 0:
        generic = ops.conv2d(x, wk, pad=1)
        assert float((got - generic).abs().max()) <= 5e-5 * max(1.0, float(ref.abs().max()))  # (tests/test_gpu_tiles.py's bar for the pair)
    # batch independence: tile 0 alone (other items per block, other neighbours in the 128-tile block) is the same bits
    assert torch.equal(ops.conv2d_wino33(x[:1], u)[0], got[0])
    # ... and with the eval epilogue (scale / shift / ReLU read per item from the decoded cout block)
    g = _gen(82)
    sc, sh = torch.rand(cout, device=DEV, generator=g) + 0.5, torch.randn(cout, device=DEV, generator=g) * 0.3
    bn = ops.conv2d_wino33(x, u, scale=sc, shift=sh, relu=True)
    want = F.relu(ref * sc.double().cpu().view(1, -1, 1, 1) + sh.double().cpu().view(1, -1, 1, 1))
    _close(bn.permute(0, 3, 1, 2), want, "wino33 scale / shift / relu")


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 17, 31, 48, 64), (3, 16, 16, 32, 48)])
def test_wino33_items_stats_vs_float64(n, h, w, cin, cout):
    """Train-mode forward: the raw output (the plain kernel's bits) and the partial sums, one row per m block -- summed in fp32 over at
    most n h w values per cout, hence 1e-4 of the sum of magnitudes (n h w eps = 6e-5 at these sizes)."""
    from robosat_amd import ops

    x, wk = _layer(n, h, w, cin, cout, 83)
    u = ops.pack_wino33_weight(wk)
    out, part = ops.conv2d_wino33_bnstats(x, u)
    ref = _conv64(x, wk)
    _close(out.permute(0, 3, 1, 2), ref, "wino33 stats: output")
    assert torch.equal(out, ops.conv2d_wino33(x, u))
    s = part.double().cpu().sum(0)
    want0, want1 = ref.sum((0, 2, 3)), (ref * ref).sum((0, 2, 3))
    assert float((s[0] - want0).abs().max()) <= 1e-4 * float(ref.abs().sum((0, 2, 3)).max())
    assert float((s[1] - want1).abs().max()) <= 1e-4 * float(want1.max())


def test_wino33_items_data_gradient_float_and_bit_masks_vs_float64():
    """The data gradient on a ragged shape, ReLU mask as floats and as bits, with and without BatchNorm's partial sums."""
    from robosat_amd import ops

    n, h, w, cin, cout = 2, 17, 31, 64, 48  # forward layer cin -> cout: the gradient has cin channels, dy has cout
    g = _gen(84)
    y1 = torch.randn(n, h, w, cin, device=DEV, generator=g)
    wk = torch.randn(cout, 3, 3, cin, device=DEV, generator=g) * (2.0 / (9 * cin)) ** 0.5
    dy = torch.randn(n, h, w, cout, device=DEV, generator=g)
    y64 = y1.double().cpu()
    mean64 = y64.mean((0, 1, 2))
    invstd64 = 1 / torch.sqrt(y64.var((0, 1, 2), unbiased=False) + 1e-5)
    mean, invstd = mean64.float().to(DEV), invstd64.float().to(DEV)
    z, bits = ops.bn_apply(y1, invstd, -mean * invstd, relu=True, want_bits=True)
    xg = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xg, wk.double().cpu().permute(0, 3, 1, 2), padding=1) * dy.double().cpu().permute(0, 3, 1, 2)).sum().backward()
    keep = (z > 0).cpu().permute(0, 3, 1, 2)  # (the mask the kernel is given: the device's own ReLU)
    ref = xg.grad * keep
    u = ops.pack_wino33_weight(ops.pack_dgrad_weight(wk))
    assert ops.wino33_dgrad_ok(dy, cin)
    gf, pf = ops.conv2d_wino33_dgrad(dy, u, relu_mask=z, bn=(y1, mean, invstd))
    gb, pb = ops.conv2d_wino33_dgrad(dy, u, relu_mask_bits=bits, bn=(y1, mean, invstd))
    _close(gf.permute(0, 3, 1, 2), ref, "wino33 dgrad, float mask")
    assert torch.equal(gf, gb) and torch.equal(pf, pb)
    xhat = (y64 - mean.double().cpu()) * invstd.double().cpu()
    r = ref.permute(0, 2, 3, 1)
    s = pf.double().cpu().sum(0)
    mag = float(r.abs().sum((0, 1, 2)).max())
    assert float((s[0] - r.sum((0, 1, 2))).abs().max()) <= 1e-4 * mag
    assert float((s[1] - (r * xhat).sum((0, 1, 2))).abs().max()) <= 1e-4 * float((r * xhat).abs().sum((0, 1, 2)).max())
    g2, none = ops.conv2d_wino33_dgrad(dy, u, relu_mask_bits=bits)
    assert none is None and torch.equal(g2, gf)
    g3, _ = ops.conv2d_wino33_dgrad(dy, u)
    _close(g3.permute(0, 3, 1, 2), xg.grad, "wino33 dgrad, no mask")


def _head_case(n, h, w, classes, seed):
    g = _gen(seed)
    x = torch.randn(n, h, w, 32, device=DEV, generator=g)
    wk = torch.randn(32, 3, 3, 32, device=DEV, generator=g) * (2.0 / (9 * 32)) ** 0.5
    fw = torch.randn(classes, 32, device=DEV, generator=g) * 0.5
    fb = torch.randn(classes, device=DEV, generator=g) * 0.2
    return x, wk, fw, fb


def _check_head(n, h, w, classes, alone):
    from robosat_amd import ops

    x, wk, fw, fb = _head_case(n, h, w, classes, 85 + classes)
    assert ops.wino33_head_ok(x, 32, classes)
    u = ops.pack_wino33_weight(wk)
    ref = torch.einsum("nchw,kc->nkhw", F.relu(_conv64(x, wk)), fw.double().cpu()) + fb.double().cpu().view(1, -1, 1, 1)
    scale = max(1.0, float(ref.abs().max()))
    dec5 = ops.conv2d_wino33(x, u, relu=True)
    logits = ops.conv2d_wino33_head(x, u, fw, fb, "logits")
    two = ops.final_conv1x1(dec5, fw, fb)
    assert logits.shape == (n, classes, h, w)
    _close(logits, ref, "head logits, {} classes".format(classes))
    assert float((logits - two).abs().max()) <= 5e-6 * scale  # (summation order over the 32 channels: tests/test_gpu_tiles.py's bar)
    probs = ops.conv2d_wino33_head(x, u, fw, fb, "softmax")
    _close(probs, torch.softmax(ref, 1), "head softmax, {} classes".format(classes))
    assert float((probs - ops.final_conv1x1(dec5, fw, fb, softmax=True)).abs().max()) <= 5e-6
    if alone:
        assert torch.equal(ops.conv2d_wino33_head(x[:1], u, fw, fb, "softmax")[0], probs[0])
        assert torch.equal(ops.conv2d_wino33_head(x[:1], u, fw, fb, "logits")[0], logits[0])
    if classes < 2:
        return  # (quantised probabilities and class indices exist from two classes on)
    # argmax / quantised bytes against the two-launch path: equal except where the two paths' logits (5e-6 apart) straddle a tie or a
    # bin edge, as tests/test_gpu_tiles.py::test_fused_dec5_final_head_vs_two_launches holds them
    am, am2 = ops.conv2d_wino33_head(x, u, fw, fb, "argmax"), ops.final_conv1x1_argmax(dec5, fw, fb)
    top2 = torch.topk(two, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4 * scale
    assert am.shape == (n, h, w) and bool((am == am2)[clear].all()) and float(clear.float().mean()) > 0.99
    assert bool((am.cpu() == ref.argmax(1))[clear.cpu()].all())
    for ov in (0, 3):
        q, q2 = ops.conv2d_wino33_head(x, u, fw, fb, "quantize", overlap=ov), ops.final_conv1x1_quantize(dec5, fw, fb, ov)
        assert q.shape == q2.shape and q.dtype == torch.uint8
        diff = (q.int() - q2.int()).abs()
        diff = torch.minimum(diff, 256 - diff)  # (bin 256 wraps to 0)
        assert int(diff.max()) <= 1 and float((diff != 0).float().mean()) <= 2e-3
    if alone:
        assert torch.equal(ops.conv2d_wino33_head(x[:1], u, fw, fb, "argmax")[0], am[0])
        assert torch.equal(ops.conv2d_wino33_head(x[:1], u, fw, fb, "quantize", overlap=3)[0], q[0])


@pytest.mark.parametrize("h,w", [(32, 48), (17, 31)])
@pytest.mark.parametrize("classes", [1, 2, 3, 4, 5, 8])
def test_wino33_items_head_every_class_bucket(classes, h, w):
    """dec5 + final in one launch at 1, 2 (class loops of 2), 3, 4 (of 4), 5, 8 (of 8) classes, every output kind."""
    _check_head(2, h, w, classes, alone=True)


@pytest.mark.parametrize("n", [4, 5])
def test_wino33_items_head_full_grid(n):
    """128 x 128: 64 items per image.  n = 4 is one item for each of 256 CUs, n = 5 a second item on a quarter of the blocks (the head's
    second half then runs behind the next item's first barrier, with the next item's pixel already decoded)."""
    _check_head(n, 128, 128, 2, alone=False)
