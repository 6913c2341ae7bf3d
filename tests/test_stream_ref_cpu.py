"""The float64 references of the streaming-kernel tests (tests/stream_ref.py) checked on the CPU: each one against torch's
own float64 operator and autograd at two or three shapes (N > 1, non-square), the inputs of the quantise and argmax GPU tests
against their caps on the reference alone, and the comparison against planted errors -- one dropped pixel in dW, a tap index
off by one, a running_var updated with the biased variance, one flipped mask bit.  The last test prints how far torch's fp32
CPU evaluation lies from the float64 reference in the units of ``compare``: what rounding alone costs under each bar."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_ref as S

EXACT = 1e-12  # float64 against float64, in units of the element's scale


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- the references against torch -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,h,w,cin,c", [(3, 7, 9, 32, 2), (2, 17, 31, 8, 5), (1, 5, 4, 128, 8)])
def test_head_forward_is_conv2d_and_softmax(n, h, w, cin, c):
    x, wt, b = S.head_case(n, h, w, cin, c, seed=1, plant=120.0)
    ref = S.head_fwd(x, wt, b)
    logits = F.conv2d(nchw(x.double()), wt.double().view(c, cin, 1, 1), b.double())
    assert S.distance(ref["logits"], logits, ref["logit_scale"]) <= EXACT
    assert S.distance(ref["probs"], F.softmax(logits, 1), ref["prob_scale"]) <= EXACT
    assert torch.equal(ref["argmax"].long(), torch.argmax(logits, 1))
    assert bool((ref["logit_scale"] >= ref["logits"].abs() * (1 - 1e-12)).all())
    if c > 1:  # the planted pixels: probability exactly 1.0 and below the smallest fp32 number, in float64 too
        hot, cold = ref["probs"][0, :, h // 2, w // 2], ref["probs"][0, :, h // 2, w // 2 - 1]
        assert float(hot[c - 1]) == 1.0 and 0 < float(hot[0]) < 1e-46 and float(cold[0]) == 1.0 and 0 < float(cold[c - 1]) < 1e-46


@pytest.mark.parametrize("c,overlap", [(2, 0), (2, 3), (3, 1), (5, 2)])
def test_quantize_is_predict_py(c, overlap):
    """tools/predict.py: probs[overlap:-overlap, overlap:-overlap] per image, then digitize of each foreground class."""

    x, wt, b = S.head_case(3, 7, 9, 32, c, seed=2, wscale=0.1, plant=120.0)
    ref = S.head_fwd(x, wt, b)
    q, bins, p, near = S.head_quantize(ref["probs"], overlap)
    anchors = np.linspace(0, 1, 256)
    assert q.dtype == np.uint8 and q.shape == (3, 7 - 2 * overlap, 9 - 2 * overlap) + ((c - 1,) if c > 2 else ())
    for i in range(3):
        for k in range(1, c):
            plane = ref["probs"][i, k].numpy()
            crop = plane[overlap:7 - overlap, overlap:9 - overlap]
            want = np.digitize(crop, anchors).astype(np.uint8)
            assert np.array_equal(q[i] if c == 2 else q[i, :, :, k - 1], want)
    if overlap <= 3:  # the planted pixels are inside every crop: bin 256 wraps to byte 0, probability ~ 0 is byte 1
        flat = q.reshape(3, 7 - 2 * overlap, 9 - 2 * overlap, c - 1)
        assert flat[0, 3 - overlap, 4 - overlap, c - 2] == 0 and bins[0, 3 - overlap, 4 - overlap, c - 2] == 256
        assert flat[0, 3 - overlap, 3 - overlap, c - 2] == 1
    assert S.max_overlap(7, 9) == 3 and S.max_overlap(17, 31) == 8


@pytest.mark.parametrize("n,h,w,cin,c,relu_mask", [(3, 7, 9, 32, 2, True), (2, 17, 31, 16, 5, False), (2, 6, 5, 64, 8, True)])
def test_head_backward_is_autograd(n, h, w, cin, c, relu_mask):
    x, wt, _ = S.head_case(n, h, w, cin, c, seed=3, relu=True)
    dl = torch.randn(n, c, h, w, generator=S.gen(4))
    pre = nchw(x.double()).clone()
    pre[pre == 0] = -1.0  # x = relu(pre)
    pre.requires_grad_(True)
    w64 = wt.double().view(c, cin, 1, 1).requires_grad_(True)
    b64 = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    act = F.relu(pre)
    act.retain_grad()
    F.conv2d(act, w64, b64).backward(dl.double())
    ref = S.head_bwd(x, wt, dl, relu_mask)
    assert S.distance(ref["dx"], nhwc(pre.grad if relu_mask else act.grad), ref["dx_scale"] + S.TINY) <= EXACT
    assert S.distance(ref["dW"], w64.grad.view(c, cin), ref["dW_scale"]) <= EXACT
    assert S.distance(ref["db"], b64.grad, ref["db_scale"]) <= EXACT
    assert bool((x == 0).any())
    if relu_mask:
        assert float(ref["dx"][x == 0].abs().max()) == 0.0 and float(ref["dx_scale"][x == 0].abs().max()) == 0.0


def _taps_from_indices(idx, h, w, k, s, p):
    """torch's flat input index of the winner -> the tap r * k + t in window coordinates (NCHW)."""

    ho, wo = idx.shape[2:]
    oy = torch.arange(ho).view(1, 1, ho, 1)
    ox = torch.arange(wo).view(1, 1, 1, wo)
    return (idx // w - (oy * s - p)) * k + (idx % w - (ox * s - p))


@pytest.mark.parametrize("n,h,w,c,k,s,p", [(n, h, w, c, k, s, p) for (k, s, p) in S.POOL_PARAMS
                                           for (n, h, w, c) in [(2, 17, 23, 4), (3, 14, 19, 8), (2, 2, 3, 4), (2, 1, 1, 4)]
                                           if S.pool_out(h, k, s, p) >= 1 and S.pool_out(w, k, s, p) >= 1])
def test_maxpool_is_torch_with_indices(n, h, w, c, k, s, p):
    """Values and taps against F.max_pool2d(return_indices=True) on inputs with exact ties, all-equal windows, -inf and NaN
    (first / middle / last tap, and two in one window); the gradient against autograd.  (1 x 1 under a 2 x 2 window has no
    output: torch refuses it too.)"""

    x = S.pool_input(n, h, w, c, seed=5)
    xt = nchw(x.double()).requires_grad_(True)
    want, idx = F.max_pool2d(xt, k, s, p, return_indices=True)
    value, tap = S.maxpool_fwd(x, k, s, p)
    assert torch.equal(torch.isnan(value), torch.isnan(nhwc(want.detach())))
    assert torch.equal(torch.nan_to_num(value, nan=7.0), torch.nan_to_num(nhwc(want.detach()), nan=7.0))
    assert torch.equal(tap, nhwc(_taps_from_indices(idx, h, w, k, s, p)))
    if h >= 12:
        assert bool(torch.isnan(value).any()) and bool((value == float("-inf")).any())
        taps_of_nan = set(tap[torch.isnan(value)].tolist())
        assert {0, k * k - 1} <= taps_of_nan  # a NaN that won as the first tap of a window and one as the last
    dy = torch.round(torch.randn(value.shape, generator=S.gen(6)) * 8) / 8
    want.backward(nchw(dy.double()))
    base = torch.randn(n, h, w, c, generator=S.gen(7))
    dx, sc, cnt = S.maxpool_bwd(dy, tap, (n, h, w, c), k, s, p)
    assert torch.equal(dx, nhwc(xt.grad))
    dx2, sc2, _ = S.maxpool_bwd(dy, tap, (n, h, w, c), k, s, p, base=base)
    assert torch.equal(dx2, dx + base.double()) and torch.equal(sc2, sc + base.double().abs())
    assert int(cnt.sum()) == value.numel() and bool((sc >= dx.abs()).all())
    if (k, s, p) == (2, 2, 0):
        assert int(cnt.max()) == 1  # disjoint windows
    elif h >= 12:
        assert int(cnt.max()) > 1


@pytest.mark.parametrize("n,h,w,c1,c2", [(3, 5, 7, 4, 0), (2, 3, 2, 12, 20), (1, 4, 6, 64, 32)])
def test_upsample_split_is_autograd(n, h, w, c1, c2):
    g = S.gen(8)
    a_pre = torch.randn(n, c1, h, w, generator=g, dtype=torch.float64).requires_grad_(True)
    b_pre = torch.randn(n, max(c2, 1), h, w, generator=g, dtype=torch.float64).requires_grad_(True)
    a, b = F.relu(a_pre), F.relu(b_pre)
    a.retain_grad()
    b.retain_grad()
    cat = torch.cat([a, b], 1) if c2 else a
    cat.retain_grad()
    up = F.interpolate(cat, scale_factor=2, mode="nearest")
    dup = torch.randn(up.shape, generator=g, dtype=torch.float64)
    up.backward(dup)
    base = torch.randn(n, h, w, c1, generator=g)
    m1, m2 = nhwc(a.detach()), nhwc(b.detach()) if c2 else None
    d1, s1, d2, s2 = S.upsample_split_bwd(nhwc(dup), c1, c2)
    assert S.distance(d1, nhwc(a.grad), s1) <= EXACT and (not c2 or S.distance(d2, nhwc(b.grad), s2) <= EXACT)
    d1, s1, d2, s2 = S.upsample_split_bwd(nhwc(dup), c1, c2, mask1=m1, mask2=m2, base1=base)
    assert S.distance(d1, nhwc(a_pre.grad) + base.double(), s1 + S.TINY) <= EXACT
    assert not c2 or S.distance(d2, nhwc(b_pre.grad), s2 + S.TINY) <= EXACT
    # the no-sum form: the split of the cat alone
    e1, t1, e2, t2 = S.upsample_split_bwd(nhwc(cat.grad), c1, c2, mask1=m1, summed=False)
    assert torch.equal(e1, nhwc(a_pre.grad)) and (not c2 or torch.equal(e2, nhwc(b.grad)))


@pytest.mark.parametrize("hs,ws,ho,wo", [(3, 4, 6, 8), (3, 4, 5, 7), (2, 5, 4, 9)])
def test_scatter_is_the_gradient_of_a_strided_slice(hs, ws, ho, wo):
    g = S.gen(9)
    t = torch.randn(2, hs, ws, 4, generator=g)
    out = torch.randn(2, ho, wo, 4, generator=g)
    src = out.double().clone().requires_grad_(True)
    src[:, ::2, ::2].backward(t.double())
    assert src[:, ::2, ::2].shape[1:3] == (hs, ws)
    got, touched = S.scatter_add_stride2(t, out)
    assert torch.equal(got, out.double() + src.grad) and int(touched.sum()) == t.numel()
    assert torch.equal(got[~touched], out.double()[~touched])


@pytest.mark.parametrize("n,h,w,c,res,relu", [(2, 3, 5, 8, True, True), (3, 2, 2, 12, False, True), (1, 2, 1, 4, True, False)])
def test_batchnorm_is_torch_batch_norm(n, h, w, c, res, relu):
    m = n * h * w
    y, gamma, beta, rm, rv = S.bn_input(m, c, seed=10, offset=0.5)
    y = y.view(n, h, w, c)
    g = S.gen(11)
    resid = torch.randn(n, h, w, c, generator=g) if res else None
    dz = torch.randn(n, h, w, c, generator=g)
    yt = nchw(y.double()).requires_grad_(True)
    gt, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rt = nchw(resid.double()).requires_grad_(True) if res else None
    rmt, rvt = rm.double().clone(), rv.double().clone()
    z = F.batch_norm(yt, rmt, rvt, gt, bt, training=True, momentum=0.1, eps=1e-5)
    if res:
        z = z + rt
    if relu:
        z = F.relu(z)
    z.backward(nchw(dz.double()))
    st = S.bn_stats(y, gamma, beta, 1e-5, 0.1, rm, rv)
    assert S.distance(st["running_mean"], rmt, st["running_mean_scale"]) <= EXACT
    assert S.distance(st["running_var"], rvt, st["running_var_scale"]) <= EXACT
    assert S.distance(st["var"], nchw(y.double()).var((0, 2, 3), unbiased=False), st["var"]) <= 1e-10
    zr, zs = S.bn_apply(y, st["scale"], st["shift"], resid, relu)
    assert S.distance(zr, nhwc(z.detach()), zs) <= EXACT
    bw = S.bn_bwd(dz, zr if relu else None, y, gamma, 1e-5)
    assert S.distance(bw["dy"], nhwc(yt.grad), bw["dy_scale"]) <= 1e-10
    assert S.distance(bw["dgamma"], gt.grad, bw["dgamma_scale"]) <= 1e-10
    assert S.distance(bw["dbeta"], bt.grad, bw["dbeta_scale"]) <= EXACT
    if res:
        assert torch.equal(bw["dmasked"], nhwc(rt.grad))
    same = S.bn_bwd(dz, zr if relu else None, y, gamma, 1e-5, mean=st["mean"], invstd=st["invstd"])
    assert torch.equal(same["dy"], bw["dy"])
    bits = S.mask_bits(zr)
    flat = (zr.reshape(-1) > 0)
    assert bits.numel() == flat.numel() // 8 and all(bool(bits[i // 8] >> (i % 8) & 1) == bool(flat[i]) for i in range(0, flat.numel(), 7))


def test_bf16_ulp_and_rounded_compare():
    v = torch.tensor([1.0, 1.5, -3.0, 0.0, 2.0 ** -20, 255.0], dtype=torch.float64)
    assert S.bf16_ulp(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.0, 2.0 ** -27, 1.0]
    want = torch.tensor([1.0 + 2.0 ** -8 - 1e-9, 0.0], dtype=torch.float64)  # just below the midpoint of 1 and 1 + 2^-7
    up, down = torch.tensor([1.0 + 2.0 ** -7, 0.0]).to(S.BF16), torch.tensor([1.0, 0.0]).to(S.BF16)
    assert S.distance(up, want, want.abs(), bf16=True) == 0.0 and S.distance(down, want, want.abs(), bf16=True) == 0.0
    two = torch.tensor([1.0 + 2.0 ** -6, 0.0]).to(S.BF16)
    assert S.distance(two, want, want.abs(), bf16=True) > 1e-3  # two ulps off
    assert S.distance(torch.tensor([1.0, 2.0 ** -60]).to(S.BF16), want, want.abs(), bf16=True) > 1.0  # an exact 0 has no allowance


# ---- the caps of the quantise and argmax inputs, on the reference alone ---------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cin", S.QUANT_CIN)
def test_quantize_inputs_stay_under_the_cap(cin, bf16):
    """At most 0.5 % of the bytes one quantise test compares lie within the probability bar of an anchor."""

    total = near_anchor = 0
    for x, wt, b, ov in S.quantize_cases(cin, bf16):
        ref = S.head_fwd(x, wt, b)
        q, _, _, _ = S.head_quantize(ref["probs"], ov)
        n, differ, allowed = S.quantize_check(q, ref["probs"], ref["prob_scale"], ov, S.head_bars(cin)[1])
        assert differ == 0
        total, near_anchor = total + n, near_anchor + allowed
    print("quantise Cin={} {}: {} of {} bytes within the bar of an anchor ({:.3%})".format(cin, "bf16" if bf16 else "fp32", near_anchor, total, near_anchor / total))
    assert total > 10000 and near_anchor <= 0.005 * total


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cin", S.QUANT_CIN)
def test_argmax_inputs_stay_under_the_cap(cin, bf16):
    total = close = 0
    for x, wt, b in S.argmax_cases(cin, bf16):
        ref = S.head_fwd(x, wt, b)
        n, differ, allowed = S.argmax_check(ref["argmax"].numpy(), ref["logits"], ref["logit_scale"], S.head_bars(cin)[0])
        assert differ == 0
        total, close = total + n, close + allowed
    print("argmax Cin={}: {} of {} pixels with the two largest logits within the bar ({:.3%})".format(cin, close, total, close / total))
    assert total > 4000 and close <= 0.005 * total


def test_tie_case_ties_on_the_float64_reference():
    for c in (2, 3, 8):
        x, wt, b, lo = S.tie_case(3, 7, 9, 32, c, seed=12)
        ref = S.head_fwd(x, wt, b)
        assert torch.equal(ref["logits"][:, lo], ref["logits"][:, lo + 1])
        am = ref["argmax"]
        assert int((am == lo).sum()) > am.numel() // 4 and int((am == lo + 1).sum()) == 0


def test_quantize_and_argmax_checks_reject_wrong_bytes():
    x, wt, b = S.head_case(3, 7, 9, 32, 3, seed=13, wscale=0.1)
    ref = S.head_fwd(x, wt, b)
    q = S.head_quantize(ref["probs"], 1)[0]
    for delta in (1, 2):  # off by one bin where no anchor is near; off by two anywhere
        bad = q.copy()
        bad[1, 2, 3, 0] += delta
        with pytest.raises(AssertionError):
            S.quantize_check(bad, ref["probs"], ref["prob_scale"], 1, S.head_bars(32)[1])
    # Himg and Wimg swapped in the crop of a non-square tile: the bytes of another pixel
    swapped = S.head_quantize(ref["probs"].transpose(2, 3).contiguous(), 1)[0].reshape(q.shape)
    with pytest.raises(AssertionError):
        S.quantize_check(swapped, ref["probs"], ref["prob_scale"], 1, S.head_bars(32)[1])
    am = ref["argmax"].numpy().copy()
    am[0, 0, 0] = (am[0, 0, 0] + 1) % 3
    with pytest.raises(AssertionError):
        S.argmax_check(am, ref["logits"], ref["logit_scale"], S.head_bars(32)[0])


# ---- planted errors -------------------------------------------------------------------------------------------------------

def test_compare_rejects_one_dropped_pixel_in_dw():
    x, wt, _ = S.head_case(2, 17, 31, 32, 2, seed=14, relu=True)
    dl = torch.randn(2, 2, 17, 31, generator=S.gen(15))
    ref = S.head_bwd(x, wt, dl, True)
    S.compare("head dW", ref["dW"].float(), ref["dW"], ref["dW_scale"])  # fp32 rounding of the right answer passes
    short = dl.clone()
    short[1, :, 16, 30] = 0  # the last pixel does not reach the sums
    bad = S.head_bwd(x, wt, short, True)
    with pytest.raises(AssertionError):
        S.compare("head dW", bad["dW"].float(), ref["dW"], ref["dW_scale"])
    with pytest.raises(AssertionError):
        S.compare("head db", bad["db"].float(), ref["db"], ref["db_scale"])
    # an element that must be exactly 0 (masked) and is not -- however small next to the largest entry of the tensor
    leak = ref["dx"].clone()
    where = (x == 0).nonzero()[0]
    leak[tuple(where)] = 1e-12
    with pytest.raises(AssertionError):
        S.compare("head dx", leak, ref["dx"], ref["dx_scale"])


def test_compare_rejects_a_tap_off_by_one():
    x = S.pool_input(2, 17, 23, 4, seed=16, special=False)
    value, tap = S.maxpool_fwd(x, 3, 2, 1)
    dy = torch.randn(value.shape, generator=S.gen(17))
    dx, sc, _ = S.maxpool_bwd(dy, tap, x.shape, 3, 2, 1)
    wrong = tap.clone()
    wrong[1, 4, 5, 2] += 1 if int(wrong[1, 4, 5, 2]) % 3 < 2 else -1
    assert not torch.equal(wrong, tap)
    bad, _, _ = S.maxpool_bwd(dy, wrong, x.shape, 3, 2, 1)
    S.compare("pool grad", dx.float(), dx, sc)
    with pytest.raises(AssertionError):
        S.compare("pool grad", bad.float(), dx, sc)


@pytest.mark.parametrize("k,s,p", S.POOL_PARAMS)
@pytest.mark.parametrize("c", [4, 12, 8, 64])
def test_pool_inputs_tell_the_first_maximum_from_the_last(c, k, s, p):
    """The GPU tests' 17 x 23 inputs have ties in many windows: a scan with ``>=`` (the last maximum wins) records other taps."""

    x = S.pool_input(2, 17, 23, c, seed=900 + c)
    _, tap = S.maxpool_fwd(x, k, s, p)
    taps, valid = S._windows(torch.nan_to_num(x, nan=-1.0), k, s, p)
    v = valid.view(k * k, 1, tap.shape[1], tap.shape[2], 1).expand_as(taps)
    order = torch.arange(k * k).view(-1, 1, 1, 1, 1).expand_as(taps)
    best = torch.where(v, taps, torch.full_like(taps, float("-inf"))).max(0).values
    last = torch.where((taps == best) & v, order, torch.full_like(order, -1)).max(0).values
    assert int((last != tap).sum()) > tap.numel() // 20


@pytest.mark.parametrize("m", [8, 65 * 65])
def test_compare_rejects_a_running_var_from_the_biased_variance(m):
    y, gamma, beta, rm, rv = S.bn_input(m, 8, seed=18)
    st = S.bn_stats(y, gamma, beta, 1e-5, 0.1, rm, rv)
    S.compare("running_var", st["running_var"].float(), st["running_var"], st["running_var_scale"])
    biased = 0.9 * rv.double() + 0.1 * st["var"]
    with pytest.raises(AssertionError):
        S.compare("running_var", biased.float(), st["running_var"], st["running_var_scale"])


def test_compare_rejects_fp32_one_pass_statistics_under_cancellation():
    """y = 100 + 0.01 randn: E[y^2] - mean^2 from fp32 sums is off by several variances; the invstd bar sees it."""

    y, gamma, beta, rm, rv = S.bn_input(65 * 65, 64, seed=1260, offset=100.0, spread=0.01)
    st = S.bn_stats(y, gamma, beta, 1e-5, 0.1, rm, rv)
    assert 5e-5 < float(st["var"].min()) and float(st["var"].max()) < 2e-4
    S.compare("bn invstd", st["invstd"].float(), st["invstd"], st["invstd_scale"])
    m = y.shape[0]
    mu = y.sum(0) / m
    var32 = ((y * y).sum(0) / m - mu * mu).clamp_min(0)  # fp32 throughout
    with pytest.raises(AssertionError):
        S.compare("bn invstd", 1 / torch.sqrt(var32 + 1e-5), st["invstd"], st["invstd_scale"])


def test_one_flipped_mask_bit_is_seen():
    z = torch.randn(4, 64, generator=S.gen(19), dtype=torch.float64)
    bits = S.mask_bits(z)
    flipped = bits.clone()
    flipped[17] ^= 1 << 5
    assert torch.equal(bits, S.mask_bits(z)) and not torch.equal(flipped, bits)
    assert int((np.unpackbits(flipped.numpy(), bitorder="little") != (z.reshape(-1) > 0).numpy()).sum()) == 1


def test_compare_fails_on_nan_and_wrong_small_elements():
    want = torch.tensor([1000.0, 1e-3], dtype=torch.float64)
    S.compare("logits", want.float(), want, want.abs())
    with pytest.raises(AssertionError):
        S.compare("logits", torch.tensor([1000.0, float("nan")]), want, want.abs())
    # 2e-3 instead of 1e-3: 1e-6 of the largest entry (a max-norm bar of 1e-5 passes it), 100 % of its own scale
    with pytest.raises(AssertionError):
        S.compare("logits", torch.tensor([1000.0, 2e-3]), want, want.abs())


# ---- what rounding alone costs --------------------------------------------------------------------------------------------

def test_fp32_torch_against_the_float64_reference():
    """torch's fp32 CPU operators on the GPU tests' inputs, in the units of ``compare`` and under the project's limits: the
    figures the docstring of tests/test_gpu_streaming.py quotes next to the device's.  (torch normalises as (y - mean) * invstd
    * gamma + beta, the kernels as y * scale + shift: different roundings, both far below the limit.)"""

    rec = {}
    for cin, c in ((32, 2), (128, 8), (64, 5)):
        x, wt, b = S.head_case(2, 17, 31, cin, c, seed=20, relu=True, plant=120.0)
        ref = S.head_fwd(x, wt, b)
        logits = F.conv2d(nchw(x), wt.view(c, cin, 1, 1), b)
        S.compare("logits", logits, ref["logits"], ref["logit_scale"], "torch fp32", rec, bar=S.LIMITS["logits"])
        S.compare("probs", F.softmax(logits, 1), ref["probs"], ref["prob_scale"], "torch fp32", rec, bar=S.LIMITS["probs"])
        if cin <= 64:
            dl = torch.randn(2, c, 17, 31, generator=S.gen(21))
            xt, wtt, bt = nchw(x).requires_grad_(True), wt.view(c, cin, 1, 1).clone().requires_grad_(True), b.clone().requires_grad_(True)
            F.conv2d(xt, wtt, bt).backward(dl)
            bw = S.head_bwd(x, wt, dl, False)
            S.compare("head dx", nhwc(xt.grad), bw["dx"], bw["dx_scale"], "torch fp32", rec, bar=S.LIMITS["head dx"])
            S.compare("head dW", wtt.grad.view(c, cin), bw["dW"], bw["dW_scale"], "torch fp32", rec, bar=S.LIMITS["head dW"])
            S.compare("head db", bt.grad, bw["db"], bw["db_scale"], "torch fp32", rec, bar=S.LIMITS["head db"])
    for m, c, offset, spread in ((65 * 65, 64, 0.5, 1.0), (513, 12, 0.5, 1.0)):
        y, gamma, beta, rm, rv = S.bn_input(m, c, seed=22, offset=offset, spread=spread)
        y4 = y.view(1, m, 1, c)
        yt, gt, bt = nchw(y4).requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        rmt, rvt = rm.clone(), rv.clone()
        z = F.relu(F.batch_norm(yt, rmt, rvt, gt, bt, training=True, momentum=0.1, eps=1e-5))
        dz = torch.randn(1, m, 1, c, generator=S.gen(23))
        z.backward(nchw(dz))
        st = S.bn_stats(y, gamma, beta, 1e-5, 0.1, rm, rv)
        S.compare("running_mean", rmt, st["running_mean"], st["running_mean_scale"], "torch fp32", rec, bar=S.LIMITS["running_mean"])
        S.compare("running_var", rvt, st["running_var"], st["running_var_scale"], "torch fp32", rec, bar=S.LIMITS["running_var"])
        zr, zs = S.bn_apply(y4, st["scale"], st["shift"], None, True)
        S.compare("bn z", nhwc(z.detach()), zr, zs, "torch fp32", rec, bar=S.LIMITS["bn z"])
        bw = S.bn_bwd(dz, zr, y4, gamma, 1e-5)
        S.compare("bn dy", nhwc(yt.grad), bw["dy"], bw["dy_scale"], "torch fp32", rec, bar=S.LIMITS["bn dy"])
        S.compare("bn dgamma", gt.grad, bw["dgamma"], bw["dgamma_scale"], "torch fp32", rec, bar=S.LIMITS["bn dgamma"])
        S.compare("bn dbeta", bt.grad, bw["dbeta"], bw["dbeta_scale"], "torch fp32", rec, bar=S.LIMITS["bn dbeta"])
    for name, d in sorted(rec.items()):
        print("torch fp32 against float64, {}: {:.2e} (limit {:.0e}, bar {:.0e})".format(name, d, S.LIMITS[name], S.BARS[name]))


# ---- host side ------------------------------------------------------------------------------------------------------------

def test_batchnorm_workspace_query_at_every_vector_width():
    """rs_bn_workspace_bytes is pure host arithmetic: C = 4 has no 8-channel geometry (the query used to divide by zero there
    and take the process down), C = 12 only a 4-channel one; the answer covers the row splits of whichever kernel runs."""

    import os

    from robosat_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librobosat_hip.so not built (run __graft_entry__.build())")
    lib = _lib.lib()
    for c in (4, 8, 12, 16, 36, 64, 320, 2048, 4096):
        assert lib.rs_bn_workspace_bytes(2, c) == 2 * c * 8  # one row split: [2][C] doubles
    # M = 4225, C = 64: 32 row lanes of >= 64 rows make two splits at 8 channels per thread, 16 lanes make four at 4: the larger
    assert lib.rs_bn_workspace_bytes(65 * 65, 64) == 4 * 2 * 64 * 8
    assert lib.rs_bn_workspace_bytes(65 * 65, 4) == 2 * 4 * 8 and lib.rs_bn_workspace_bytes(256 * 64 * 3, 4) == 3 * 2 * 4 * 8
    for m, c in ((0, 4), (2, 0), (2, 6)):
        assert lib.rs_bn_workspace_bytes(m, c) == _lib.RS_EINVAL
