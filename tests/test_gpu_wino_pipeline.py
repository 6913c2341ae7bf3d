"""The fp32 Winograd DecoderBlock kernel's chunk pipeline (conv_wino_f32.hip): a chunk's last position(s) run behind the barrier with the
NEXT chunk's patch reads and transform between their MFMAs, across item boundaries too.  These shapes aim at the pipeline's edges: two-chunk
items (every second "next chunk" is the next item's first), the concat source switch falling on the pipelined chunk, blocks with one and with
an odd number of items, ragged patches and the DG form's four-unit items.  The same edges for the 3x3 kernel's HEAD / STATS forms
(conv_wino33_f32.hip), whose LDS exchange is read behind the first barrier of the next item.  Each against a float64 reference, and where
the layout allows against the generic kernel and against itself at another batch size (bit for bit)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


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


# (n, c1, c2, cout, h, w): C1 + C2 = 32 -> nk = 2 (the smallest the geometry allows: the next item's table is built in an item's first
# chunk); c1 = 16, c2 = 16 -> the source switch is the second chunk, fetched under the first one's head and read in its tail
PHASE = [
    (2, 16, 16, 64, 16, 16),   # nk = 2, the switch on the pipelined chunk, one 8x8 patch per image
    (3, 32, 0, 64, 18, 22),    # nk = 2, one source, ragged patches (9 x 11 tiles)
    (2, 48, 16, 32, 16, 30),   # nk = 4, switch at the last chunk, 32-cout block (two patches per block)
    (8, 16, 16, 128, 64, 60),  # the 128 x 64 block, ragged last patch row, nk = 2
]


@pytest.mark.parametrize("n,c1,c2,cout,h,w", PHASE)
def test_wino_phase_pipeline_edges_vs_float64(n, c1, c2, cout, h, w):
    from robosat_amd import ops

    g = _gen(71)
    a = torch.randn(n, h, w, c1, device=DEV, generator=g)
    b = torch.randn(n, h, w, c2, device=DEV, generator=g) if c2 else None
    wk = torch.randn(cout, 3, 3, c1 + c2, device=DEV, generator=g) * (2.0 / (9 * (c1 + c2))) ** 0.5
    assert ops.wino_ok(a, b, cout, force=True)
    wp = ops.pack_phase_weight(wk)
    u = ops.pack_wino_phase_weight(wp)
    got = ops.conv2d_phase_wino(a, u, src2=b, relu=False)
    ref = _up_conv64(a if b is None else torch.cat([a, b], 3), wk)
    _close(got.permute(0, 3, 1, 2), ref, "wino phase")
    if c1 % 32 == 0 and c2 % 32 == 0:
        generic = ops.conv2d_phase(a, wp, src2=b)
        assert float((got - generic).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    # batch independence: the first image alone (one item per block, most blocks idle) is the same bits as inside the batch
    alone = ops.conv2d_phase_wino(a[:1], u, src2=None if b is None else b[:1], relu=False)
    assert torch.equal(alone[0], got[0])


@pytest.mark.parametrize("extra", [0, 1, 3])
def test_wino_phase_odd_item_counts_per_block(extra):
    """Work items = 4 parities x m blocks x cout blocks, dealt round-robin over one block per CU: a whole number of rounds plus 0, 1 or 3
    items, so some blocks run one item more than others and the last item's pipelined tail reads past the block's last chunk."""
    from robosat_amd import ops

    cus = _cus()
    g = _gen(72 + extra)
    # 16 x 16 sources = one 8x8 patch per image (one m block per image on the 64 x 64 block): items = 4 n
    n = (cus + 3) // 4 + extra  # items = 4 n: just past one item per CU
    a = torch.randn(n, 16, 16, 32, device=DEV, generator=g)
    wk = torch.randn(64, 3, 3, 32, device=DEV, generator=g) * 0.08
    u = ops.pack_wino_phase_weight(ops.pack_phase_weight(wk))
    got = ops.conv2d_phase_wino(a, u, relu=True)
    ref = F.relu(_up_conv64(a, wk))
    _close(got.permute(0, 3, 1, 2), ref, "wino phase, odd items")
    assert torch.equal(ops.conv2d_phase_wino(a[-1:], u, relu=True)[0], got[-1])


@pytest.mark.parametrize("n,c1,c2,cout,hs", [(2, 32, 32, 64, 16), (3, 64, 0, 32, 18)])
def test_wino_dgrad_four_unit_items_vs_float64(n, c1, c2, cout, hs):
    """The DG form: an output item is four units (parity planes of dz) accumulating into one tile; the pipeline carries the next unit's
    patch across each unit boundary.  cout = 32 here is dz's channel count: nk = 2 per unit."""
    from robosat_amd import ops

    assert ops.wino_dgrad_ok(n, hs, hs, c1, c2, cout)
    g = _gen(73)
    wk = torch.randn(cout, 3, 3, c1 + c2, device=DEV, generator=g) * 0.05
    dz = torch.randn(n, 2 * hs, 2 * hs, cout, device=DEV, generator=g)
    mask = torch.randn(n, hs, hs, c1 + c2, device=DEV, generator=g)
    u = ops.pack_wino_dgrad_weight(ops.pack_dgrad_phase_weight(wk))
    got, _ = ops.conv2d_dgrad_phase_wino(dz, u, c1, c2, mask1=mask)
    x = torch.zeros(n, c1 + c2, hs, hs, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wk.double().cpu().permute(0, 3, 1, 2), padding=1)
    (y * dz.double().cpu().permute(0, 3, 1, 2)).sum().backward()
    ref = x.grad * (mask.cpu().permute(0, 3, 1, 2) > 0)
    _close(got.permute(0, 3, 1, 2), ref, "wino dgrad")


def _conv64(x, w):
    return F.conv2d(x.double().cpu().permute(0, 3, 1, 2), w.double().cpu().permute(0, 3, 1, 2), padding=1)


@pytest.mark.parametrize("n,h,w", [(1, 16, 16), (3, 20, 36), (37, 16, 16)])
def test_wino33_head_pipeline_edges_vs_float64(n, h, w):
    """dec5 + final + softmax in one launch with two-chunk items (Cin = 32): the cg = 1 waves' partial logits are read behind the next
    item's first barrier.  One item (n = 1), ragged, and an odd count per block."""
    from robosat_amd import ops

    g = _gen(74)
    x = torch.randn(n, h, w, 32, device=DEV, generator=g)
    wk = torch.randn(32, 3, 3, 32, device=DEV, generator=g) * 0.08
    fw, fb = torch.randn(2, 32, device=DEV, generator=g) * 0.3, torch.randn(2, device=DEV, generator=g)
    assert ops.wino33_head_ok(x, 32, 2)
    u = ops.pack_wino33_weight(wk)
    got = ops.conv2d_wino33_head(x, u, fw, fb, mode="softmax")
    y = F.relu(_conv64(x, wk))
    logits = torch.einsum("nchw,kc->nkhw", y, fw.double().cpu()) + fb.double().cpu().view(1, -1, 1, 1)
    _close(got, torch.softmax(logits, 1), "wino33 head softmax", rel=1e-5)
    alone = ops.conv2d_wino33_head(x[:1], u, fw, fb, mode="softmax")
    assert torch.equal(alone[0], got[0])


@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 32, 64, 16, 16), (5, 48, 32, 15, 17), (33, 32, 32, 16, 16)])
def test_wino33_stats_pipeline_edges_vs_float64(n, cin, cout, h, w):
    """The train-mode forward: raw output + per-block partial sums exchanged through LDS behind the next item's first barrier."""
    from robosat_amd import ops

    g = _gen(75)
    x = torch.randn(n, h, w, cin, device=DEV, generator=g)
    wk = torch.randn(cout, 3, 3, cin, device=DEV, generator=g) * 0.08
    assert ops.wino33_ok(x, cout)
    u = ops.pack_wino33_weight(wk)
    out, part = ops.conv2d_wino33_bnstats(x, u)
    ref = _conv64(x, wk)
    _close(out.permute(0, 3, 1, 2), ref, "wino33 stats: output")
    s = part.double().cpu().sum(0)
    want0, want1 = ref.sum((0, 2, 3)), (ref * ref).sum((0, 2, 3))
    assert float((s[0] - want0).abs().max()) <= 1e-4 * float(ref.abs().sum((0, 2, 3)).max())
    assert float((s[1] - want1).abs().max()) <= 1e-4 * float(want1.max())
    plain = ops.conv2d_wino33(x, u)
    assert torch.equal(plain, out)  # (same MFMAs in the same order: only the epilogue differs)


def test_wino_pipeline_beside_an_lds_user():
    """The pipelined kernels twice on the same data, each time with LDS-DMA traffic of a neighbour on four side streams: bit for bit.
    (The positive control that shows such a neighbour exposes a missing wait on this box is tests/test_gpu_race_screen.py's.)"""
    from robosat_amd import ops

    g = _gen(76)
    sides = [torch.cuda.Stream() for _ in range(4)]
    nx = torch.randn(32, 64, 64, 256, device=DEV, generator=g).to(BF)
    nw = (torch.randn(64, 1, 1, 256, device=DEV, generator=g) * 0.05).to(BF)
    no = [torch.empty(32, 64, 64, 64, device=DEV, dtype=BF) for _ in range(4)]

    def neighbour():
        for side, o in zip(sides, no):
            with torch.cuda.stream(side):
                for _ in range(6):
                    ops.conv2d(nx, nw, out=o)

    a = torch.randn(4, 64, 64, 16, device=DEV, generator=g)
    b = torch.randn(4, 64, 64, 16, device=DEV, generator=g)
    up = ops.pack_wino_phase_weight(ops.pack_phase_weight(torch.randn(64, 3, 3, 32, device=DEV, generator=g) * 0.08))
    x = torch.randn(8, 64, 64, 32, device=DEV, generator=g)
    u3 = ops.pack_wino33_weight(torch.randn(32, 3, 3, 32, device=DEV, generator=g) * 0.08)
    fw, fb = torch.randn(2, 32, device=DEV, generator=g) * 0.3, torch.randn(2, device=DEV, generator=g)
    runs = [lambda: ops.conv2d_phase_wino(a, up, src2=b, relu=True),
            lambda: ops.conv2d_wino33(x, u3, relu=True),
            lambda: ops.conv2d_wino33_head(x, u3, fw, fb, mode="softmax"),
            lambda: ops.conv2d_wino33_bnstats(x, u3)]
    bad = []
    for r in range(20):
        for i, fn in enumerate(runs):
            torch.cuda.synchronize()
            neighbour()
            one = fn()
            neighbour()
            two = fn()
            one, two = (one if isinstance(one, tuple) else (one,)), (two if isinstance(two, tuple) else (two,))
            if not all(torch.equal(p, q) for p, q in zip(one, two)):
                bad.append((r, i))
    torch.cuda.synchronize()
    assert not bad, bad
