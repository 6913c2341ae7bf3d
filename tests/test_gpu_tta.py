"""Dihedral test-time augmentation on the MI355X (csrc/tta.hip, UNet.predict_* ``tta=``): the fan-out and the merge against
torch restatements, bit for bit; the whole predict path against the same computation composed from the existing single-view
calls; exact equivariance under every element of each mode's group; the CPU oracle; and that ``tta="none"`` changes nothing."""

import numpy as np
import pytest
import torch

from oracle import robosat_ref as R, seeded
from robosat_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)


def view(t, op, dims):
    """torch restatement of view g_op (op = f + 2*k: flip left-right when f, then k counter-clockwise rot90s); dims = (H, W)."""

    if op & 1:
        t = torch.flip(t, dims=[dims[1]])
    return torch.rot90(t, (op >> 1) & 3, dims=list(dims))


def unview(t, op, dims):
    t = torch.rot90(t, -((op >> 1) & 3), dims=list(dims))
    if op & 1:
        t = torch.flip(t, dims=[dims[1]])
    return t


def views_u8(u8, op_list):
    """[N,H,W,C] uint8 -> [N*V,H,W,C], view v of tile n at n*V + v."""

    return torch.stack([view(u8, op, (1, 2)) for op in op_list], dim=1).flatten(0, 1).contiguous()


def merge_ref(probs, op_list):
    """The merge of the definition: inverse view, sort over the views, sequential fp32 sum from the smallest, times 1/V."""

    v = len(op_list)
    p = probs.view(-1, v, *probs.shape[1:])
    back = torch.stack([unview(p[:, i], op, (2, 3)) for i, op in enumerate(op_list)], dim=0)
    s = torch.sort(back, dim=0).values
    acc = s[0].clone()
    for i in range(1, v):
        acc = acc + s[i]
    return acc * (1.0 / v)


def quantize_ref(merged, overlap):
    """np.digitize of every foreground class over the crop: the layout of final_conv1x1_quantize."""

    m = merged.cpu().numpy()
    h, w = m.shape[2:]
    crop = m[:, 1:, overlap:h - overlap, overlap:w - overlap]
    q = np.digitize(crop, np.linspace(0, 1, 256)).astype(np.uint8)
    return q[:, 0] if m.shape[1] == 2 else np.ascontiguousarray(q.transpose(0, 2, 3, 1))


def argmax_ref(merged):
    return np.argmax(merged.cpu().numpy(), axis=1).astype(np.uint8)  # (numpy: first maximum)


def _net(classes, seed=7, dtype=torch.float32):
    from robosat_amd.unet import UNet

    net = UNet(classes, pretrained=False, compute_dtype=dtype)
    net.load_state_dict(seeded.seeded_state_dict(R.UNetRef(classes).state_dict(), seed))
    return net.to(DEV).eval()


def _u8(n, h, w, c=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8).to(DEV)


# ---- fan-out ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("hw,op_list", [((64, 64), list(range(8))), ((64, 64), [6, 3]), ((192, 256), [0, 1, 4, 5]),
                                        ((192, 256), [5, 0])])
def test_fan_out_u8_matches_transformed_tiles(c, hw, op_list):
    u8 = _u8(3, *hw, c=c, seed=c)
    mean, std = MEAN[:c], STD[:c]
    want = ops.u8_to_nhwc4_norm(views_u8(u8, op_list), mean, std)
    got = ops.tta_fan_out_u8(u8, mean, std, op_list)
    assert got.shape == want.shape and torch.equal(got, want)
    got16 = ops.tta_fan_out_u8(u8, mean, std, op_list, torch.bfloat16)
    assert got16.dtype == torch.bfloat16 and torch.equal(got16, want.to(torch.bfloat16))


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("hw,op_list", [((64, 64), list(range(8))), ((192, 256), [0, 1, 4, 5])])
def test_fan_out_f32_matches_transformed_images(c, hw, op_list):
    x = seeded.synthetic_images(2, c, *hw, seed=3).to(DEV)
    xv = torch.stack([view(x, op, (2, 3)) for op in op_list], dim=1).flatten(0, 1).contiguous()
    for dt in (torch.float32, torch.bfloat16):
        assert torch.equal(ops.tta_fan_out_f32(x, op_list, dt), ops.nchw_to_nhwc4(xv, dt))


def test_fan_out_refuses_rotations_off_the_square():
    u8 = _u8(1, 64, 96)
    with pytest.raises(ValueError):
        ops.tta_fan_out_u8(u8, MEAN[:3], STD[:3], [0, 2])
    with pytest.raises(ValueError):
        ops.tta_fan_out_u8(u8, MEAN[:3], STD[:3], [0, 1, 4])  # (V must be a power of two)


# ---- merge --------------------------------------------------------------------------------------------------------------------

def _probs(nv, c, h, w, seed):
    """Probabilities with exact ties across views and the edge values 0, 1 and the quantisation anchors."""

    g = torch.Generator().manual_seed(seed)
    p = torch.rand((nv, c, h, w), generator=g)
    coarse = torch.randint(0, 5, (nv, c, h, w), generator=g).float() / 4  # ties: 0, .25, .5, .75, 1
    pick = torch.rand((nv, c, h, w), generator=g) < 0.3
    p = torch.where(pick, coarse, p)
    p[:, :, :8, :8] = 1.0
    p[:, :, 8:16, :8] = 0.0
    p[:, :, 16:24, :8] = torch.from_numpy(np.linspace(0, 1, 256)[:64].astype(np.float32)).view(8, 8)
    p[:, :, 24:26, :8] = 1e-8
    return p.to(DEV)


@pytest.mark.parametrize("c", [2, 3, 5])
@pytest.mark.parametrize("op_list", [[0, 1], [0, 1, 4, 5], list(range(8)), [7, 2, 5, 0, 3, 6, 1, 4]])
def test_merge_matches_torch_restatement(c, op_list):
    hw = (96, 96) if any((op >> 1) & 1 for op in op_list) else (96, 128)
    n = 2
    probs = _probs(n * len(op_list), c, *hw, seed=c * 10 + len(op_list))
    merged = merge_ref(probs, op_list)
    got = ops.tta_merge(probs, op_list, "probs")
    assert got.shape == (n, c) + hw and torch.equal(got, merged)
    assert np.array_equal(ops.tta_merge(probs, op_list, "argmax").cpu().numpy(), argmax_ref(merged))
    for overlap in (0, 32):
        q = ops.tta_merge(probs, op_list, "quantize", overlap).cpu().numpy()
        want = quantize_ref(merged, overlap)
        assert q.shape == want.shape and np.array_equal(q, want), (overlap, int((q != want).sum()))


def test_merge_is_independent_of_view_order():
    op_list = list(range(8))
    probs = _probs(8, 3, 64, 64, seed=1)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    shuffled = probs[perm].contiguous()
    assert torch.equal(ops.tta_merge(probs, op_list, "probs"), ops.tta_merge(shuffled, [op_list[i] for i in perm], "probs"))


# ---- end to end ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("classes", [2, 3])
@pytest.mark.parametrize("mode", ["hflip", "flips", "d4"])
def test_predict_equals_composition_of_single_view_calls(dtype, classes, mode):
    net = _net(classes, 7, dtype)
    n, overlap = 2, 32
    u8 = _u8(n, 128, 128, seed=11)
    mean, std = MEAN[:3], STD[:3]
    op_list = ops.tta_ops(mode, 128, 128)
    with torch.no_grad():
        # the existing single-view device path on the torch-transformed views: u8 -> NHWC4 (-> bf16) -> softmax forward.  One
        # network batch of N*V views, as the TTA path runs them: the bf16 forward is not bit-independent of the batch SIZE
        x4 = ops.u8_to_nhwc4_norm(views_u8(u8, op_list), mean, std)
        if dtype == torch.bfloat16:
            x4 = x4.to(torch.bfloat16)
        probs = net._forward_eval(None, softmax=True, x4=x4)
    merged = merge_ref(probs, op_list)
    q = net.predict_quantized(u8, overlap=overlap, mean=mean, std=std, tta=mode).cpu().numpy()
    assert np.array_equal(q, quantize_ref(merged, overlap))
    cls = net.predict_classes(u8, mean=mean, std=std, tta=mode).cpu().numpy()
    assert np.array_equal(cls, argmax_ref(merged))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["hflip", "flips", "d4"])
def test_tta_is_exactly_equivariant(dtype, mode):
    """tta(g.x) == g.tta(x) bit for bit for every g of the mode's group; the plain forward of the same net is not equivariant."""

    net = _net(2, 5, dtype)
    overlap = 32
    u8 = _u8(2, 256, 256, seed=4)
    x = seeded.synthetic_images(1, 3, 256, 256, seed=9).to(DEV)
    q0 = net.predict_quantized(u8, overlap=overlap, tta=mode)
    c0 = net.predict_classes(u8, tta=mode)
    p0 = net.predict_probs(x, tta=mode)
    for g in ops.tta_ops(mode, 256, 256):
        ug = view(u8, g, (1, 2)).contiguous()
        assert torch.equal(net.predict_quantized(ug, overlap=overlap, tta=mode), view(q0, g, (1, 2))), g
        assert torch.equal(net.predict_classes(ug, tta=mode), view(c0, g, (1, 2))), g
        assert torch.equal(net.predict_probs(view(x, g, (2, 3)).contiguous(), tta=mode), view(p0, g, (2, 3))), g
    # teeth: without TTA the seeded net's output moves with the flip only approximately
    g = 1
    plain = net.predict_quantized(u8, overlap=overlap)
    assert not torch.equal(net.predict_quantized(view(u8, g, (1, 2)).contiguous(), overlap=overlap), view(plain, g, (1, 2)))
    pp = net.predict_probs(x)
    assert not torch.equal(net.predict_probs(view(x, g, (2, 3)).contiguous()), view(pp, g, (2, 3)))


def test_d4_probs_match_oracle():
    """fp32 d4 probabilities within the north-star 1e-3 of the CPU oracle's per-view softmax, inverse-transformed and averaged."""

    ref = R.UNetRef(2)
    sd = seeded.seeded_state_dict(ref.state_dict(), 13)
    ref.load_state_dict(sd)
    ref.eval()
    net = _net(2, 13)
    x = seeded.synthetic_images(1, 3, 256, 256, seed=2)
    op_list = list(range(8))
    xv = torch.cat([view(x, op, (2, 3)) for op in op_list], dim=0).contiguous()
    pv = R.predict_probs(ref, xv).double()
    want = torch.stack([unview(pv[i:i + 1], op, (2, 3)) for i, op in enumerate(op_list)]).mean(0)
    got = net.predict_probs(x.to(DEV), tta="d4").cpu().double()
    err = float((got - want).abs().max())
    print("d4 vs oracle max|dprob|", err)
    assert err <= 1e-3


# ---- unchanged behaviour --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tta_none_is_the_plain_path(dtype):
    net = _net(3, 3, dtype)
    u8 = _u8(2, 128, 128, seed=8)
    x = seeded.synthetic_images(2, 3, 128, 128, seed=8).to(DEV)
    assert torch.equal(net.predict_quantized(u8, overlap=16, tta="none"), net.predict_quantized(u8, overlap=16))
    assert torch.equal(net.predict_classes(u8, tta="none"), net.predict_classes(u8))
    assert torch.equal(net.predict_probs(x, tta="none"), net.predict_probs(x))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graph_replay_equals_eager(monkeypatch, dtype):
    net = _net(2, 21, dtype)
    u8 = _u8(2, 128, 128, seed=12)
    out = {}
    for graphs in ("0", "1"):
        monkeypatch.setenv("ROBOSAT_GRAPHS", graphs)
        out[graphs] = (net.predict_quantized(u8, overlap=32, tta="d4"), net.predict_classes(u8, tta="d4"))
        out[graphs + "again"] = (net.predict_quantized(u8, overlap=32, tta="d4"), net.predict_classes(u8, tta="d4"))
    for k in ("0again", "1", "1again"):
        assert torch.equal(out[k][0], out["0"][0]) and torch.equal(out[k][1], out["0"][1]), k


def test_d4_on_non_square_tiles_raises_before_any_launch():
    net = _net(2, 1)
    u8 = _u8(1, 192, 256)
    torch.cuda.synchronize()
    for call in (lambda: net.predict_quantized(u8, overlap=32, tta="d4"), lambda: net.predict_classes(u8, tta="d4"),
                 lambda: net.predict_probs(torch.zeros(1, 3, 192, 256, device=DEV), tta="d4")):
        with pytest.raises(ValueError, match="square"):
            call()
    assert not net.__dict__.get("_graphs")  # (nothing was captured either)
    with pytest.raises(ValueError, match="unknown TTA mode"):
        net.predict_classes(u8, tta="rot")
    # flips are fine off the square
    assert net.predict_quantized(u8, overlap=32, tta="flips").shape == (1, 128, 192)
