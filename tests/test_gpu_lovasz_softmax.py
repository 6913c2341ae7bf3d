"""Lovasz-Softmax on the MI355X (``rs_lovasz_softmax_fwd``, ``LovaszSoftmax2d``) against the float64 restatement of the paper
in ``lovasz_softmax_ref``: at small shapes from the logits alone, at real sizes from the kernel's own fp32 probabilities (same
keys, same tie order), and against 1 - mean IoU at hard predictions, which needs no sort at all."""

import pytest
import torch

import lovasz_hinge_ref
import lovasz_softmax_ref as ref
from robosat_amd import ops
from robosat_amd.losses import LovaszSoftmax2d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (N, C, H, W): N * H * W within what separated_inputs can space 1 / 90000 apart for C classes
SMALL = [(1, 2, 64, 64), (3, 2, 64, 64), (1, 3, 32, 32), (3, 3, 48, 48), (1, 5, 32, 32), (3, 5, 24, 24), (3, 3, 15, 17)]


def _run(x, y, per_image, classes, want_probs=False):
    loss, grad, probs = ops.lovasz_softmax_fwd(x.to(DEV), y.to(DEV), per_image=per_image, classes=classes, want_probs=want_probs)
    torch.cuda.synchronize()
    return float(loss), grad.cpu(), (probs.cpu() if probs is not None else None)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("per_image", [True, False])
@pytest.mark.parametrize("classes", ["present", "all"])
def test_vs_float64_truth_from_the_logits(shape, per_image, classes):
    n, c, h, w = shape
    x64, y = ref.separated_inputs(n, c, h, w, seed=n * 100 + c * 10 + h)
    x = x64.float()  # (the truth is taken at the fp32 logits the kernel sees)
    assert ref.min_error_gap(torch.softmax(x.double(), 1), y, per_image) >= 1e-5  # the order is unambiguous
    xa = x.double().requires_grad_(True)
    want = ref.lovasz_softmax(torch.softmax(xa, 1), y, per_image=per_image, classes=classes)
    want.backward()
    got, grad, _ = _run(x, y, per_image, classes)
    assert abs(got - float(want)) <= 1e-5 * abs(float(want)), (got, float(want))
    scale = float(xa.grad.abs().max())
    assert float((grad.double() - xa.grad).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize("shape,per_image", [((8, 2, 512, 512), True), ((2, 4, 512, 512), True), ((4, 3, 256, 256), False),
                                             ((16, 2, 512, 512), False)],
                         ids=["8x2x512-img", "2x4x512-img", "4x3x256-flat", "16x2x512-flat-chunked-scan"])
def test_exact_permutation_at_real_sizes(shape, per_image):
    """The restatement fed the kernel's own fp32 p, with the errors rounded as fp32 rounds them: the very keys the kernel
    sorted, so the same order and ties -- this checks the closed-form deltas, the segment layout and the tie order."""

    n, c, h, w = shape
    g = torch.Generator().manual_seed(n + c)
    x = torch.randn(n, c, h, w, generator=g) * 2.0
    y = torch.randint(0, c, (n, h, w), generator=g)
    y[0, : h // 2][y[0, : h // 2] == c - 1] = 0  # fewer pixels of one class in one image
    got, grad, probs = _run(x, y, per_image, "present", want_probs=True)
    assert torch.allclose(probs, torch.softmax(x.double(), 1).float(), rtol=1e-5, atol=1e-7)
    p = probs.double().requires_grad_(True)
    want = ref.lovasz_softmax(p, y, per_image=per_image, classes="present", fp32_errors=True)
    want.backward()
    assert abs(got - float(want)) <= 1e-6 * abs(float(want)), (got, float(want))
    want_dx = ref.softmax_backward(probs.double(), p.grad)
    scale = float(want_dx.abs().max())
    assert float((grad.double() - want_dx).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (3, 2, 2, 257), (2, 2, 17, 241), (16, 2, 65, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("per_image", [True, False])
@pytest.mark.parametrize("name", ["quant", "two"])
def test_exact_permutation_at_ties_and_tile_edges(name, shape, per_image):
    """The same comparison under the same bars where the shared sort can go wrong: logits on a grid (``quant``) or in {-3, 3}
    (``two``, a handful of keys per segment, so the result hangs on the sort's stability), HW % 4 != 0, a second sort tile of
    2 keys (flattened, at 2x2x17x241), the XCD-affine orders."""

    x, y = lovasz_hinge_ref.family(name, shape, seed=sum(shape))
    got, grad, probs = _run(x, y, per_image, "present", want_probs=True)
    assert torch.allclose(probs, torch.softmax(x.double(), 1).float(), rtol=1e-5, atol=1e-7)
    p = probs.double().requires_grad_(True)
    want = ref.lovasz_softmax(p, y, per_image=per_image, classes="present", fp32_errors=True)
    want.backward()
    want = want.item()
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    want_dx = ref.softmax_backward(probs.double(), p.grad)
    scale = float(want_dx.abs().max())
    assert float((grad.double() - want_dx).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize("c", [2, 3, 5])
def test_hard_predictions_give_one_minus_mean_iou(c):
    n, h, w = 4, 128, 96
    g = torch.Generator().manual_seed(c)
    y = torch.randint(0, c, (n, h, w), generator=g)
    y[1][y[1] == c - 1] = 0
    pred = torch.where(torch.rand(n, h, w, generator=g) < 0.7, y, torch.randint(0, c, (n, h, w), generator=g))
    x = (torch.nn.functional.one_hot(pred, c).permute(0, 3, 1, 2).float() * 200.0 - 100.0).contiguous()  # p = 0 or 1 in fp32
    for per_image in (True, False):
        got, _, probs = _run(x, y, per_image, "present", want_probs=True)
        assert set(torch.unique(probs).tolist()) <= {0.0, 1.0}
        want = ref.mean_iou_loss(pred, y, c, per_image=per_image)
        assert abs(got - want) <= 1e-6, (per_image, got, want)


@pytest.mark.parametrize("per_image", [True, False])
def test_deterministic(per_image):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 3, 256, 256, generator=g).to(DEV)
    y = torch.randint(0, 3, (4, 256, 256), generator=g).to(DEV)
    l1, g1, _ = ops.lovasz_softmax_fwd(x, y, per_image=per_image)
    l2, g2, _ = ops.lovasz_softmax_fwd(x, y, per_image=per_image)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_per_image_batch_is_the_mean_of_its_images():
    n, c, h, w = 4, 3, 128, 128
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, c, h, w, generator=g).to(DEV)
    y = torch.randint(0, c, (n, h, w), generator=g).to(DEV)
    y[2][y[2] == 1] = 0
    lb, gb, _ = ops.lovasz_softmax_fwd(x, y)
    singles = [ops.lovasz_softmax_fwd(x[i:i + 1].contiguous(), y[i:i + 1].contiguous()) for i in range(n)]
    mean = sum(float(l) for l, _, _ in singles) / n
    assert abs(float(lb) - mean) <= 1e-6 * abs(mean)
    for i, (_, gi, _) in enumerate(singles):
        assert float((gb[i] * n - gi[0]).abs().max()) <= 1e-6 * float(gi.abs().max())


def test_odd_sizes_and_invalid_arguments():
    # HW % 4 != 0 takes the one-pixel-per-thread kernels; flattened, a segment spans two sort tiles and nine scan blocks
    x64, y = ref.separated_inputs(3, 3, 45, 67, seed=1)
    x = x64.float()
    for per_image in (True, False):
        assert ref.min_error_gap(torch.softmax(x.double(), 1), y, per_image) >= 1e-5
        xa = x.double().requires_grad_(True)
        want = ref.lovasz_softmax(torch.softmax(xa, 1), y, per_image=per_image)
        want.backward()
        got, grad, _ = _run(x, y, per_image, "present")
        assert abs(got - float(want)) <= 1e-5 * abs(float(want))
        assert float((grad.double() - xa.grad).abs().max()) <= 1e-5 * float(xa.grad.abs().max())
    from robosat_amd import _lib

    lib = _lib.lib()
    assert lib.rs_lovasz_softmax_workspace_bytes(2, 1, 8, 8, 1) == _lib.RS_EINVAL  # C < 2
    assert lib.rs_lovasz_softmax_workspace_bytes(0, 3, 8, 8, 1) == _lib.RS_EINVAL
    assert lib.rs_lovasz_softmax_workspace_bytes(2, 3, -8, 8, 0) == _lib.RS_EINVAL
    assert lib.rs_lovasz_softmax_workspace_bytes(1 << 12, 4, 512, 256, 1) == _lib.RS_EINVAL  # 2^31 elements
    assert lib.rs_lovasz_softmax_workspace_bytes(2, 3, 8, 8, 0) > 0
    with pytest.raises(ValueError):
        ops.lovasz_softmax_fwd(torch.zeros(1, 1, 8, 8, device=DEV), torch.zeros(1, 8, 8, dtype=torch.long, device=DEV))


def test_module_autograd_scales_the_unit_gradient():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 4, 64, 64, generator=g).to(DEV)
    y = torch.randint(0, 4, (2, 64, 64), generator=g).to(DEV)
    for per_image, classes in ((True, "present"), (False, "all")):
        _, unit, _ = ops.lovasz_softmax_fwd(x, y, per_image=per_image, classes=classes)
        xr = x.clone().requires_grad_(True)
        loss = LovaszSoftmax2d(per_image=per_image, classes=classes)(xr, y)
        (loss * 2.5).backward()
        assert torch.equal(xr.grad, unit * 2.5)


def test_bf16_model_logits_flow_through():
    from robosat_amd.unet import UNet

    net = UNet(3, pretrained=False, compute_dtype="bf16").to(DEV).train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 64, 64, generator=g).to(DEV)
    y = torch.randint(0, 3, (2, 64, 64), generator=g).to(DEV)
    out = net(x)
    assert out.dtype == torch.float32
    loss = LovaszSoftmax2d()(out, y)
    loss.backward()
    assert torch.isfinite(loss) and 0.0 < float(loss) <= 1.0
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(t).all() for t in grads)


def test_cpu_input_raises():
    with pytest.raises(RuntimeError, match="MI355X only"):
        LovaszSoftmax2d()(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8, dtype=torch.long))
