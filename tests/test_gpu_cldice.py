"""The soft skeleton and the clDice term on the MI355X against tests/cldice_ref.py (include/robosat_hip.h).

The forward is compared bit for bit with the fp32 torch evaluation; the backward exactly where every number is a small dyadic
(planes from {0, 1/2, 1}, integer gradients: the fp32 and fp64 references agree to the last bit there, so no summation order can
matter), and elsewhere against the fp64 reference with a bound taken from the fp32 reference's own distance to it."""

import functools
import zlib

import pytest
import torch

import cldice_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

# (the last one spans several 64 x 4 tiles of the kernels in both directions, with a ragged last tile each way)
SHAPES = [(1, 1, 1), (2, 1, 7), (2, 5, 1), (1, 3, 3), (4, 17, 33), (3, 70, 130), (2, 37, 200)]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))  # (the same draws in every process)


@functools.lru_cache(maxsize=None)
def _planes(shape, kind):
    if kind == "random":
        return torch.rand(shape, generator=_gen(shape, kind, 1))
    return torch.randint(0, 3, shape, generator=_gen(shape, kind, 2)).float() / 2  # plateaus: {0, 1/2, 1}


@functools.lru_cache(maxsize=None)
def _upstream(shape, kind):
    if kind == "integer":
        return torch.randint(-3, 4, shape, generator=_gen(shape, kind, 3)).float()
    return torch.randn(shape, generator=_gen(shape, kind, 4))


@functools.lru_cache(maxsize=None)
def _skeleton_refs(shape, kind, gkind, iters):
    """(skeleton fp32, gradient fp32, gradient fp64) by torch CPU autograd from the same plane bits."""

    x, g = _planes(shape, kind), _upstream(shape, gkind)
    s32, d32 = R.skeleton_autograd(x, iters, g, torch.float32)
    _, d64 = R.skeleton_autograd(x, iters, g, torch.float64)
    return s32, d32, d64


def _gpu_skeleton(x, iters, grad=None):
    from robosat_amd import ops

    skel, saved = ops.soft_skeleton(x.to(DEV), iters)
    dx = None if grad is None else ops.soft_skeleton_bwd(saved, grad.to(DEV).contiguous()).cpu()
    return skel.cpu(), dx


@pytest.mark.parametrize("kind", ["random", "plateaus"])
@pytest.mark.parametrize("iters", [0, 1, 3, 10])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_bit_for_bit(shape, iters, kind):
    x = _planes(shape, kind)
    want = R.soft_skeleton(x, iters)
    got, _ = _gpu_skeleton(x, iters)
    assert torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize("iters", [0, 1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_exact_at_ties(shape, iters):
    x, g = _planes(shape, "plateaus"), _upstream(shape, "integer")
    _, d32, d64 = _skeleton_refs(shape, "plateaus", "integer", iters)
    assert torch.equal(d32.double(), d64)  # (what makes the exact comparison legitimate)
    _, got = _gpu_skeleton(x, iters, g)
    assert torch.equal(got, d32), float((got - d32).abs().max())


@pytest.mark.parametrize("iters", [3, 10])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_on_random_planes(shape, iters):
    """|gpu - f64| <= max(4 max|ref32 - f64|, 16 * 2^-24 max|f64|) elementwise; the margin of 4 covers another summation order over at
    most 9 + 5 contributions per level.  Measured on the MI355X at (3, 70, 130), iters 10: max|ref32 - f64| = 1.17e-6, largest
    gradient 13.1, max|gpu - f64| = 1.03e-6 under a bound of 1.25e-5; at (2, 37, 200), iters 10: 1.93e-6, 10.6, 1.93e-6."""

    x, g = _planes(shape, "random"), _upstream(shape, "normal")
    _, d32, d64 = _skeleton_refs(shape, "random", "normal", iters)
    _, got = _gpu_skeleton(x, iters, g)
    ref_err = float((d32.double() - d64).abs().max())
    bound = max(4.0 * ref_err, 16.0 * EPS * float(d64.abs().max()))
    err = float((got.double() - d64).abs().max())
    print("skeleton bwd", shape, iters, "ref32-f64", ref_err, "max|f64|", float(d64.abs().max()), "gpu-f64", err, "bound", bound)
    assert torch.isfinite(got).all() and err <= bound, (err, bound)


def test_planes_do_not_see_each_other_and_the_edge_is_closed():
    m, h, w = 3, 9, 70
    x = torch.zeros(m, h, w)
    x[1, h - 1, w - 1] = 1.0
    g = _upstream((m, h, w), "integer")
    for iters in (0, 2, 10):
        s32, d32 = R.skeleton_autograd(x, iters, g)
        skel, dx = _gpu_skeleton(x, iters, g)
        assert torch.equal(skel, s32) and torch.equal(dx, d32)
        for other in (0, 2):
            assert not skel[other].any() and not dx[other].any()
        assert float(skel[1, h - 1, w - 1]) == 1.0 and float(skel[1].sum()) == 1.0


# ---- the whole loss from logits ----


def _logits(shape, kind, seed):
    n, c, h, w = shape
    x = torch.randn(shape, generator=_gen(shape, kind, seed))
    if kind == "smooth":
        x = 6.0 * torch.nn.functional.avg_pool2d(x, 7, 1, 3, count_include_pad=False)
    return x.contiguous()


def _targets(shape, seed):
    """Labels with structure: thresholded smooth noise, so that the classes form blobs and bands and not salt and pepper."""

    n, c, h, w = shape
    field = torch.nn.functional.avg_pool2d(torch.randn((n, 1, h, w), generator=_gen(shape, "t", seed)), 9, 1, 4)[:, 0]
    q = torch.quantile(field.flatten(), torch.linspace(0, 1, c + 1)[1:-1])
    return torch.bucketize(field, q).to(torch.int64).contiguous()


def _reference(logits, targets, iters, classes, ignore, dtype, smooth=1.0):
    x = logits.detach().clone().to(dtype).requires_grad_(True)
    loss = R.cldice_term(x, targets, iters, smooth, classes, ignore, dtype)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def _gpu_term(logits, targets, iters, classes, ignore, smooth=1.0):
    from robosat_amd.losses import ClDiceLoss2d, CrossEntropyLoss2d

    crit = ClDiceLoss2d(CrossEntropyLoss2d(), 0.5, iters=iters, smooth=smooth, classes=classes, ignore_index=ignore)
    x = logits.to(DEV).requires_grad_(True)
    loss = crit.term(x, targets.to(DEV))
    loss.backward()
    return loss.detach().cpu(), x.grad.cpu()


def _check_against_references(logits, targets, iters, classes, ignore, label):
    l32, g32 = _reference(logits, targets, iters, classes, ignore, torch.float32)
    l64, g64 = _reference(logits, targets, iters, classes, ignore, torch.float64)
    loss, grad = _gpu_term(logits, targets, iters, classes, ignore)
    loss_bound = max(4.0 * abs(float(l32) - float(l64)), 16.0 * EPS)
    grad_bound = max(4.0 * float((g32.double() - g64).abs().max()), 16.0 * EPS * float(g64.abs().max()))
    out32 = int(((g32.double() - g64).abs() > grad_bound).sum())
    out = int(((grad.double() - g64).abs() > grad_bound).sum())
    print(label, "loss", float(loss), "f64", float(l64), "|gpu-f64|", abs(float(loss) - float(l64)), "bound", loss_bound,
          "| grad max|f64|", float(g64.abs().max()), "max|ref32-f64|", float((g32.double() - g64).abs().max()),
          "max|gpu-f64|", float((grad.double() - g64).abs().max()), "bound", grad_bound, "left out", out, "ref32 left out", out32)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert abs(float(loss) - float(l64)) <= loss_bound, (float(loss), float(l64), loss_bound)
    assert out32 == 0  # (the references themselves agree everywhere on these inputs)
    assert out <= 8, out  # (a last-bit difference of the softmax may flip a selection between two nearly equal neighbours)
    return loss, grad, g64


@pytest.mark.parametrize("iters", [3, 10])
@pytest.mark.parametrize("kind", ["white", "smooth"])
@pytest.mark.parametrize("shape, classes", [((2, 2, 64, 64), None), ((2, 3, 40, 72), (2,))], ids=["2x2x64x64", "2x3x40x72-one-class"])
def test_whole_loss_from_logits(shape, classes, kind, iters):
    logits, targets = _logits(shape, kind, 5), _targets(shape, 6)
    _check_against_references(logits, targets, iters, classes, None, "loss {} {} {}".format(shape, kind, iters))


@pytest.mark.parametrize("iters", [3, 10])
def test_ignore_label(iters):
    shape = (2, 3, 40, 72)
    logits, targets = _logits(shape, "smooth", 7), _targets(shape, 8)
    targets[0, 5:20, 10:40] = 255
    targets[torch.rand(targets.shape, generator=_gen("scatter")) < 0.03] = 255
    _, grad, _ = _check_against_references(logits, targets, iters, None, 255, "ignore {}".format(iters))
    under = (targets == 255)[:, None].expand_as(grad)
    assert under.any() and not grad[under].any()


def test_runs_and_ranks():
    shape = (4, 2, 64, 64)
    logits, targets = _logits(shape, "smooth", 9), _targets(shape, 10)
    loss_a, grad_a = _gpu_term(logits, targets, 3, None, None)
    loss_b, grad_b = _gpu_term(logits, targets, 3, None, None)
    assert torch.equal(loss_a, loss_b) and torch.equal(grad_a, grad_b)
    halves = [_gpu_term(logits[i:i + 2].contiguous(), targets[i:i + 2].contiguous(), 3, None, None) for i in (0, 2)]
    mean = 0.5 * (float(halves[0][0]) + float(halves[1][0]))
    assert abs(float(loss_a) - mean) <= 4.0 * EPS * 2.0 * abs(mean), (float(loss_a), mean)  # (4 ulp of the loss's magnitude)
    _, g32 = _reference(logits, targets, 3, None, None, torch.float32)
    _, g64 = _reference(logits, targets, 3, None, None, torch.float64)
    bound = max(4.0 * float((g32.double() - g64).abs().max()), 16.0 * EPS * float(g64.abs().max()))
    joined = torch.cat([halves[0][1], halves[1][1]]).double() / 2.0
    assert float((grad_a.double() - joined).abs().max()) <= bound


def test_saturation():
    shape = (2, 2, 64, 64)
    logits, targets = (60.0 * _logits(shape, "white", 11)).contiguous(), _targets(shape, 12)
    probs = torch.softmax(logits, 1)
    assert 0.3 < float(((probs == 0) | (probs == 1)).float().mean())
    l32, _ = _reference(logits, targets, 10, None, None, torch.float32)
    l64, _ = _reference(logits, targets, 10, None, None, torch.float64)
    loss, grad = _gpu_term(logits, targets, 10, None, None)
    print("saturation", float(loss), float(l64), float(l32))
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert abs(float(loss) - float(l64)) <= max(4.0 * abs(float(l32) - float(l64)), 16.0 * EPS)


def test_the_wrapper_mixes_base_and_term():
    from robosat_amd.losses import ClDiceLoss2d, CrossEntropyLoss2d

    shape = (2, 2, 64, 64)
    logits, targets = _logits(shape, "smooth", 13).to(DEV), _targets(shape, 14).to(DEV)
    base = CrossEntropyLoss2d().to(DEV)
    crit = ClDiceLoss2d(base, 0.3, iters=3).to(DEV)
    want = 0.7 * float(base(logits, targets)) + 0.3 * float(crit.term(logits, targets))
    assert abs(float(crit(logits, targets)) - want) <= 16.0 * EPS  # (a few fp32 roundings of numbers below 1)
    crit.eval()
    assert not base.training
