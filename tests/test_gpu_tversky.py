"""The Tversky loss family on the MI355X (``rs_tversky_sums`` / ``rs_tversky_finalize`` / ``rs_tversky_bwd``, ``TverskyLoss2d``) against
the float64 reference of tests/tversky_ref.py, with the project's own bars: ``LOSS_BAR`` for the loss, ``MIOU_GRAD_BAR`` of the
largest wanted entry for the gradient (the coefficients have mIoU's structure; float32 torch stays 20 times inside both on these
inputs: tests/test_tversky_cpu.py).  Random logits of scale 2 keep 1 - TI far from 0, so the kink is not in play."""

import functools
import itertools

import pytest
import torch

import losses_ref as L
import tversky_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run(logits, targets, weight=None, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, per_image=True, classes="present", ce=0.0,
        ignore=None, world=1, grad_out=None):
    """The three calls on the device: (loss as a float, gradient, sums, stats), all on the host."""

    from robosat_amd import ops

    x, t = logits.to(DEV).contiguous(), targets.to(DEV)
    w = None if weight is None else weight.to(DEV)
    sums = ops.tversky_sums(x, t, w, per_image, ignore=ignore)
    loss, stats = ops.tversky_finalize(sums, x.shape[0], x.shape[1], alpha, beta, gamma, smooth, ce, classes, per_image, world)
    grad = ops.tversky_bwd(x, t, w, stats, grad_out, ce, per_image, ignore=ignore)
    return float(loss.cpu()), grad.cpu(), sums.cpu(), stats.cpu()


def check(logits, targets, weight=None, what="", **kw):
    want_loss, want_grad, _ = T.ref64(logits, targets, weight=weight, **kw)
    loss, grad, _, stats = run(logits, targets, weight, **kw)
    assert loss == float(stats[0])
    return T.compare(loss, grad, want_loss, want_grad, what)


@functools.lru_cache(maxsize=None)
def case(n, c, h, w):
    return T.random_case(n, c, h, w, seed=c)


# ---- class counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(2, 9))
def test_every_class_count(c):
    logits, targets, weight = case(3, c, 7, 9)
    alpha, beta, gamma, smooth = T.PARAMS[c % 4]
    for per_image in (True, False):
        check(logits, targets, weight, "C = {}".format(c), alpha=alpha, beta=beta, gamma=gamma, smooth=smooth, per_image=per_image,
              classes="all" if c % 2 else "present", ce=0.5)


@pytest.mark.parametrize("c", [1, 9])
def test_one_and_nine_classes_are_refused(c):
    from robosat_amd import losses

    x = torch.zeros(1, c, 4, 4, device=DEV, requires_grad=True)
    with pytest.raises(ValueError):
        losses.TverskyLoss2d().to(DEV)(x, torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV))


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", [True, False])
@pytest.mark.parametrize("shape", T.SHAPES)
def test_shapes(shape, per_image):
    n, h, w = shape
    logits, targets, weight = case(n, 3, h, w)
    alpha, beta, gamma, smooth = T.PARAMS[T.SHAPES.index(shape) % 4]
    check(logits, targets, weight, "{}".format(shape), alpha=alpha, beta=beta, gamma=gamma, smooth=smooth, per_image=per_image, ce=0.5)


# ---- parameters ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", T.PARAMS)
def test_parameters_with_every_form(params):
    """Every (alpha, beta, gamma, smooth) per image and over the batch, over the classes present and over all, with lambda 0 and 0.5, with
    and without class weights: the whole product, at 3 x 5 x 33 x 31 (four blocks per image, an odd size)."""

    alpha, beta, gamma, smooth = params
    logits, targets, weight = case(3, 5, 33, 31)
    for per_image, classes, ce, w in itertools.product((True, False), ("present", "all"), (0.0, 0.5), (None, weight)):
        check(logits, targets, w, "{} {} {} ce {} {}".format(params, "per image" if per_image else "batch", classes, ce,
                                                             "weighted" if w is not None else "unweighted"),
              alpha=alpha, beta=beta, gamma=gamma, smooth=smooth, per_image=per_image, classes=classes, ce=ce)


def test_lambda_zero_ignores_the_weights_bit_for_bit():
    logits, targets, weight = case(3, 5, 33, 31)
    a = run(logits, targets, None, ce=0.0)
    b = run(logits, targets, weight, ce=0.0)
    assert a[0] == b[0] and torch.equal(a[1], b[1])


# ---- a class absent from one image --------------------------------------------------------------------------------------------------
def test_absent_class_present_and_all_differ():
    logits, targets, weight = T.absent_class_case()
    n, c = 2, logits.shape[1]
    absent = c - 1
    p = torch.softmax(logits.double(), 1)
    out = {}
    for classes in ("present", "all"):
        for per_image in (True, False):
            check(logits, targets, weight, "absent class, {}".format(classes), classes=classes, per_image=per_image, ce=0.5)
        out[classes] = run(logits, targets, None, classes=classes)
    assert abs(out["present"][0] - out["all"][0]) > 100 * L.LOSS_BAR
    for classes in ("present", "all"):
        loss, grad, sums, stats = out[classes]
        g1 = stats[4:4 + n * c].double().view(n, c)
        g0 = stats[4 + n * c:4 + 2 * n * c].double().view(n, c)
        if classes == "present":  # no coefficient of its own: exactly the Jacobian's cross-terms
            assert float(g1[0, absent]) == 0.0 and float(g0[0, absent]) == 0.0
        else:  # the FP-only coefficient of Dice with smooth 1: TP = cnt = 0, TI = 1 / (SP / 2 + 1), weight 1 / (N C)
            sp = float(p[0, absent].sum())
            want = 0.5 / (0.5 * sp + 1.0) ** 2 / (n * c)
            assert abs(float(g0[0, absent]) - want) <= 1e-6 * want, (float(g0[0, absent]), want)
        g = torch.where(T.segment_hot(targets, c)[0], g1[0].view(c, 1, 1), g0[0].view(c, 1, 1))
        dot = (g * p[0]).sum(0)
        want_plane = p[0, absent] * (g[absent] - dot)
        scale = float(want_plane.abs().max())
        assert scale > 0 and float((grad[0, absent].double() - want_plane).abs().max()) <= 1e-5 * scale


# ---- the ignore label ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", [True, False])
def test_ignore_label(per_image):
    logits, targets, weight = case(3, 3, 33, 31)
    marked = T.with_ignored(targets)
    marked[2] = T.IGNORE  # an image with no valid pixel
    kw = dict(alpha=0.3, beta=0.7, gamma=0.75, smooth=1.0, per_image=per_image, ce=0.5, ignore=T.IGNORE)
    for classes in ("present", "all"):
        check(logits, marked, weight, "ignore {}".format(classes), classes=classes, **kw)
    loss, grad, sums, stats = run(logits, marked, weight, **kw)
    ignored = (marked == T.IGNORE).unsqueeze(1).expand_as(grad)
    assert bool((grad[ignored].view(torch.int32) == 0).all())  # +0.0f bit for bit
    assert bool((grad[2].view(torch.int32) == 0).all())
    if per_image:
        assert float(sums[2 * 9:3 * 9].abs().max()) == 0.0
        two = run(logits[:2], marked[:2], weight, **kw)  # the empty image contributes 0 to T and the divisor stays N
        assert abs(float(stats[1]) - float(two[3][1]) * 2.0 / 3.0) <= 1e-6
    # logits under ignored pixels are never read
    poisoned = torch.where(ignored, torch.full_like(logits, float("nan")), logits)
    again = run(poisoned, marked, weight, **kw)
    assert again[0] == loss and torch.equal(again[1], grad) and torch.equal(again[2], sums)


@pytest.mark.parametrize("per_image", [True, False])
def test_no_pixel_ignored_gives_the_plain_bits(per_image):
    logits, targets, weight = case(2, 3, 129, 129)
    kw = dict(alpha=0.7, beta=0.3, gamma=2.0, smooth=0.0, per_image=per_image, ce=0.5)
    plain = run(logits, targets, weight, **kw)
    with_label = run(logits, targets, weight, ignore=T.IGNORE, **kw)
    assert plain[0] == with_label[0] and all(torch.equal(a, b) for a, b in zip(plain[1:], with_label[1:]))


def test_a_batch_without_a_valid_pixel():
    logits, targets, weight = case(2, 3, 1, 300)
    for per_image in (True, False):
        loss, grad, _, _ = run(logits, torch.full_like(targets, T.IGNORE), weight, per_image=per_image, classes="all", ce=0.5,
                               ignore=T.IGNORE)
        assert loss == 0.0 and bool((grad.view(torch.int32) == 0).all())


# ---- single-pixel probes at the block and trip borders of the sums kernel -----------------------------------------------------------
def test_single_pixel_probes():
    """Relabelling ONE pixel of image 1 -- at a block border, the last pixel of trip 1, the first of trip 2, the last of the image --
    changes the sums of exactly its two classes: cnt by one, TP by the pixel's probability, nothing else by a bit."""

    from robosat_amd import ops

    n, c, h, w = L.MIOU_PROBE_SHAPE
    logits, targets, _ = case(n, c, h, w)
    x = logits.to(DEV)
    p = torch.softmax(logits.double(), 1).view(n, c, h * w)
    base = ops.tversky_sums(x, targets.to(DEV), None, True).cpu()
    for hw in L.MIOU_PROBE_HW:
        a = int(targets.view(n, h * w)[1, hw])
        b = (a + 1) % c
        edited = targets.clone()
        edited.view(n, h * w)[1, hw] = b
        got = ops.tversky_sums(x, edited.to(DEV), None, True).cpu()
        d = (got - base)[:3 * n * c].view(n, c, 3)
        assert float(d[0].abs().max()) == 0.0, hw  # image 0: not a bit
        assert float(d[1, :, 1].abs().max()) == 0.0, hw  # SP: the probabilities did not change
        other = 3 - a - b
        assert float(d[1, other].abs().max()) == 0.0, hw
        assert float(d[1, a, 2]) == -1.0 and float(d[1, b, 2]) == 1.0, hw
        assert abs(float(d[1, a, 0]) + float(p[1, a, hw])) <= 1e-6 and abs(float(d[1, b, 0]) - float(p[1, b, hw])) <= 1e-6, hw
        assert float(got[3 * n * c + 1]) == float(base[3 * n * c + 1]), hw  # the CE denominator: unweighted, one pixel each way
        want_num = float(torch.log(p[1, a, hw]) - torch.log(p[1, b, hw]))
        assert abs(float(got[3 * n * c] - base[3 * n * c]) - want_num) <= 1e-4, hw
    # and the batch form adds the images in a fixed order: its sums are the per-image sums added
    batch = ops.tversky_sums(x, targets.to(DEV), None, False).cpu()
    want = base[:3 * n * c].view(n, c * 3).sum(0)
    assert torch.equal(batch[:3 * c], want) and torch.equal(batch[3 * c:], base[3 * n * c:])


# ---- reproducibility and layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", [True, False])
def test_same_bits_twice_and_a_small_call_after_a_large_one(per_image):
    kw = dict(alpha=0.3, beta=0.7, gamma=0.75, smooth=1.0, per_image=per_image, ce=0.5)
    small = case(1, 3, 1, 5)
    large = case(2, 3, 129, 129)
    first = run(small[0], small[1], small[2], **kw)
    big = run(large[0], large[1], large[2], **kw)
    again = run(large[0], large[1], large[2], **kw)
    assert big[0] == again[0] and all(torch.equal(a, b) for a, b in zip(big[1:], again[1:]))
    after = run(small[0], small[1], small[2], **kw)  # (the workspace now holds the large call's partial sums)
    assert first[0] == after[0] and all(torch.equal(a, b) for a, b in zip(first[1:], after[1:]))


def test_a_strided_input_equals_its_contiguous_copy():
    from robosat_amd import losses

    logits, targets, weight = case(3, 3, 33, 31)
    crit = losses.TverskyLoss2d(0.3, 0.7, 0.75, ce=0.5, weight=weight).to(DEV)
    out = []
    nhwc = logits.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # same values, channels-last strides
    assert not nhwc.is_contiguous()
    for x in (logits.to(DEV), nhwc):
        x = x.detach().requires_grad_(True)
        loss = crit(x, targets.to(DEV))
        loss.backward()
        out.append((loss.item(), x.grad.contiguous().cpu()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])


# ---- identity with the shipped mIoU kernel ------------------------------------------------------------------------------------------
def test_the_soft_jaccard_is_the_shipped_miou_kernels_soft_iou_branch():
    from robosat_amd import losses

    logits, targets, weight = L.miou_case("confident")  # (asserts the "miou" branch by >= 1e-2 on the float64 reference)
    x = logits.to(DEV).requires_grad_(True)
    want = losses.mIoULoss2d(weight=weight).to(DEV)(x, targets.to(DEV))
    want.backward()
    loss, grad, _, _ = run(logits, targets, None, alpha=1.0, beta=1.0, gamma=1.0, smooth=0.0, per_image=True, classes="all", ce=0.0)
    T.compare(loss, grad, want.item(), x.grad.cpu(), "against mIoULoss2d")


# ---- data parallelism, emulated in one process --------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", T.PARAMS)
@pytest.mark.parametrize("per_image", [True, False])
def test_two_shards_with_the_exchange_give_the_single_evaluation(params, per_image):
    from robosat_amd import ops

    alpha, beta, gamma, smooth = params
    logits, targets, weight = T.shard_case()
    kw = dict(alpha=alpha, beta=beta, gamma=gamma, smooth=smooth, classes="present", ce=0.5)
    (want_loss, want_grad), _ = T.two_shard_reference(logits, targets, weight, per_image, **kw)
    w = weight.to(DEV)
    shards = [(logits[s].to(DEV).contiguous(), targets[s].to(DEV).contiguous()) for s in (slice(0, 2), slice(2, 4))]
    sums = [ops.tversky_sums(x, t, w, per_image) for x, t in shards]

    def finish(blocks, world):
        losses, grads = [], []
        for (x, t), block in zip(shards, blocks):
            loss, stats = ops.tversky_finalize(block, 2, 3, alpha, beta, gamma, smooth, 0.5, "present", per_image, world)
            losses.append(float(loss.cpu()))
            grads.append(ops.tversky_bwd(x, t, w, stats, None, 0.5, per_image).cpu())
        return sum(losses) / 2, torch.cat(grads, 0) / 2

    if per_image:  # only the CE denominators are added
        den = sums[0][-1] + sums[1][-1]
        exchanged = [torch.cat([s[:-1], den.view(1)]) for s in sums]
    else:  # the whole block
        exchanged = [sums[0] + sums[1]] * 2
    loss, grad = finish(exchanged, 2)
    T.compare(loss, grad, want_loss, want_grad, "two shards, exchanged")
    naive_loss, naive_grad = finish(sums, 1)
    dl, dg = L.distances(naive_loss, naive_grad, want_loss, want_grad)
    print("un-exchanged: loss distance {:.2e}, gradient distance {:.2e}".format(dl, dg))
    if not per_image:
        assert dl > 10 * L.LOSS_BAR and dg > 10 * L.MIOU_GRAD_BAR, (dl, dg)


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def test_module_behaviour():
    from robosat_amd import losses

    logits, targets, weight = case(3, 3, 33, 31)
    crit = losses.TverskyLoss2d(alpha=0.3, beta=0.7, gamma=0.75, ce=0.5, weight=weight)
    assert crit.weight.device.type == "cpu"
    crit = crit.to(DEV)
    assert crit.weight.is_cuda  # a buffer: .to(device) moves it
    want_loss, want_grad, _ = T.ref64(logits, targets, 0.3, 0.7, 0.75, 1.0, ce=0.5, weight=weight)
    for upstream in (1.0, 1.5):
        x = logits.to(DEV).requires_grad_(True)
        loss = crit(x, targets.to(DEV))
        assert loss.dim() == 0 and loss.dtype == torch.float32
        (loss * upstream).backward()
        T.compare(loss.item(), x.grad.cpu().double() / upstream, want_loss, want_grad, "module, upstream {}".format(upstream))
    ignoring = losses.TverskyLoss2d(ignore_index=T.IGNORE, per_image=False, classes="all").to(DEV)
    marked = T.with_ignored(targets)
    x = logits.to(DEV).requires_grad_(True)
    loss = ignoring(x, marked.to(DEV))
    loss.backward()
    want = T.ref64(logits, marked, per_image=False, classes="all", ignore=T.IGNORE)
    T.compare(loss.item(), x.grad.cpu(), want[0], want[1], "module, ignore, batch form")
    with pytest.raises(RuntimeError, match="no CPU"):
        crit(logits, targets)
    with pytest.raises(ValueError, match="ignore_index"):
        losses.TverskyLoss2d(ignore_index=2).to(DEV)(logits.to(DEV), targets.to(DEV))
