"""Losses of the reference (``robosat/losses.py``) on the MI355X: same class names, constructor arguments and
``forward(inputs[N,C,H,W] float32, targets[N,H,W] int64) -> 0-dim tensor`` contract (tools/train.py:97-106,185), with
the arithmetic in ``librobosat_hip.so`` (``rs_nll_loss_*``, ``rs_lovasz_fwd``), and two losses the reference does not have:
``LovaszSoftmax2d`` (``rs_lovasz_softmax_fwd``) and ``TverskyLoss2d`` (``rs_tversky_*``): Dice, the Tversky index and the focal
Tversky loss, per image or over the batch, with an optional cross-entropy term fused into the same passes.  No CPU path.

Every loss takes ``ignore_index=None``, the ``ignore_index`` of ``nn.CrossEntropyLoss`` for all six: a label value (no class, at
most 255) whose pixels are left out -- the loss is the same definition evaluated on the other pixels only, as if the ignored
ones had been cut out of every image (``rs_*_ig``, include/robosat_hip.h; DESIGN.md "Ignore label").  ``None`` makes exactly the
calls made without the argument.

``CrossEntropyLoss2d`` and ``FocalLoss2d`` also take ``boundary=(w0, sigma)``: the U-Net paper's border weight map on top of the class
weights (``rs_boundary_weight_plane``, ``rs_nll_loss_*_pw``), and ``hard=fraction`` or ``hard=(fraction, below)``: hard-pixel mining, per
image only the hardest share of the pixels keeps its weight (``rs_hard_pixel_plane``), in training mode only.  ``mIoULoss2d``,
``TverskyLoss2d`` and the two Lovasz forms take neither.  ``separation=(ws, sigma)`` adds the paper's second term, the weight of the
narrow background gap between two objects (``rs_separation_weight_plane``), for the same two criteria.  ``relax=R`` is boundary
label relaxation for the same two: in training mode a pixel within R pixels of other classes is charged ``-log`` of the probability
of all of them together (``rs_label_set_plane``, ``rs_nll_loss_*_rx``).

``ClDiceLoss2d(base, weight)`` wraps any of them and adds the clDice topology term (``rs_soft_skeleton_*``, ``rs_cldice_*``)."""

import torch
import torch.nn as nn

from . import ops


def _check(inputs, targets):
    if not inputs.is_cuda:
        raise RuntimeError("robosat_amd losses run on the MI355X only (got a {} tensor); there is no CPU fallback".format(inputs.device))
    assert inputs.dim() == 4 and targets.dim() == 3 and inputs.shape[0] == targets.shape[0] and inputs.shape[2:] == targets.shape[1:]
    assert targets.dtype == torch.int64
    return inputs.contiguous(), targets.contiguous()


def _check_ignore(ignore_index, inputs):
    """``ignore_index`` against the class count of the logits it meets in ``forward`` (``None`` passes)."""

    if ignore_index is None:
        return None
    classes = inputs.shape[1]
    if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index or not classes <= ignore_index <= 255:
        raise ValueError("ignore_index must be an integer in {}..255 for logits of {} classes (a class index cannot be ignored), "
                         "got {!r}".format(classes, classes, ignore_index))
    return int(ignore_index)


def _dp_world(global_batch):
    """World size when ``global_batch`` asks for the data-parallel exchange and there is a group of > 1 ranks, else 1."""

    import torch.distributed as dist

    if not global_batch or not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size()


def _global_batch_normaliser(loss, stats, global_batch):
    """Data-parallel ranks: make the weighted-NLL normaliser the GLOBAL batch's.

    The reference's ``DataParallel`` gathers the logits of all replicas and evaluates ONE loss over the global batch
    (tools/train.py:180-186): ``sum_i w_i l_i / sum_i w_i`` with both sums over every pixel of every shard.  Each rank here
    sees only its shard, and the mean of per-shard ratios is a different number (and gradient) whenever the shards' class
    mixes -- hence their weight sums -- differ.  The fix costs one scalar all-reduce: with ``D = mean_r sum_i w_i`` (the
    global denominator / world) replacing the local denominator, the rank's loss becomes ``num_r / D`` and the average of
    the ranks' losses / gradients that ``rs train`` forms anyway is exactly the global-batch loss / gradient.
    ``stats[1]`` (what ``rs_nll_loss_bwd`` divides by) is rewritten in place; returns the rescaled loss.

    OPT-IN (``criterion.global_batch = True``; ``rs train`` and ``bench.py`` set it on the ranks of a data-parallel job):
    it is a blocking collective inside ``forward``, so EVERY rank must call the loss the same number of times -- a
    rank-0-only evaluation or an unevenly sharded validation pass would hang in it."""

    import torch.distributed as dist

    world = _dp_world(global_batch)
    if world == 1:
        return loss
    local = stats[1].clone()
    den = stats[1:2]
    dist.all_reduce(den)  # (a 4-byte SUM on the device; no host sync)
    den.div_(world).clamp_(min=1e-30)  # (a global batch whose every pixel has weight 0: 0 / tiny = 0, not NaN)
    return loss * (local / den[0])


def _global_batch_miou(loss, stats, global_batch):
    """Data-parallel ranks: ``mIoULoss2d``'s ``max(miou, nll)`` decided ONCE over the global batch (losses.py:72-83 under
    tools/train.py:69), not per shard.

    The soft-IoU term is a mean over (class, image), so the global value is the mean of the ranks' values; the NLL term is
    ``sum_i w_i l_i / sum_i w_i`` over every shard.  The ranks exchange three scalars (their miou, NLL numerator, weight sum:
    one 12-byte all-reduce on the device, no host sync), every rank takes the same branch, and in the NLL branch the
    denominator becomes ``D = mean_r sum_i w_i`` as for the plain weighted losses: the average of the ranks' losses and
    gradients then equals the reference's single evaluation.  ``stats[1]`` / ``stats[2]`` (what ``rs_miou_loss_bwd`` divides
    by / branches on) are rewritten in place.  Opt-in like ``_global_batch_normaliser``."""

    import torch.distributed as dist

    world = _dp_world(global_batch)
    if world == 1:
        return loss
    n = stats.numel()
    miou_r, num_r = stats[n - 2], stats[n - 1]
    v = torch.stack([miou_r, num_r, stats[1]])
    dist.all_reduce(v)
    miou_g = v[0] / world
    den = (v[2] / world).clamp(min=1e-30)
    nll_g = v[1] / v[2].clamp(min=1e-30)
    use_nll = nll_g > miou_g
    stats[1] = den
    stats[2] = use_nll.to(stats.dtype)
    return torch.where(use_nll, num_r / den, miou_r)


class _NLLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, weight, mode, gamma, global_batch=False, ignore=None):
        x = inputs.detach().float()
        loss, stats = ops.nll_loss_fwd(x, targets, weight, mode, gamma, ignore=ignore)
        loss = _global_batch_normaliser(loss, stats, global_batch)
        ctx.save_for_backward(x, targets, stats)
        ctx.weight, ctx.mode, ctx.gamma, ctx.ignore = weight, mode, gamma, ignore
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, targets, stats = ctx.saved_tensors
        g = grad_out.detach().float().contiguous()
        return ops.nll_loss_bwd(x, targets, ctx.weight, stats, g, ctx.mode, ctx.gamma, ignore=ctx.ignore), None, None, None, None, None, None


class _NLLBoundaryFn(torch.autograd.Function):
    """``_NLLFn`` with the boundary weight plane (``ops.boundary_weight_plane``) made from ``targets`` in forward and kept for
    backward; the exchange of ``stats[1]`` is the same one."""

    @staticmethod
    def forward(ctx, inputs, targets, weight, mode, gamma, global_batch, ignore, boundary):
        x = inputs.detach().float()
        plane = ops.boundary_weight_plane(targets, boundary[0], boundary[1], ignore=ignore, classes=x.shape[1])
        loss, stats = ops.nll_loss_fwd(x, targets, weight, mode, gamma, ignore=ignore, pixel_weight=plane)
        loss = _global_batch_normaliser(loss, stats, global_batch)
        ctx.save_for_backward(x, targets, stats, plane)
        ctx.weight, ctx.mode, ctx.gamma, ctx.ignore = weight, mode, gamma, ignore
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, targets, stats, plane = ctx.saved_tensors
        g = grad_out.detach().float().contiguous()
        dx = ops.nll_loss_bwd(x, targets, ctx.weight, stats, g, ctx.mode, ctx.gamma, ignore=ctx.ignore, pixel_weight=plane)
        return dx, None, None, None, None, None, None, None


class _NLLHardFn(torch.autograd.Function):
    """``_NLLFn`` with the hard-pixel plane (``ops.hard_pixel_plane``) made from the logits in forward and kept for backward; with
    ``boundary`` the boundary weight plane is its base, so a kept pixel carries its boundary weight.  The selection is piecewise
    constant, so the gradient is the ``_pw`` gradient with the plane as it stands; the exchange of ``stats[1]`` is the same one."""

    @staticmethod
    def forward(ctx, inputs, targets, weight, mode, gamma, global_batch, ignore, boundary, hard):
        x = inputs.detach().float()
        base = None
        if boundary is not None:
            base = ops.boundary_weight_plane(targets, boundary[0], boundary[1], ignore=ignore, classes=x.shape[1])
        plane, _ = ops.hard_pixel_plane(x, targets, hard[0], below=hard[1], ignore=ignore, base=base)
        loss, stats = ops.nll_loss_fwd(x, targets, weight, mode, gamma, ignore=ignore, pixel_weight=plane)
        loss = _global_batch_normaliser(loss, stats, global_batch)
        ctx.save_for_backward(x, targets, stats, plane)
        ctx.weight, ctx.mode, ctx.gamma, ctx.ignore = weight, mode, gamma, ignore
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, targets, stats, plane = ctx.saved_tensors
        g = grad_out.detach().float().contiguous()
        dx = ops.nll_loss_bwd(x, targets, ctx.weight, stats, g, ctx.mode, ctx.gamma, ignore=ctx.ignore, pixel_weight=plane)
        return dx, None, None, None, None, None, None, None, None


class _NLLSeparationFn(torch.autograd.Function):
    """``_NLLFn`` with the separation weight (``ops.separation_weight_plane``): the boundary weight plane (if any) is made first, the
    separation term is added onto it, and the hard-pixel mining (if any) takes the sum as its base.  The plane is made from ``targets``
    per image, so the exchange of ``stats[1]`` is the same one; the criteria without ``separation`` never come here."""

    @staticmethod
    def forward(ctx, inputs, targets, weight, mode, gamma, global_batch, ignore, boundary, separation, hard):
        x = inputs.detach().float()
        base = None
        if boundary is not None:
            base = ops.boundary_weight_plane(targets, boundary[0], boundary[1], ignore=ignore, classes=x.shape[1])
        plane = ops.separation_weight_plane(targets, separation[0], separation[1], ignore=ignore, classes=x.shape[1], base=base)
        if hard is not None:
            plane, _ = ops.hard_pixel_plane(x, targets, hard[0], below=hard[1], ignore=ignore, base=plane)
        loss, stats = ops.nll_loss_fwd(x, targets, weight, mode, gamma, ignore=ignore, pixel_weight=plane)
        loss = _global_batch_normaliser(loss, stats, global_batch)
        ctx.save_for_backward(x, targets, stats, plane)
        ctx.weight, ctx.mode, ctx.gamma, ctx.ignore = weight, mode, gamma, ignore
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, targets, stats, plane = ctx.saved_tensors
        g = grad_out.detach().float().contiguous()
        dx = ops.nll_loss_bwd(x, targets, ctx.weight, stats, g, ctx.mode, ctx.gamma, ignore=ctx.ignore, pixel_weight=plane)
        return dx, None, None, None, None, None, None, None, None, None


class _NLLRelaxFn(torch.autograd.Function):
    """``_NLLFn`` with boundary label relaxation: the label set plane (``ops.label_set_plane``) made from ``targets`` in forward and
    kept for backward.  The boundary and separation planes (if any) are made from the strict labels as without relaxation and passed
    as ``pixel_weight``.  ``stats[1]`` is the sum of the pixels' OWN class weights, which the sets do not enter, so its exchange is
    the same one; the criteria without ``relax`` never come here."""

    @staticmethod
    def forward(ctx, inputs, targets, weight, mode, gamma, global_batch, ignore, boundary, separation, relax):
        x = inputs.detach().float()
        plane = None
        if boundary is not None:
            plane = ops.boundary_weight_plane(targets, boundary[0], boundary[1], ignore=ignore, classes=x.shape[1])
        if separation is not None:
            plane = ops.separation_weight_plane(targets, separation[0], separation[1], ignore=ignore, classes=x.shape[1], base=plane)
        sets = ops.label_set_plane(targets, relax, ignore=ignore, classes=x.shape[1])
        loss, stats = ops.nll_loss_fwd(x, targets, weight, mode, gamma, ignore=ignore, pixel_weight=plane, label_sets=sets)
        loss = _global_batch_normaliser(loss, stats, global_batch)
        ctx.save_for_backward(x, targets, stats, sets, *(() if plane is None else (plane,)))
        ctx.weight, ctx.mode, ctx.gamma, ctx.ignore = weight, mode, gamma, ignore
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, targets, stats, sets = ctx.saved_tensors[:4]
        plane = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        g = grad_out.detach().float().contiguous()
        dx = ops.nll_loss_bwd(x, targets, ctx.weight, stats, g, ctx.mode, ctx.gamma, ignore=ctx.ignore, pixel_weight=plane,
                              label_sets=sets)
        return dx, None, None, None, None, None, None, None, None, None


class _MIoUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, weight, global_batch=False, ignore=None):
        x = inputs.detach().float()
        loss, stats = ops.miou_loss_fwd(x, targets, weight, ignore=ignore)
        loss = _global_batch_miou(loss, stats, global_batch)
        ctx.save_for_backward(x, targets, stats)
        ctx.weight, ctx.ignore = weight, ignore
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, targets, stats = ctx.saved_tensors
        return ops.miou_loss_bwd(x, targets, ctx.weight, stats, grad_out.detach().float().contiguous(), ignore=ctx.ignore), None, None, None, None


def _global_batch_tversky(sums, per_image, global_batch):
    """Data-parallel ranks: the sums of ``TverskyLoss2d`` made the GLOBAL batch's between its two forward stages; returns the world
    size ``rs_tversky_finalize`` is told.

    Per image the Tversky term is a mean over images, so the mean of the ranks' terms is the global one already and only the
    cross-entropy denominator (the last of the sums) is exchanged, as in ``_global_batch_normaliser``.  The batch form is a function
    of the per-class sums over every image of every rank: the whole block is exchanged (SUM, float64, 3 C + 2 numbers, on the device,
    no host sync), every rank then reports the global loss, and its gradient coefficients are multiplied by the world size so that
    the reducer's average of the ranks' gradients is the gradient of the one evaluation over the concatenated batch -- exact, unlike
    the flattened Lovasz-Softmax, which would need one sort over the global batch.  Opt-in like ``_global_batch_normaliser``."""

    import torch.distributed as dist

    world = _dp_world(global_batch)
    if world > 1:
        dist.all_reduce(sums[-1:] if per_image else sums)
    return world


class _TverskyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, weight, params, per_image, classes, global_batch=False, ignore=None):
        x = inputs.detach().float()
        alpha, beta, gamma, smooth, ce = params
        sums = ops.tversky_sums(x, targets, weight, per_image, ignore=ignore)
        world = _global_batch_tversky(sums, per_image, global_batch)
        loss, stats = ops.tversky_finalize(sums, x.shape[0], x.shape[1], alpha, beta, gamma, smooth, ce, classes, per_image, world)
        ctx.save_for_backward(x, targets, stats)
        ctx.weight, ctx.ce, ctx.per_image, ctx.ignore = weight, ce, per_image, ignore
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, targets, stats = ctx.saved_tensors
        g = grad_out.detach().float().contiguous()
        dx = ops.tversky_bwd(x, targets, ctx.weight, stats, g, ctx.ce, ctx.per_image, ignore=ctx.ignore)
        return dx, None, None, None, None, None, None, None


class _ClDiceFn(torch.autograd.Function):
    """The clDice term alone: planes, the two soft skeletons, the four sums per (image, class) and the scalar stage; the backward
    runs the skeleton's gather passes and the softmax Jacobian (``rs_soft_skeleton_*``, ``rs_cldice_*``)."""

    @staticmethod
    def forward(ctx, inputs, targets, iters, smooth, classes, ignore):
        x = inputs.detach().float()
        p, y = ops.cldice_planes(x, targets, classes, ignore)
        sp, saved = ops.soft_skeleton(p, iters)
        sy, _ = ops.soft_skeleton(y, iters, save=False)  # (no gradient through the labels: nothing kept)
        loss, coef = ops.cldice_finalize(ops.cldice_sums(p, y, sp, sy), smooth)
        ctx.save_for_backward(x, targets, y, sy, coef, saved[0], saved[1])
        ctx.iters, ctx.classes, ctx.ignore = iters, classes, ignore
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        x, targets, y, sy, coef, p, state = ctx.saved_tensors
        dp = ops.soft_skeleton_bwd((p, state, ctx.iters), ops.cldice_skel_grad(y, coef))
        g = grad_out.detach().float().contiguous()
        return ops.cldice_bwd(x, targets, dp, sy, coef, g, ctx.classes, ctx.ignore), None, None, None, None, None


class _LovaszFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, ignore=None):
        loss, grad_unit = ops.lovasz_fwd(inputs.detach().float(), targets, want_grad=True, ignore=ignore)
        ctx.save_for_backward(grad_unit)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (grad_unit,) = ctx.saved_tensors
        return ops.scale_by_scalar(grad_unit, grad_out.detach().float().contiguous()), None, None


class _LovaszSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, per_image, classes, ignore=None):
        loss, grad_unit, _ = ops.lovasz_softmax_fwd(inputs.detach().float(), targets, per_image, classes, want_grad=True, ignore=ignore)
        ctx.save_for_backward(grad_unit)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (grad_unit,) = ctx.saved_tensors
        return ops.scale_by_scalar(grad_unit, grad_out.detach().float().contiguous()), None, None, None, None


class _WeightedLoss(nn.Module):
    # Set to True on the ranks of a data-parallel job (rs train, bench.py): the batch-level terms of the loss -- the weighted
    # NLL's normaliser, mIoU's branch choice -- are then the GLOBAL batch's, as in the reference's single evaluation over the
    # gathered logits.  It adds a small blocking collective to forward(): every rank must call the loss equally often.
    global_batch = False

    def __init__(self, weight=None, ignore_index=None):
        super().__init__()
        self.ignore_index = ignore_index
        # a buffer (not a parameter) so that ``criterion.to(device)`` moves it, as nn.NLLLoss(weight) does
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32).clone())


def _check_boundary(boundary):
    """``boundary`` = ``(w0, sigma)`` of the boundary weight (``None`` passes): both finite and > 0, ``ceil(3 sigma) <= 128``."""

    if boundary is None:
        return None
    try:
        w0, sigma = boundary
    except (TypeError, ValueError):
        raise ValueError("boundary must be None or a pair (w0, sigma), got {!r}".format(boundary))
    ops.boundary_reach(w0, sigma)
    return (float(w0), float(sigma))


def _check_separation(separation):
    """``separation`` = ``(ws, sigma)`` of the separation weight (``None`` passes): both finite and > 0, ``ceil(3 sigma) <= 32``."""

    if separation is None:
        return None
    try:
        ws, sigma = separation
    except (TypeError, ValueError):
        raise ValueError("separation must be None or a pair (ws, sigma), got {!r}".format(separation))
    ops.separation_reach(ws, sigma)
    return (float(ws), float(sigma))


def _check_hard(hard):
    """``hard`` = ``fraction`` or ``(fraction, below)`` of the hard-pixel mining (``None`` passes) as ``(fraction, below | None)``: a
    finite fraction in (0, 1], a probability bound in (0, 1)."""

    if hard is None:
        return None
    if isinstance(hard, (int, float)) and not isinstance(hard, bool):
        hard = (hard, None)
    try:
        fraction, below = hard
    except (TypeError, ValueError):
        raise ValueError("hard must be None, a fraction or a pair (fraction, below), got {!r}".format(hard))
    fraction = ops.hard_fraction(fraction)
    if below is not None:
        ops.hard_cap(below)
        below = float(below)
    return (fraction, below)


def _check_relax(relax, hard):
    """``relax`` = the relaxation radius R in pixels (``None`` passes): an int in 1..16, no bool and no float; refused beside
    ``hard``."""

    if relax is None:
        return None
    if isinstance(relax, bool) or not isinstance(relax, int) or not 1 <= relax <= ops.RELAX_MAX_RADIUS:
        raise ValueError("relax must be None or an integer radius in 1..{} pixels, got {!r}".format(ops.RELAX_MAX_RADIUS, relax))
    if hard is not None:
        raise ValueError("relax cannot be combined with hard: hard-pixel mining ranks the pixels by their strict cross-entropy, which "
                         "is largest exactly on the band that relaxation forgives; ranking by the relaxed loss is not implemented")
    return relax


def _nll(self, inputs, targets, mode, gamma):
    """The call ``CrossEntropyLoss2d`` and ``FocalLoss2d`` make: without ``boundary``, ``separation``, ``hard`` and ``relax`` the calls
    they have always made; mining and relaxation are training devices, so in eval mode the criterion makes the calls it makes without
    ``hard`` and ``relax``."""

    inputs, targets = _check(inputs, targets)
    ignore = _check_ignore(self.ignore_index, inputs)
    if self.relax is not None and self.training:
        return _NLLRelaxFn.apply(inputs, targets, self.weight, mode, gamma, self.global_batch, ignore, self.boundary,
                                 self.separation, self.relax)
    if self.separation is not None:
        return _NLLSeparationFn.apply(inputs, targets, self.weight, mode, gamma, self.global_batch, ignore, self.boundary,
                                      self.separation, self.hard if self.training else None)
    if self.hard is not None and self.training:
        return _NLLHardFn.apply(inputs, targets, self.weight, mode, gamma, self.global_batch, ignore, self.boundary, self.hard)
    if self.boundary is not None:
        return _NLLBoundaryFn.apply(inputs, targets, self.weight, mode, gamma, self.global_batch, ignore, self.boundary)
    if ignore is None:
        return _NLLFn.apply(inputs, targets, self.weight, mode, gamma, self.global_batch)
    return _NLLFn.apply(inputs, targets, self.weight, mode, gamma, self.global_batch, ignore)


class CrossEntropyLoss2d(_WeightedLoss):
    """Cross-entropy: weighted NLL of log_softmax over the class axis (reference losses.py:8-25).  ``boundary=(w0, sigma)``: every
    pixel's term is also weighted by ``1 + w0 exp(-d^2 / (2 sigma^2))``, d its distance to the nearest label boundary, made from
    ``targets`` on the device in every call (include/robosat_hip.h; DESIGN.md "Boundary weight"); ``None`` makes today's calls.
    ``hard=fraction`` or ``(fraction, below)``: in training mode, per image only the valid pixels whose cross-entropy is among the
    ``ceil(fraction * V)`` largest, or whose true class has a probability below ``below``, keep their weight (include/robosat_hip.h;
    DESIGN.md "Hard-pixel mining"); with ``boundary`` a kept pixel keeps its boundary weight.  ``None`` makes today's calls.
    ``separation=(ws, sigma)``: ``ws exp(-(d1 + d2)^2 / (2 sigma^2))`` is added to a background pixel's weight, d1 and d2 its distances
    to the two nearest objects (the 4-connected components of the pixels of the classes 1 .. C - 1), so that the narrow gap between
    two neighbouring objects counts (include/robosat_hip.h; DESIGN.md "Separation weight").  It adds onto the boundary plane where
    that is given too, mining takes the sum as its base, and like ``boundary`` it stays on in eval mode.  ``None`` makes today's calls.
    ``relax=R`` (an int in 1..16): boundary label relaxation (Zhu et al., CVPR 2019).  In training mode a pixel's term is
    ``-log sum_{c in S} p_c``, S the classes of the valid pixels within R pixels in x and in y (``rs_label_set_plane``), weighted by
    the class weight of the pixel's own label; labels that are shifted by up to R pixels then cost nothing near an outline
    (include/robosat_hip.h; DESIGN.md "Label relaxation").  ``boundary`` and ``separation`` are made from the strict labels and
    weigh the relaxed terms; in eval mode the criterion makes the strict calls; ``relax`` with ``hard`` is a ``ValueError`` (mining
    would have to rank by the relaxed loss).  ``None`` makes today's calls."""

    def __init__(self, weight=None, ignore_index=None, boundary=None, hard=None, separation=None, relax=None):
        super().__init__(weight, ignore_index)
        self.boundary = _check_boundary(boundary)
        self.separation = _check_separation(separation)
        self.hard = _check_hard(hard)
        self.relax = _check_relax(relax, self.hard)

    def forward(self, inputs, targets):
        return _nll(self, inputs, targets, ops.NLL_CROSS_ENTROPY, 0.0)


class FocalLoss2d(_WeightedLoss):
    """Focal loss, gamma = 2 by default (reference losses.py:28-50); ``boundary``, ``separation`` and ``hard`` as in ``CrossEntropyLoss2d``
    (the pixels are ranked by their cross-entropy: Focal is monotone in the true class's probability, so that is its ranking too);
    ``relax`` as there, with the class set's probability q in place of the true class's: ``-(1 - q)^gamma log q``."""

    def __init__(self, gamma=2, weight=None, ignore_index=None, boundary=None, hard=None, separation=None, relax=None):
        super().__init__(weight, ignore_index)
        self.gamma = gamma
        self.boundary = _check_boundary(boundary)
        self.separation = _check_separation(separation)
        self.hard = _check_hard(hard)
        self.relax = _check_relax(relax, self.hard)

    def forward(self, inputs, targets):
        return _nll(self, inputs, targets, ops.NLL_FOCAL, float(self.gamma))


class mIoULoss2d(_WeightedLoss):
    """Soft mean-IoU loss; like the reference it returns ``max(miou, weighted NLL)`` and back-propagates through
    whichever of the two is larger (reference losses.py:53-83); with ``global_batch`` the choice is made once over the
    data-parallel job's global batch (``_global_batch_miou``)."""

    def forward(self, inputs, targets):
        inputs, targets = _check(inputs, targets)
        ignore = _check_ignore(self.ignore_index, inputs)
        if ignore is None:
            return _MIoUFn.apply(inputs, targets, self.weight, self.global_batch)
        return _MIoUFn.apply(inputs, targets, self.weight, self.global_batch, ignore)


class TverskyLoss2d(_WeightedLoss):
    """The Tversky loss family, a region-overlap loss the reference does not have, with an optional fused cross-entropy term
    (``rs_tversky_sums`` / ``rs_tversky_finalize`` / ``rs_tversky_bwd``; include/robosat_hip.h).

    With p = softmax over the classes and, per segment -- (image, class) with ``per_image``, class over the whole batch without --
    TP = sum of p_c over the pixels of the class, FP = sum of p_c over the others, FN = (pixels of the class) - TP:
    ``TI = (TP + smooth) / (TP + alpha FP + beta FN + smooth)``, the segment's loss ``(1 - TI) ** gamma``, averaged over the classes
    present (``classes="present"``) or over all of them (``"all"``), per image then over the batch or once over the whole batch; plus
    ``ce`` times the cross-entropy weighted by ``weight`` (which weighs that term only).  ``alpha = beta = 0.5`` is Dice (the default),
    ``alpha = beta = 1`` the soft Jaccard, ``beta > alpha`` favours recall (Salehi et al. 2017), ``gamma < 1`` is the focal Tversky loss
    of Abraham & Khan 2019.  With ``global_batch`` the batch-level terms are the data-parallel job's global batch's
    (``_global_batch_tversky``).  It takes neither ``boundary`` nor ``hard``."""

    def __init__(self, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, per_image=True, classes="present", ce=0.0, weight=None,
                 ignore_index=None):
        super().__init__(weight, ignore_index)
        self.alpha, self.beta, self.gamma, self.smooth, self.ce = ops.tversky_params(alpha, beta, gamma, smooth, ce)
        if classes not in ("present", "all"):
            raise ValueError("classes must be \"present\" or \"all\" (got {!r})".format(classes))
        if not isinstance(per_image, bool):
            raise ValueError("per_image must be True or False (got {!r})".format(per_image))
        self.per_image = per_image
        self.classes = classes

    def forward(self, inputs, targets):
        inputs, targets = _check(inputs, targets)
        ignore = _check_ignore(self.ignore_index, inputs)
        params = (self.alpha, self.beta, self.gamma, self.smooth, self.ce)
        return _TverskyFn.apply(inputs, targets, self.weight, params, self.per_image, self.classes, self.global_batch, ignore)


class LovaszLoss2d(nn.Module):
    """The reference's Lovasz hinge variant over the flattened C*H*W vector per image (losses.py:86-119)."""

    def __init__(self, ignore_index=None):
        super().__init__()
        self.ignore_index = ignore_index

    def forward(self, inputs, targets):
        inputs, targets = _check(inputs, targets)
        ignore = _check_ignore(self.ignore_index, inputs)
        if ignore is None:
            return _LovaszFn.apply(inputs, targets)
        return _LovaszFn.apply(inputs, targets, ignore)


class LovaszSoftmax2d(nn.Module):
    """The multi-class Lovasz-Softmax loss of Berman et al. 2018 (arXiv 1705.08790), which the reference's ``LovaszLoss2d``
    cites but does not implement: softmax over the classes of the LOGITS it is given, then per class the Lovasz extension of
    the Jaccard loss over the errors ``|1[y = c] - p_c|``, averaged over the classes present (``classes="present"``) or
    over all of them (``"all"``), per image then over the batch (``per_image=True``) or once over the whole batch."""

    def __init__(self, per_image=True, classes="present", ignore_index=None):
        super().__init__()
        self.ignore_index = ignore_index
        if classes not in ("present", "all"):
            raise ValueError("classes must be \"present\" or \"all\" (got {!r})".format(classes))
        self.per_image = bool(per_image)
        self.classes = classes

    def forward(self, inputs, targets):
        inputs, targets = _check(inputs, targets)
        ignore = _check_ignore(self.ignore_index, inputs)
        if ignore is None:
            return _LovaszSoftmaxFn.apply(inputs, targets, self.per_image, self.classes)
        return _LovaszSoftmaxFn.apply(inputs, targets, self.per_image, self.classes, ignore)


class ClDiceLoss2d(nn.Module):
    """``(1 - weight) * base(inputs, targets) + weight * clDice(inputs, targets)``: the topology loss of Shit et al. (CVPR 2021) on top
    of any of the region and pixel losses above (include/robosat_hip.h).

    Per (image, class) of ``classes`` (indices of non-background classes; ``None`` = all of 1 .. C - 1): P = the softmax plane,
    Y = the 0/1 label plane, S_P and S_Y their soft skeletons after ``iters`` iterations (at least half the widest structure in
    pixels), ``Tprec = (sum S_P Y + smooth) / (sum S_P + smooth)``, ``Tsens = (sum S_Y P + smooth) / (sum S_Y + smooth)`` and the
    term ``1 - 2 Tprec Tsens / (Tprec + Tsens)``, averaged over all N * K pairs: an absent class is not skipped.  Pixels of
    ``ignore_index`` are 0 in both planes and get no gradient.  The divisor depends on the batch size alone, so data-parallel
    ranks with equal batches need no exchange for this term.  ``train()`` / ``eval()`` reach ``base`` (hard-pixel mining and label
    relaxation depend on the mode) because it is a submodule."""

    def __init__(self, base, weight, iters=10, smooth=1.0, classes=None, ignore_index=None):
        super().__init__()
        import math

        if not isinstance(base, nn.Module):
            raise ValueError("base must be a criterion module (got {!r})".format(base))
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0 < weight < 1:
            raise ValueError("weight must be a number with 0 < weight < 1 (got {!r})".format(weight))
        if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= ops.SKELETON_MAX_ITERS:
            raise ValueError("iters must be an integer in 0..{} (got {!r})".format(ops.SKELETON_MAX_ITERS, iters))
        if isinstance(smooth, bool) or not isinstance(smooth, (int, float)) or not math.isfinite(smooth) or smooth < 0:
            raise ValueError("smooth must be a finite number >= 0 (got {!r})".format(smooth))
        if classes is not None:
            classes = tuple(classes)
            if not classes or any(isinstance(k, bool) or not isinstance(k, int) or k < 1 for k in classes) or len(set(classes)) != len(classes):
                raise ValueError("classes must be distinct indices of non-background classes (got {!r})".format(classes))
        self.base = base
        self.cldice_weight, self.iters, self.smooth, self.classes = float(weight), iters, float(smooth), classes
        self.ignore_index = ignore_index

    @property
    def hard(self):
        """``base``'s hard-pixel mining, if it has any: ``rs train`` switches a mining criterion between train and eval mode."""

        return getattr(self.base, "hard", None)

    @property
    def relax(self):
        """``base``'s label relaxation, if it has any: a training device like ``hard``."""

        return getattr(self.base, "relax", None)

    def term(self, inputs, targets):
        """The clDice term alone."""

        inputs, targets = _check(inputs, targets)
        ignore = _check_ignore(self.ignore_index, inputs)
        return _ClDiceFn.apply(inputs, targets, self.iters, self.smooth, self.classes, ignore)

    def forward(self, inputs, targets):
        a = self.cldice_weight
        return (1.0 - a) * self.base(inputs, targets) + a * self.term(inputs, targets)
