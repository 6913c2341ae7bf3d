"""Float64 reference of the Tversky loss family with a cross-entropy term (TEST INFRASTRUCTURE ONLY): the definition of
include/robosat_hip.h (``rs_tversky_*``) and DESIGN.md section 7g in float64 torch, the gradient from autograd.  It shares no code with
the kernels; tests/test_tversky_cpu.py ties it to the original project's soft IoU (``losses_ref.miou_terms64``) and to
``losses_ref.nll_family64``.

The seeded builders return float32 CPU tensors that depend only on their arguments and assert, on this reference, the property their
case is named after."""

import torch
import torch.nn.functional as F

import losses_ref as L

PARAMS = [(0.5, 0.5, 1.0, 1.0), (0.3, 0.7, 0.75, 1.0), (0.7, 0.3, 2.0, 0.0), (1.0, 1.0, 1.0, 0.0)]  # (alpha, beta, gamma, smooth)
SHAPES = [(1, 1, 5), (2, 1, 300), (2, 300, 1), (3, 33, 31), (2, 129, 129)]  # (N, H, W)
IGNORE = 255


def segment_hot(targets, c):
    """bool [N, C, H, W]: the pixel carries the class."""

    return torch.stack([targets == k for k in range(c)], 1)


def segment_sums(x, targets, per_image=True, ignore=None):
    """(TP, SP, cnt) as float64 tensors [N, C] (per image) or [C], over the valid pixels, from float64 logits ``x``."""

    c = x.shape[1]
    valid = torch.ones_like(targets, dtype=torch.bool) if ignore is None else targets != ignore
    p = F.softmax(x, dim=1) * valid.unsqueeze(1).double()
    hot = torch.stack([(targets == k) & valid for k in range(c)], 1).double()
    dims = (2, 3) if per_image else (0, 2, 3)
    return (p * hot).sum(dims), p.sum(dims), hot.sum(dims)


def tversky_index(tp, sp, cnt, alpha, beta, smooth):
    den = tp + alpha * (sp - tp) + beta * (cnt - tp) + smooth
    safe = torch.where(den > 0, den, torch.ones_like(den))
    return torch.where(den > 0, (tp + smooth) / safe, torch.ones_like(den))


def tversky_term(x, targets, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, per_image=True, classes="present", ignore=None):
    """T of the definition as a 0-dim float64 tensor that depends on ``x``."""

    tp, sp, cnt = segment_sums(x, targets, per_image, ignore)
    u = (1.0 - tversky_index(tp, sp, cnt, alpha, beta, smooth)).clamp(min=0.0)
    # (u ** gamma by autograd: at u > 0 the definition's derivative; the cases keep u away from 0)
    l = u if gamma == 1.0 else torch.where(u > 0, u.clamp(min=1e-300) ** gamma, torch.zeros_like(u))
    if classes == "present":
        counts = cnt > 0
    else:
        counts = (cnt.sum(-1, keepdim=True) > 0).expand_as(cnt)
    k = counts.double().sum(-1)
    per_group = torch.where(k > 0, (l * counts.double()).sum(-1) / k.clamp(min=1.0), torch.zeros_like(k))
    return per_group.mean() if per_image else per_group


def ce_term(x, targets, weight=None, ignore=None):
    """(numerator, denominator) of the pixel term as 0-dim float64 tensors."""

    c = x.shape[1]
    valid = torch.ones_like(targets, dtype=torch.bool) if ignore is None else targets != ignore
    t = torch.where(valid, targets, torch.zeros_like(targets))
    w = torch.ones(c, dtype=torch.float64) if weight is None else weight.double()
    wp = w[t] * valid.double()
    nll = -F.log_softmax(x, dim=1).gather(1, t.unsqueeze(1)).squeeze(1)
    return (wp * nll).sum(), wp.sum()


def ref64(logits, targets, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, per_image=True, classes="present", ce=0.0, weight=None,
          ignore=None):
    """(loss as a float, d loss / d logits float64, T as a float) of the definition in float64.  Logits under ignored pixels may hold
    anything: they are replaced by zeros before the evaluation, and their gradient is zero."""

    x = logits.double().clone()
    if ignore is not None:
        x = torch.where((targets == ignore).unsqueeze(1), torch.zeros_like(x), x)
    x.requires_grad_(True)
    t = tversky_term(x, targets, alpha, beta, gamma, smooth, per_image, classes, ignore)
    loss = t
    if ce > 0:
        num, den = ce_term(x, targets, weight, ignore)
        if float(den) > 0:
            loss = loss + ce * num / den
    if loss.requires_grad:
        loss.backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return float(loss.detach()), grad, float(t.detach())


def ref32(logits, targets, **kw):
    """The definition evaluated in float32 torch (what the number format alone costs): (loss, gradient)."""

    x = logits.float().clone().requires_grad_(True)
    alpha, beta, gamma, smooth = (kw.get(k, d) for k, d in (("alpha", 0.5), ("beta", 0.5), ("gamma", 1.0), ("smooth", 1.0)))
    c = x.shape[1]
    p = F.softmax(x, dim=1)
    hot = F.one_hot(targets, c).permute(0, 3, 1, 2).float()
    dims = (2, 3) if kw.get("per_image", True) else (0, 2, 3)
    tp, sp, cnt = (p * hot).sum(dims), p.sum(dims), hot.sum(dims)
    l = (1 - (tp + smooth) / (tp + alpha * (sp - tp) + beta * (cnt - tp) + smooth)).clamp(min=0) ** gamma
    counts = (cnt > 0).float() if kw.get("classes", "present") == "present" else torch.ones_like(cnt)
    loss = ((l * counts).sum(-1) / counts.sum(-1)).mean()
    if kw.get("ce", 0.0) > 0:
        loss = loss + kw["ce"] * F.cross_entropy(x, targets, weight=kw.get("weight"))
    loss.backward()
    return float(loss.detach()), x.grad


def compare(got_loss, got_grad, want_loss, want_grad, what=""):
    """The project's bars for a loss with mIoU's coefficient structure: ``LOSS_BAR`` and ``MIOU_GRAD_BAR`` (tests/losses_ref.py)."""

    return L.compare("mIoU", got_loss, got_grad, want_loss, want_grad, what="Tversky " + what)


def random_case(n, c, h, w, seed=0):
    """Random logits of scale 2 (1 - TI stays far from 0: the kink is not in play), uniform labels, weight = rand(C) + 0.2."""

    return L.random_case(n, c, h, w, seed=500 + seed)


def with_ignored(targets, seed=0, share=1.0 / 3.0, label=IGNORE):
    """``targets`` with about ``share`` of the pixels relabelled ``label`` (seeded)."""

    g = torch.Generator().manual_seed(900 + seed)
    out = targets.clone()
    out[torch.rand(targets.shape, generator=g) < share] = label
    return out


def absent_class_case(seed=0, c=3, h=33, w=31):
    """Two images; class c-1 is absent from image 0 and present in image 1.  Asserts that "present" and "all" differ by more than 100
    loss bars on the reference, per image and over the batch."""

    logits, targets, weight = random_case(2, c, h, w, seed=40 + seed)
    targets[0][targets[0] == c - 1] = 0
    assert int((targets[0] == c - 1).sum()) == 0 and int((targets[1] == c - 1).sum()) > 0
    a = ref64(logits, targets, classes="present")[0]
    b = ref64(logits, targets, classes="all")[0]
    assert abs(a - b) > 100 * L.LOSS_BAR, (a, b)
    return logits, targets, weight


def shard_case(seed=0, c=3, h=17, w=19):
    """A batch of 4 whose two halves have different class mixes: images 0, 1 are mostly class 0 with a little of class 1, images 2, 3
    mostly class 2 with some of class 1.  Returns (logits, targets, weight)."""

    g = torch.Generator().manual_seed(700 + seed)
    logits = torch.randn(4, c, h, w, generator=g) * 2.0
    r = torch.rand(4, h, w, generator=g)
    targets = torch.zeros(4, h, w, dtype=torch.int64)
    targets[:2][r[:2] < 0.1] = 1
    targets[2:] = 2
    targets[2:][r[2:] < 0.4] = 1
    weight = torch.tensor([0.5, 2.0, 1.0])[:c].clone()
    return logits, targets, weight


def two_shard_reference(logits, targets, weight, per_image, **kw):
    """On the float64 reference: (loss, gradient) of the single evaluation over the batch of 4, and the mean of the two un-exchanged
    per-shard losses with the two per-shard gradients laid side by side and halved (what averaging ranks without an exchange gives)."""

    whole = ref64(logits, targets, per_image=per_image, weight=weight, **kw)
    parts = [ref64(logits[s], targets[s], per_image=per_image, weight=weight, **kw) for s in (slice(0, 2), slice(2, 4))]
    naive_loss = 0.5 * (parts[0][0] + parts[1][0])
    naive_grad = 0.5 * torch.cat([parts[0][1], parts[1][1]], 0)
    return (whole[0], whole[1]), (naive_loss, naive_grad)


def exchanged64(logits, targets, weight, per_image, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, classes="present", ce=0.0):
    """The data-parallel recipe on the float64 reference, two shards of 2 images: per shard the sums; batch form -- both shards see the
    added sums, report the global loss, and their gradients are taken through their own pixels times world; per image -- only the CE
    denominator is added and divided by world.  Returns (mean of the two losses, the two gradients side by side, halved)."""

    world = 2
    xs = [logits[s].double().clone().requires_grad_(True) for s in (slice(0, 2), slice(2, 4))]
    ts = [targets[s] for s in (slice(0, 2), slice(2, 4))]
    ces = [ce_term(x, t, weight) for x, t in zip(xs, ts)]
    den_all = sum(float(d.detach()) for _, d in ces)
    losses, grads = [], []
    if per_image:
        for r in range(world):
            loss = tversky_term(xs[r], ts[r], alpha, beta, gamma, smooth, True, classes)
            if ce > 0:
                loss = loss + ce * ces[r][0] / (den_all / world)
            loss.backward()
            losses.append(float(loss.detach()))
            grads.append(xs[r].grad)
        return sum(losses) / world, torch.cat(grads, 0) / world
    # batch form: the sums of the other rank arrive as constants
    sums = [segment_sums(x, t, False) for x, t in zip(xs, ts)]
    for r in range(world):
        o = 1 - r
        tp, sp, cnt = (sums[r][k] + sums[o][k].detach() for k in range(3))
        u = (1.0 - tversky_index(tp, sp, cnt, alpha, beta, smooth)).clamp(min=0.0)
        l = u if gamma == 1.0 else u.clamp(min=1e-300) ** gamma
        counts = (cnt > 0) if classes == "present" else torch.ones_like(cnt, dtype=torch.bool)
        loss = (l * counts.double()).sum() / counts.double().sum()
        if ce > 0:
            loss = loss + ce * (ces[r][0] + ces[o][0].detach()) / den_all
        (loss * world).backward(retain_graph=True)
        losses.append(float(loss.detach()))
        grads.append(xs[r].grad)
    return sum(losses) / world, torch.cat(grads, 0) / world
