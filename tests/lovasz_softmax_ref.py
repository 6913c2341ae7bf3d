"""A float64 restatement of the Lovasz-Softmax loss (Berman, Rannen Triki, Blaschko 2018, arXiv 1705.08790, Algorithm 1 and
eq. 9-12), written from the paper for the tests of ``rs_lovasz_softmax_fwd`` / ``LovaszSoftmax2d``; and inputs whose errors
are far enough apart that their order is unambiguous.

Per segment (image n and class c, or class c over the whole batch): errors ``e = |1[y = c] - p_c|`` sorted descending (a
STABLE sort, so equal errors keep ascending pixel order), ``g`` = the segment's foreground count, the Jaccard loss of the
first r + 1 errors ``J_r = 1 - (g - k_r) / (g + r + 1 - k_r)`` and its increments ``delta``; ``L_s = sum_r e_r delta_r``.
Autograd through the sort's indices (constant) gives the gradient."""

import numpy as np
import torch


def _segment_loss(err, lab):
    order = torch.sort(-err.detach(), stable=True).indices  # descending, ties in ascending position
    e, m = err[order], lab[order]
    g = m.sum()
    k = torch.cumsum(m, 0)
    r = torch.arange(1, e.numel() + 1, dtype=e.dtype)
    jac = 1.0 - (g - k) / (g + r - k)
    delta = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    return (e * delta).sum(), float(g)


def lovasz_softmax(p, y, per_image=True, classes="present", fp32_errors=False):
    """p: float64 probabilities [N, C, H, W] (softmax of the logits, may require grad), y: int64 [N, H, W].
    ``fp32_errors``: the errors take the values fp32 arithmetic gives them (``1 - p`` rounded as a kernel computes it from an
    fp32 p) -- the same numbers, hence the same order and ties, as the kernel's keys; their derivative stays -+1."""

    n, c = p.shape[:2]
    m = torch.nn.functional.one_hot(y, c).permute(0, 3, 1, 2).to(p.dtype)
    err = (m - p).abs()
    if fp32_errors:
        err = err + (err.detach().float().double() - err.detach())

    def mean_over_classes(segments):
        keep = [l for l, g in segments if classes == "all" or g > 0]
        return torch.stack(keep).mean()

    if per_image:
        return torch.stack([mean_over_classes([_segment_loss(err[i, k].reshape(-1), m[i, k].reshape(-1)) for k in range(c)])
                            for i in range(n)]).mean()
    return mean_over_classes([_segment_loss(err[:, k].reshape(-1), m[:, k].reshape(-1)) for k in range(c)])


def softmax_backward(p, grad_p):
    """d loss / d logits from d loss / d p through the softmax Jacobian: p_c (G_c - sum_k p_k G_k)."""

    return p * (grad_p - (p * grad_p).sum(1, keepdim=True))


def mean_iou_loss(pred, y, c, per_image=True):
    """1 - mean IoU over the classes present in the targets (per image, then averaged; or over the whole batch) for a hard
    prediction ``pred`` [N, H, W]: what the Lovasz extension equals at the cube's vertices."""

    def one(pr, t):
        ious = []
        for k in range(c):
            gk = t == k
            if gk.any():
                pk = pr == k
                ious.append(float((gk & pk).sum()) / float((gk | pk).sum()))
        return 1.0 - sum(ious) / len(ious)

    if per_image:
        return sum(one(pred[i], y[i]) for i in range(pred.shape[0])) / pred.shape[0]
    return one(pred, y)


def separated_inputs(n, c, h, w, seed, absent_last_in_first=True, K=90000):
    """(logits float64 [N, C, H, W] = log p, targets int64 [N, H, W]) with every segment's float64 errors on a grid of 1 / K:
    distinct, hence at least 1 / K apart, in every segment of either form.

    Each pixel's wrong classes get probabilities (C a + 1) / K with the a's distinct over the whole batch (pixel i, in a
    shuffled order, takes a = pi(i) + M j, j = 0 .. C-2 dealt to its wrong classes in a random order, M = N*H*W); its class
    gets the rest.  A class's background errors are then distinct and = 1 (mod C); its foreground errors 1 - p_y = the sum
    of the pixel's wrong-class numerators, distinct because sum_j a = (C-1) pi(i) + const, and = C-1 (mod C) -- apart from
    the background ones when C >= 3 (for C = 2 both are wrong-class numerators, all distinct).  Image 0 leaves out the last
    class (when asked), so that "present" and "all" differ."""

    rng = np.random.default_rng(seed)
    M = n * h * w
    y = rng.integers(0, c, size=(n, h, w))
    if absent_last_in_first:
        y[0] = rng.integers(0, c - 1, size=(h, w))
    y = y.reshape(-1)
    perm = rng.permutation(M)
    num = np.zeros((M, c), dtype=np.int64)
    for i in range(M):
        wrong = [k for k in range(c) if k != y[i]]
        rng.shuffle(wrong)
        for j, k in enumerate(wrong):
            num[i, k] = c * (perm[i] + M * j) + 1
        num[i, y[i]] = K - num[i].sum()
    assert num.min() >= 1, "K too small for this shape"
    p = torch.from_numpy(num).double().div(K).reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()
    return p.log(), torch.from_numpy(y.reshape(n, h, w)).long()


def min_error_gap(p, y, per_image):
    """The smallest distance between two float64 errors of one segment."""

    c = p.shape[1]
    m = torch.nn.functional.one_hot(y, c).permute(0, 3, 1, 2).to(p.dtype)
    err = (m - p).abs()
    segs = [err[i, k] for i in range(p.shape[0]) for k in range(c)] if per_image else [err[:, k] for k in range(c)]
    return min(float(torch.sort(s.reshape(-1)).values.diff().min()) for s in segs)
