"""Float64 reference of the five losses with an ignore label, BY COMPACTION, and the inputs of its tests (TEST INFRASTRUCTURE ONLY).

The definition ("Ignore label"): the loss is the existing definition evaluated on the valid pixels only, as if the
ignored pixels had been cut out of each image and the rest packed together in their (n, h, w) order.  So the reference does
exactly that: per image it gathers the valid pixels into a ``[1, C, 1, K]`` tensor, calls the oracle's own criterion on it
(``oracle.robosat_ref``; ``lovasz_softmax_ref.lovasz_softmax`` for the fifth loss) and combines the images as the definition says:

  * CrossEntropy / Focal: ``sum_i D_i L_i / sum_i D_i`` with ``D_i`` the image's sum of target weights (the oracle's own
    denominator), 0 where ``sum_i D_i == 0``;
  * mIoU: the soft-IoU term is the mean over the N images of the image's term (an image's term is itself a mean over its C
    classes, so this is the mean over C*N ratios), an image with no valid pixel counting 0 (ratio 1 in every class); the NLL term
    is the CrossEntropy combination; the result is Python's ``max(miou, nll)``.  The oracle's ``miou2d`` returns that maximum
    only, so an image's two terms are taken apart: the soft-IoU term is ``_miou_term``, the oracle's expression for it on the
    caller's graph, the NLL term ``R.cross_entropy2d``.  tests/test_ignore_cpu.py checks that ``_miou_term`` equals
    ``losses_ref.miou_terms64`` (pinned to the oracle by tests/test_losses_ref_cpu.py) and that the combination IS the oracle's
    ``miou2d`` when nothing is ignored;
  * Lovasz (hinge) and LovaszSoftmax per image: ``sum_i L_i / N``, an image with no valid pixel counting 0;
  * LovaszSoftmax flattened: ONE call on the valid pixels of the whole batch, 0 where there is none.

Everything hangs off one float64 leaf, so autograd scatters the gradient back with zeros at the ignored pixels.

The input builders assert the property their name claims -- on the labels and on this reference, never on the code under test."""

import contextlib
import functools

import torch

import losses_ref as L
import lovasz_softmax_ref as LS
from oracle import robosat_ref as R

IGNORE = 255

# (N, C, H, W) of the issue's table, each the smallest shape that reaches its edge of the kernels
SHAPES = [
    (2, 2, 5, 7),     # HW % 4 != 0: the scalar key kernels
    (3, 4, 16, 16),   # the 4-pixel vector path, one scan block
    (2, 3, 33, 32),   # HW = 1056 > the 1024-entry scan chunk: the tail crosses a scan block
    (1, 2, 96, 96),   # hinge P = 18 432 spans three 8192-key sort tiles; a softmax segment spans two
    (2, 8, 9, 9),     # eight classes
]
PATTERNS = ["none", "random30", "one_in_four", "all_but_one", "image0_all", "all", "class_vanishes"]
VANISHING_CLASS = 1


def cases():
    """(shape, pattern) pairs: every pattern at every shape; ``image0_all`` needs a second image."""

    return [(s, p) for s in SHAPES for p in PATTERNS if not (p == "image0_all" and s[0] < 2)]


def case_id(case):
    return "{}-{}".format("x".join(map(str, case[0])), case[1])


def ignored_mask(pattern, targets, seed=0):
    """bool [N, H, W], True where the pixel is ignored; asserts what the pattern's name says."""

    n, h, w = targets.shape
    g = torch.Generator().manual_seed(1000 + seed)
    if pattern == "none":
        m = torch.zeros(n, h, w, dtype=torch.bool)
        assert not m.any()
    elif pattern == "random30":
        m = torch.rand(n, h, w, generator=g) < 0.3
        assert 0.15 < float(m.float().mean()) < 0.45 and all(0 < int(m[i].sum()) < h * w for i in range(n))
    elif pattern == "one_in_four":
        m = (torch.arange(n * h * w) % 4 == 3).view(n, h, w)
        groups = m.view(-1)[: (n * h * w) // 4 * 4].view(-1, 4)
        assert bool((groups.sum(1) == 1).all())  # every aligned group of four label entries (16 bytes of the byte raster) is mixed
    elif pattern == "all_but_one":
        m = torch.ones(n, h * w, dtype=torch.bool)
        for i in range(n):
            m[i, int(torch.randint(0, h * w, (1,), generator=g))] = False
        m = m.view(n, h, w)
        assert all(int((~m[i]).sum()) == 1 for i in range(n))
    elif pattern == "image0_all":
        assert n >= 2
        m = torch.zeros(n, h, w, dtype=torch.bool)
        m[0] = True
        assert bool(m[0].all()) and not m[1:].any()
    elif pattern == "all":
        m = torch.ones(n, h, w, dtype=torch.bool)
        assert bool(m.all())
    elif pattern == "class_vanishes":
        m = targets == VANISHING_CLASS
        assert 0 < int(m.sum()) < n * h * w and not ((targets == VANISHING_CLASS) & ~m).any()
    else:
        raise KeyError(pattern)
    return m


def with_ignored(targets, mask, ignore=IGNORE):
    out = targets.clone()
    out[mask] = ignore
    assert bool(((out == ignore) == mask).all())
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _float64_default():
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(before)


def _compact(x, targets, i, ignore):
    """Image i's valid pixels: (logits [1, C, 1, K] as a view of the leaf ``x``, labels [1, 1, K]), in (h, w) order."""

    keep = (targets[i] != ignore).view(-1)
    c = x.shape[1]
    return x[i].reshape(c, -1)[:, keep].reshape(1, c, 1, -1), targets[i].view(-1)[keep].view(1, 1, -1)


def _weighted_mean(terms):
    """sum D_i L_i / sum D_i over (L_i, D_i) pairs, 0 (of no graph) where there is nothing to divide by."""

    den = sum(d for _, d in terms)
    if not terms or den == 0:
        return torch.zeros((), dtype=torch.float64)
    return sum(l * d for l, d in terms) / den


def _nll_terms(name, x, targets, weight, gamma, ignore):
    terms = []
    for i in range(x.shape[0]):
        xi, ti = _compact(x, targets, i, ignore)
        if ti.numel() == 0:
            continue
        d = float(ti.numel()) if weight is None else float(weight[ti.view(-1)].sum())
        if d == 0:
            continue  # (the oracle's own 0 / 0; the definition gives such an image no say)
        li = R.cross_entropy2d(xi, ti, weight=weight) if name == "CrossEntropy" else R.focal2d(xi, ti, gamma=gamma, weight=weight)
        terms.append((li, d))
    return terms


def loss64(name, logits, targets, ignore=IGNORE, weight=None, gamma=2, per_image=True, classes="present"):
    """(loss as a Python float, d loss / d logits as float64 [N, C, H, W] with zeros at the ignored pixels, extras) of criterion
    ``name`` ("CrossEntropy" | "Focal" | "mIoU" | "Lovasz" | "LovaszSoftmax") by compaction.  extras: for mIoU the two terms."""

    n, c = logits.shape[:2]
    x = logits.double().clone().requires_grad_(True)
    w = None if weight is None else weight.double()
    extras = {}
    if name in ("CrossEntropy", "Focal"):
        loss = _weighted_mean(_nll_terms(name, x, targets, w, gamma, ignore))
    elif name == "mIoU":
        mious = []
        for i in range(n):
            xi, ti = _compact(x, targets, i, ignore)
            if ti.numel():
                # (miou_terms64 makes a leaf of its own from its argument: evaluate it on the graph of x instead)
                mious.append(_miou_term(xi, ti, c))
        miou = (sum(mious) if mious else torch.zeros((), dtype=torch.float64)) / n
        nll = _weighted_mean(_nll_terms("CrossEntropy", x, targets, w, gamma, ignore))
        extras = {"miou": float(miou.detach()), "nll": float(nll.detach())}
        loss = max(miou, nll)  # Python's max, as in the oracle: nll only where nll > miou
    elif name == "Lovasz":
        parts = []
        for i in range(n):
            xi, ti = _compact(x, targets, i, ignore)
            if ti.numel():
                with _float64_default():  # (the oracle's one-hot mask takes the default dtype: its Jaccard curve in float64 too)
                    parts.append(R.lovasz2d(xi, ti))
        loss = (sum(parts) if parts else torch.zeros((), dtype=torch.float64)) / n
    elif name == "LovaszSoftmax":
        if per_image:
            parts = []
            for i in range(n):
                xi, ti = _compact(x, targets, i, ignore)
                if ti.numel():
                    parts.append(LS.lovasz_softmax(torch.softmax(xi, 1), ti, per_image=True, classes=classes))
            loss = (sum(parts) if parts else torch.zeros((), dtype=torch.float64)) / n
        else:
            keep = (targets != ignore)
            if keep.any():
                xa = x.permute(1, 0, 2, 3).reshape(c, -1)[:, keep.view(-1)].reshape(1, c, 1, -1)  # (n, h, w) order
                ta = targets.view(-1)[keep.view(-1)].view(1, 1, -1)
                loss = LS.lovasz_softmax(torch.softmax(xa, 1), ta, per_image=False, classes=classes)
            else:
                loss = torch.zeros((), dtype=torch.float64)
    else:
        raise KeyError(name)
    if loss.requires_grad:
        loss.backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return float(loss.detach()), grad.detach(), extras


def _miou_term(xi, ti, c):
    """The soft-IoU term of one compacted image on the caller's graph: ``losses_ref.miou_terms64``'s expression (the oracle's
    sums).  Checked against that helper, and through it the oracle, in tests/test_ignore_cpu.py."""

    softs = torch.softmax(xi, dim=1)
    masks = R.onehot(ti, c).double()
    inter = (softs * masks).sum((2, 3))
    union = (softs + masks - softs * masks).sum((2, 3))
    return 1.0 - (inter / union).mean()


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------

def _seed(shape, pattern):
    return sum(shape) * 7 + PATTERNS.index(pattern)


@functools.lru_cache(maxsize=None)
def random_inputs(shape, pattern, confident=False):
    """(logits fp32, labels with the pattern's pixels set to IGNORE, ignored mask, weight) from ``losses_ref.random_case``:
    the plain logits (scale 2) put mIoULoss2d on its NLL branch; ``confident`` (noise 0.5 and a margin on the labelled class) on
    its soft-IoU branch where the pattern leaves one -- with half the images empty the soft-IoU term halves and the NLL term
    stays.  The margin is the first of 4, 2, 1, 8 at which the two terms of the REFERENCE are >= 1e-2 apart with and without the
    class weights (``assert_miou_terms_apart``), so that no rounding can flip the branch; the plain logits must be so as they are."""

    n, c, h, w = shape
    seed = _seed(shape, pattern)
    for margin in ((4.0, 2.0, 1.0, 8.0) if confident else (0.0,)):
        logits, targets, weight = (L.random_case(n, c, h, w, seed, scale=0.5, margin=margin) if confident
                                   else L.random_case(n, c, h, w, seed))
        mask = ignored_mask(pattern, targets, seed)
        labels = with_ignored(targets, mask)
        terms = [loss64("mIoU", logits, labels, weight=wt)[2] for wt in (None, weight)]
        if bool(mask.all()) or all(abs(t["miou"] - t["nll"]) >= 1e-2 for t in terms):
            break
    for t in terms:
        assert_miou_terms_apart(t, mask)
    return logits, labels, mask, weight


def separation_grid(n, c, h, w):
    """The K of ``separated_inputs`` for a shape: twice the largest sum of wrong-class numerators a pixel can get (so that K is
    never "too small" there), at most the helper's own 90000.  With the default K a SMALL batch gets wrong-class probabilities of
    at most a few 1e-3 everywhere -- 70 pixels at 2 classes: at most 141 / 90000 -- and the gradient through the softmax,
    p_c (G_c - sum_k p_k G_k), is then a difference of nearly equal fp32 numbers that no fp32 kernel holds to 1e-5 of its largest
    entry (true of the entry point without an ignore label on the same input: pattern ``none`` is bit-equal to it).  A grid of
    this size spreads the probabilities over (0, 1/2] as the helper's default does at the shapes its own tests use; the errors
    stay at least 1 / K >= 1 / 90000 apart."""

    m = n * h * w
    most = c * ((m - 1) * (c - 1) + m * (c - 1) * (c - 2) // 2) + (c - 1)
    return min(90000, 2 * most)


@functools.lru_cache(maxsize=None)
def separated_softmax_inputs(shape, pattern):
    """The same for the Lovasz-Softmax cases, from ``lovasz_softmax_ref.separated_inputs``: every segment's errors at least
    1 / 90000 apart, so that the order is unambiguous -- before and, a subset staying as far apart, after compaction.  Asserts the
    gap on the fp32 logits the kernel sees."""

    n, c, h, w = shape
    seed = _seed(shape, pattern)
    x64, targets = LS.separated_inputs(n, c, h, w, seed=seed, absent_last_in_first=n > 1, K=separation_grid(n, c, h, w))
    logits = x64.float()
    for per_image in (True, False):
        assert LS.min_error_gap(torch.softmax(logits.double(), 1), targets, per_image) >= 1e-5
    mask = ignored_mask(pattern, targets, seed)
    return logits, with_ignored(targets, mask), mask


def other_logits_at(logits, mask, seed=99):
    """``logits`` with other finite random values in every class plane of the ignored pixels, and the same bits elsewhere."""

    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(logits.shape, generator=g) * 5.0
    m = mask.unsqueeze(1).expand_as(logits)
    out = torch.where(m, noise, logits)
    assert torch.equal(out[~m], logits[~m]) and bool(torch.isfinite(out).all())
    assert not mask.any() or not torch.equal(out[m], logits[m])
    return out


def assert_miou_terms_apart(extras, mask):
    """As ``losses_ref.assert_miou_branch_is_safe``: the two terms are >= 1e-2 apart on the reference, so that no rounding flips
    the branch.  With no valid pixel at all both terms are exactly 0, and so are both gradients (as at C = 1 there)."""

    if bool(mask.all()):
        assert extras["miou"] == 0.0 and extras["nll"] == 0.0
        return
    assert abs(extras["miou"] - extras["nll"]) >= 1e-2, extras
