"""Float64 reference, seeded inputs and the one comparison of the per-pixel loss tests (TEST INFRASTRUCTURE ONLY).

The reference is ``oracle.robosat_ref.cross_entropy2d / focal2d / miou2d`` evaluated on ``logits.double()`` and
``weight.double()`` with the gradient from autograd: independent of the kernels and of ``Metrics``, and pinned to the unmodified
reference by tests/test_oracle_pin.py.  The builders return float32 CPU tensors that depend only on their arguments; each one
asserts -- on the float64 reference, never on the code under test -- the property its case is named after.  ``compare`` holds
the project's bars (tests/test_gpu_train_ops.py: ``test_losses_match_reference_golden``, ``test_miou_both_branches_vs_oracle``)
and is used by the CPU tests (tests/test_losses_ref_cpu.py) and the GPU tests (tests/test_gpu_losses.py) alike.

``nll_family64`` and ``miou_terms64`` restate the same sums with a per-pixel multiplicity / a per-pixel mask: they exist to
show what a dropped or doubled pixel does to the answer (and agree with the reference when nothing is dropped, which
tests/test_losses_ref_cpu.py checks)."""

import torch
import torch.nn.functional as F

from oracle import robosat_ref as R

LOSS_BAR = 2e-5  # |got - want| <= LOSS_BAR * max(1, |want|)
GRAD_BAR = 2e-4  # max |got - want| <= GRAD_BAR * max(1e-6, max |want|)
MIOU_GRAD_BAR = 1e-3

CRITERIA = ("CrossEntropy", "Focal", "mIoU")


def grad_bar(name):
    return MIOU_GRAD_BAR if name == "mIoU" else GRAD_BAR


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the float64 reference ------------------------------------------------------------------------------------------------

def _ref_call(name, x, targets, weight, gamma):
    if name == "CrossEntropy":
        return R.cross_entropy2d(x, targets, weight=weight)
    if name == "Focal":
        return R.focal2d(x, targets, gamma=gamma, weight=weight)
    if name == "mIoU":
        return R.miou2d(x, targets, weight=weight)
    raise KeyError(name)


def ref64(name, logits, targets, weight=None, gamma=2):
    """(loss as a Python float, d loss / d logits as a float64 tensor) of the oracle's criterion ``name`` in float64."""

    x = logits.double().clone().requires_grad_(True)
    w = None if weight is None else weight.double()
    loss = _ref_call(name, x, targets, w, gamma)
    loss.backward()
    return float(loss.detach()), x.grad


def ref32(name, logits, targets, weight=None, gamma=2):
    """The same in float32: what the oracle itself gives at the kernels' precision."""

    x = logits.float().clone().requires_grad_(True)
    loss = _ref_call(name, x, targets, weight, gamma)
    loss.backward()
    return float(loss.detach()), x.grad


def nll_family64(name, logits, targets, weight=None, gamma=2, mult=None):
    """CrossEntropy / Focal in float64 as sum_p m_p w[t_p] l_p / sum_p m_p w[t_p], ``mult`` [N,H,W] = m_p (default 1): a
    dropped pixel is m_p = 0, a doubled one m_p = 2.  Returns (loss, gradient, sum_p m_p w[t_p])."""

    x = logits.double().clone().requires_grad_(True)
    logp = F.log_softmax(x, dim=1)
    if name == "Focal":
        logp = (1 - F.softmax(x, dim=1)) ** gamma * logp
    per_pixel = -logp.gather(1, targets.unsqueeze(1)).squeeze(1)
    w = torch.ones(logits.shape[1], dtype=torch.float64) if weight is None else weight.double()
    wp = w[targets] if mult is None else w[targets] * mult.double()
    loss = (wp * per_pixel).sum() / wp.sum()
    loss.backward()
    return float(loss.detach()), x.grad, float(wp.sum())


def miou_terms64(logits, targets, weight=None, keep=None):
    """(soft-IoU term, NLL term) of mIoULoss2d in float64 as 0-dim tensors of one graph; ``keep`` [N,H,W] bool leaves pixels
    out of the soft-IoU sums (all kept by default).  Returns (miou, nll, x) with ``x`` the leaf the terms depend on."""

    n, c, h, w = logits.shape
    x = logits.double().clone().requires_grad_(True)
    k = torch.ones(n, h, w, dtype=torch.float64) if keep is None else keep.double()
    softs = F.softmax(x, dim=1)
    masks = R.onehot(targets, c).double()
    inter = (softs * masks * k.unsqueeze(1)).sum((2, 3))
    union = ((softs + masks - softs * masks) * k.unsqueeze(1)).sum((2, 3))
    miou = 1.0 - (inter / union).mean()
    nll = F.nll_loss(F.log_softmax(x, dim=1), targets, weight=None if weight is None else weight.double())
    return miou, nll, x


def miou_branch64(logits, targets, weight=None):
    """("miou" | "nll", |miou - nll|) on the float64 reference: the branch Python's max(miou, nll) returns."""

    miou, nll, _ = miou_terms64(logits, targets, weight)
    miou, nll = float(miou.detach()), float(nll.detach())
    return ("nll" if nll > miou else "miou"), abs(miou - nll)


# ---- the comparison -------------------------------------------------------------------------------------------------------

def distances(got_loss, got_grad, want_loss, want_grad):
    """(loss distance in units of max(1, |want|), gradient distance in units of the largest wanted entry) -- the two
    quantities the project's bars bound."""

    dl = abs(float(got_loss) - float(want_loss)) / max(1.0, abs(float(want_loss)))
    want = want_grad.double()
    scale = max(1e-6, float(want.abs().max()))
    dg = float((got_grad.double() - want).abs().max()) / scale
    return dl, dg


def compare(name, got_loss, got_grad, want_loss, want_grad, what="", record=None):
    """Asserts the project's bars for criterion ``name`` and returns (loss distance, gradient distance).  NaN fails.  The
    distances are printed, and kept in ``record[name]`` as running maxima when a dict is given."""

    assert tuple(got_grad.shape) == tuple(want_grad.shape), (what, got_grad.shape, want_grad.shape)
    dl, dg = distances(got_loss, got_grad, want_loss, want_grad)
    print("{} {}: loss {!r} want {!r} distance {:.2e} (bar {:.0e}); gradient distance {:.2e} (bar {:.0e})".format(
        name, what, float(got_loss), float(want_loss), dl, LOSS_BAR, dg, grad_bar(name)))
    if record is not None and dl == dl and dg == dg:
        old = record.get(name, (0.0, 0.0))
        record[name] = (max(old[0], dl), max(old[1], dg))
    assert bool(torch.isfinite(got_grad).all()), "{} {}: gradient not finite".format(name, what)
    assert dl <= LOSS_BAR, "{} {}: loss {!r} want {!r}: distance {:.3e} > {:.0e}".format(name, what, got_loss, want_loss, dl, LOSS_BAR)
    assert dg <= grad_bar(name), "{} {}: gradient distance {:.3e} > {:.0e}".format(name, what, dg, grad_bar(name))
    return dl, dg


# ---- seeded inputs --------------------------------------------------------------------------------------------------------

def random_case(n, c, h, w, seed, scale=2.0, weight="rand", margin=0.0):
    """logits = randn * scale + margin * onehot(target), labels uniform over the classes, weight = rand(C) + 0.2 ("rand"),
    None, or a given tensor."""

    g = _gen(seed)
    logits = torch.randn(n, c, h, w, generator=g) * scale
    targets = torch.randint(0, c, (n, h, w), generator=g)
    if margin:
        logits = logits + margin * R.onehot(targets, c)
    if isinstance(weight, str):
        weight = torch.rand(c, generator=g) + 0.2
    return logits, targets, weight


def class_count_case(c, confident=False):
    """N = 3, H x W = 7 x 9 at C classes; ``confident`` (noise 0.5, margin 4) puts mIoULoss2d on its soft-IoU branch, the plain
    random logits (scale 2) on its NLL branch."""

    return random_case(3, c, 7, 9, seed=10 + c, scale=0.5, margin=4.0) if confident else random_case(3, c, 7, 9, seed=10 + c)


def shape_case(n, c, h, w, confident=False):
    return random_case(n, c, h, w, seed=100 + c, scale=0.5, margin=4.0) if confident else random_case(n, c, h, w, seed=100 + c)


def assert_miou_branch_is_safe(logits, targets, weight, branch=None):
    """Every mIoU case keeps its two terms >= 1e-2 apart on the float64 reference (at C = 1 both are exactly 0 and so are both
    gradients), so that no rounding difference can flip the branch."""

    got, gap = miou_branch64(logits, targets, weight)
    if logits.shape[1] > 1:
        assert gap >= 1e-2, (got, gap)
        assert branch is None or got == branch, (got, branch)
    return got, gap


SHAPES = [(1, 1, 5), (2, 1, 300), (2, 300, 1), (2, 129, 129), (1, 513, 513), (3, 297, 297)]  # (N, H, W) of the issue's table


def weight_cases(c, targets):
    """{"none": None, "zero": one PRESENT class at exactly 0, "rare1e3": 1e3 on the rarest present class}."""

    counts = torch.bincount(targets.view(-1), minlength=c)
    present = [k for k in range(c) if counts[k] > 0]
    assert len(present) >= 2
    zero = torch.linspace(0.5, 1.5, c)
    zero[present[-1]] = 0.0
    rare = torch.ones(c)
    rare[min(present, key=lambda k: int(counts[k]))] = 1e3
    return {"none": None, "zero": zero, "rare1e3": rare}


def rare_class_case(n, c, h, w, seed):
    """A random case whose class c-1 occurs on about 1 pixel in 200 (the class ``weight_cases`` then weighs 1e3)."""

    g = _gen(seed)
    logits = torch.randn(n, c, h, w, generator=g) * 2.0
    targets = torch.randint(0, c - 1, (n, h, w), generator=g)
    rare = torch.rand(n, h, w, generator=g) < 0.005
    targets[rare] = c - 1
    assert 0 < int(rare.sum()) < n * h * w // 50
    return logits, targets


def unsaturated_case(n, c, h, w, seed):
    """Unit-scale logits for gamma in (0, 1): the reference's gradient is NaN (inf * 0) where pt == 1, so every pixel has
    pt < 1 in float32 -- with room (1 - pt >= 1e-5 in float64) for the kernel's own rounding of pt."""

    logits, targets, weight = random_case(n, c, h, w, seed, scale=1.0)
    pt32 = F.softmax(logits, dim=1).gather(1, targets.unsqueeze(1))
    assert bool((pt32 < 1).all())
    pt64 = F.softmax(logits.double(), dim=1).gather(1, targets.unsqueeze(1))
    assert float((1 - pt64).min()) >= 1e-5
    return logits, targets, weight


def saturated_case(s, m, seed, n=2, c=4, h=33, w=31):
    """logits = randn * s + m * onehot(target) on about 90 % of the pixels and m * onehot(another class) on the rest: pt
    rounds to exactly 1 on right pixels and to ~1e-26 (s = 1) or exactly 0 (s = 30) on wrong ones."""

    g = _gen(seed)
    targets = torch.randint(0, c, (n, h, w), generator=g)
    wrong = torch.rand(n, h, w, generator=g) < 0.1
    shift = torch.randint(1, c, (n, h, w), generator=g)
    hot = torch.where(wrong, (targets + shift) % c, targets)
    logits = torch.randn(n, c, h, w, generator=g) * s + m * R.onehot(hot, c)
    weight = torch.rand(c, generator=g) + 0.2
    frac = float(wrong.float().mean())
    assert 0.05 < frac < 0.15
    pt32 = F.softmax(logits, dim=1).gather(1, targets.unsqueeze(1))
    assert bool((pt32 == 1).any()) and bool((pt32 < 1e-20).any())  # saturated both ways at the kernels' precision
    if s >= 30:
        assert bool((pt32 == 0).any())  # (exp(-60) is still a normal float32; the wide logits go below the smallest one)
    return logits, targets, weight


MIOU_SHAPE = (2, 3, 129, 129)  # 16 641 pixels per image: 66 blocks of 256 > the 64 blocks of the per-image loop
MIOU_CASES = {
    # name: (noise, margin, edit of the label map, branch)
    "uniform": (0.05, 0.1, None, "nll"),
    "confident": (0.5, 3.0, None, "miou"),
    "absent_class": (0.5, 3.0, "image 0 has no pixel of class 2", "miou"),
    "all_background": (0.5, 3.0, "image 1 is all background", "miou"),
}


def miou_case(kind, seed=31):
    """One of ``MIOU_CASES`` at ``MIOU_SHAPE``: blocky label maps, logits = randn * noise + margin * onehot(target).  Asserts on
    the float64 reference the branch the case is named for and that the two terms are >= 1e-2 apart (no rounding flips it)."""

    n, c, h, w = MIOU_SHAPE
    noise, margin, edit, branch = MIOU_CASES[kind]
    g = _gen(seed)
    coarse = torch.randint(0, c, (n, (h + 7) // 8, (w + 7) // 8), generator=g)
    targets = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :h, :w].contiguous()
    if kind == "absent_class":
        targets[0][targets[0] == 2] = 0
        assert int((targets[0] == 2).sum()) == 0 and int((targets[1] == 2).sum()) > 0
    elif kind == "all_background":
        targets[1] = 0
    logits = torch.randn(n, c, h, w, generator=g) * noise + margin * R.onehot(targets, c)
    weight = torch.tensor([1.0, 2.0, 0.5])
    got, gap = miou_branch64(logits, targets, weight)
    assert got == branch and gap >= 1e-2, (kind, got, gap)
    return logits, targets, weight


NLL_PROBE_SHAPE = (2, 3, 363, 363)  # HW = 131 769 = 514 * 256 + 185, P = 263 538 > 1 024 blocks * 256 threads
_HW, _P = 363 * 363, 2 * 363 * 363
NLL_PROBE_POSITIONS = (0, 255, 256, _HW - 1, _HW, 262143, 262144, _P - 1)


def nll_probe_case(pstar, seed=41):
    """Every pixel predicts its own class with margin 30 (loss and gradient ~ 0) except the flat pixel ``pstar``, which
    predicts another class with margin 5: the loss is that pixel's, and the gradient is nonzero only there."""

    n, c, h, w = NLL_PROBE_SHAPE
    g = _gen(seed)
    targets = torch.randint(0, c, (n, h, w), generator=g)
    weight = torch.rand(c, generator=g) + 0.2
    logits = 30.0 * R.onehot(targets, c)
    flat_t = targets.view(-1)
    img, hw = divmod(pstar, h * w)
    wrong = (int(flat_t[pstar]) + 1) % c
    logits.view(n, c, h * w)[img, :, hw] = 0.0
    logits.view(n, c, h * w)[img, wrong, hw] = 5.0
    return logits, targets, weight


def nll_probe_share(name, logits, targets, weight, pstar):
    """Share of the float64 loss that the probe pixel carries, and the largest |gradient| away from it over the largest at it."""

    n, c, h, w = logits.shape
    full, grad, _ = nll_family64(name, logits, targets, weight)
    mult = torch.ones(n * h * w)
    mult[pstar] = 0
    rest, _, _ = nll_family64(name, logits, targets, weight, mult=mult.view(n, h, w))
    gp = grad.view(n, c, h * w)
    img, hw = divmod(pstar, h * w)
    at = float(gp[img, :, hw].abs().max())
    away = gp.abs().clone()
    away[img, :, hw] = 0
    return 1.0 - rest / full, float(away.max()) / at


MIOU_PROBE_SHAPE = (2, 3, 129, 129)
MIOU_PROBE_HW = (0, 255, 256, 16383, 16384, 16640)  # in image 1: block borders, the last pixel of trip 1, the first of trip 2, the last
# With six alike pixels, leaving one out would move inter and union together and their ratio hardly at all: the seed is one (of
# about 1 in 100) at which each soft prediction is >= 0.06 from the mean of the six, which miou_probe_case asserts.
MIOU_PROBE_SEED = 3


def miou_probe_case(seed=MIOU_PROBE_SEED):
    """Class 2 occurs only at ``MIOU_PROBE_HW`` of image 1, predicted softly (margin 0.5, noise 0.3); every other pixel
    predicts its own class (0 or 1) with margin 8 and rejects class 2 with margin 8 -- the (class 2, image 1) term of the
    soft IoU rests on those six pixels.  Asserts on the float64 reference: the soft-IoU branch by >= 1e-2, and that leaving any
    ONE of the six out of the sums moves the loss by more than 100 loss bars.  Returns (logits, targets, weight, moves)."""

    n, c, h, w = MIOU_PROBE_SHAPE
    g = _gen(seed)
    targets = torch.randint(0, 2, (n, h, w), generator=g)
    logits = 8.0 * R.onehot(targets, c)
    logits[:, 2] = -8.0
    soft = torch.randn(c, len(MIOU_PROBE_HW), generator=g) * 0.3
    soft[2] += 0.5
    for i, hw in enumerate(MIOU_PROBE_HW):
        targets.view(n, h * w)[1, hw] = 2
        logits.view(n, c, h * w)[1, :, hw] = soft[:, i]
    weight = torch.tensor([1.0, 1.5, 2.0])
    branch, gap = miou_branch64(logits, targets, weight)
    assert branch == "miou" and gap >= 1e-2, (branch, gap)
    full = float(miou_terms64(logits, targets, weight)[0].detach())
    moves = []
    for hw in MIOU_PROBE_HW:
        keep = torch.ones(n, h * w, dtype=torch.bool)
        keep[1, hw] = False
        moves.append(abs(float(miou_terms64(logits, targets, weight, keep.view(n, h, w))[0].detach()) - full))
    assert min(moves) > 100 * LOSS_BAR * max(1.0, abs(full)), moves
    return logits, targets, weight, moves


COUNT_SHAPES = [(1, 2, 513, 513), (3, 4, 7, 9), (2, 8, 129, 129)]


def counts_case(n, c, h, w, seed):
    """Scores rounded to multiples of 0.5 (ties are common: the first maximal index must win) and uniform labels."""

    g = _gen(seed)
    scores = torch.round(torch.randn(n, c, h, w, generator=g) * 2) / 2
    targets = torch.randint(0, c, (n, h, w), generator=g)
    top = scores.max(1, keepdim=True).values
    assert int(((scores == top).sum(1) > 1).sum()) > n * h * w // 20  # ties on more than 5 % of the pixels
    return scores, targets


def counts_ref(scores, targets):
    """[tn, fn, fp, tp] summed over the samples with the oracle's ``confusion_counts``, and the number of pixels its quotient
    drops (prediction and label both foreground and different)."""

    total = [0, 0, 0, 0]
    for i in range(scores.shape[0]):
        total = [a + b for a, b in zip(total, R.confusion_counts(targets[i], scores[i]))]
    pred = torch.argmax(scores, 1)
    dropped = int(((pred != targets) & (pred > 0) & (targets > 0)).sum())
    assert sum(total) + dropped == targets.numel()
    return total, dropped
