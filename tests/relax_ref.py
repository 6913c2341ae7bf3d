"""Reference of boundary label relaxation (TEST INFRASTRUCTURE ONLY; numpy and float64 torch on the CPU, never the device).

``sets_brute`` is the definition of the label set plane as a loop over the window; ``sets_separable`` the same plane by a row
pass and a column pass (tests/test_relax_cpu.py holds them against each other).  ``loss64`` is the definition of the relaxed
CrossEntropy / Focal loss in float64 with the gradient from autograd: ``logsumexp`` over the classes with -inf outside the
pixel's set.  The builders return CPU tensors that depend on their arguments alone, and ``census`` says what a case exercises,
so that every test can assert it on the reference before it looks at the code under test."""

import functools

import numpy as np
import torch

IGNORE = 255


def sets_brute(labels, radius, ignore=None):
    """uint8 numpy [N, H, W] from int64 numpy [N, H, W]: bit c of a valid pixel = some valid pixel of its image within ``radius`` in x
    and in y has label c; 0 at an ignored pixel.  A loop over the pixels, each of which ORs the class bits of its whole window."""

    labels = np.asarray(labels)
    n, h, w = labels.shape
    valid = np.ones(labels.shape, dtype=bool) if ignore is None else labels != ignore
    bit = np.where(valid, np.left_shift(1, np.where(valid, labels, 0)), 0).astype(np.uint8)
    out = np.zeros((n, h, w), dtype=np.uint8)
    for i in range(n):
        for y in range(h):
            for x in range(w):
                if valid[i, y, x]:
                    out[i, y, x] = np.bitwise_or.reduce(bit[i, max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1], axis=None)
    return out


def sets_separable(labels, radius, ignore=None):
    """The same plane by a row pass and a column pass over the class bits (OR is associative: the square window is separable)."""

    labels = np.asarray(labels)
    valid = np.ones(labels.shape, dtype=bool) if ignore is None else labels != ignore
    bits = np.where(valid, np.left_shift(1, np.where(valid, labels, 0)), 0).astype(np.uint8)
    n, h, w = labels.shape
    rows = np.zeros_like(bits)
    for d in range(-radius, radius + 1):
        lo, hi = max(0, -d), min(w, w - d)
        if lo < hi:
            rows[:, :, lo:hi] |= bits[:, :, lo + d:hi + d]
    out = np.zeros_like(bits)
    for d in range(-radius, radius + 1):
        lo, hi = max(0, -d), min(h, h - d)
        if lo < hi:
            out[:, lo:hi, :] |= rows[:, lo + d:hi + d, :]
    return np.where(valid, out, 0).astype(np.uint8)


def popcount(sets):
    s = np.asarray(sets).astype(np.int64)
    return sum((s >> c) & 1 for c in range(8))


def census(labels, sets, ignore=None):
    """What a case holds: the numbers of valid pixels whose set has 1, 2 and >= 3 classes, of ignored pixels, and the OR of all sets."""

    labels, sets = np.asarray(labels), np.asarray(sets)
    valid = np.ones(labels.shape, dtype=bool) if ignore is None else labels != ignore
    k = popcount(sets)
    return {"one": int((valid & (k == 1)).sum()), "two": int((valid & (k == 2)).sum()), "more": int((valid & (k >= 3)).sum()),
            "ignored": int((~valid).sum()), "bits": int(np.bitwise_or.reduce(sets.ravel())) if sets.size else 0}


def loss64(name, logits, targets, sets, weight=None, mult=None, ignore=None, gamma=2):
    """(loss, gradient float64, denominator) of ``sum_valid m w[t] l / sum_valid m w[t]`` with the relaxed pixel term:
    ``log q = logsumexp_{c in S} x_c - logsumexp_c x_c``, CrossEntropy ``l = -log q``, Focal ``l = -(1 - q)^gamma log q``.  ``sets`` is a
    uint8 tensor / array [N, H, W]; the class weight is the pixel's own label's; ``mult`` the optional pixel weights.  An ignored
    pixel gets multiplicity 0 (and a set of all classes, a label of 0: nothing of it reaches the result); a denominator of 0 gives
    loss 0 and gradient 0."""

    n, c, h, w = logits.shape
    s = torch.as_tensor(np.asarray(sets).astype(np.int64))
    t = targets
    m = torch.ones(n, h, w, dtype=torch.float64) if mult is None else mult.double()
    if ignore is not None:
        bad = targets == ignore
        t = torch.where(bad, torch.zeros_like(targets), targets)
        m = torch.where(bad, torch.zeros_like(m), m)
        s = torch.where(bad, torch.full_like(s, (1 << c) - 1), s)
    member = torch.stack([(s >> k) & 1 for k in range(c)], dim=1).bool()
    assert bool(member.gather(1, t.unsqueeze(1)).all()), "a valid pixel holds its own bit"
    wc = torch.ones(c, dtype=torch.float64) if weight is None else weight.double()
    wp = wc[t] * m
    den = float(wp.sum())
    if den == 0.0:
        return 0.0, torch.zeros(logits.shape, dtype=torch.float64), 0.0
    x = logits.double().clone().requires_grad_(True)
    lse = torch.logsumexp(x, dim=1)
    lse_s = torch.logsumexp(torch.where(member, x, torch.full_like(x, float("-inf"))), dim=1)
    logq = lse_s - lse
    if name == "CrossEntropy":
        per_pixel = -logq
    elif name == "Focal":
        per_pixel = -((1 - torch.exp(logq)).clamp(min=0) ** gamma) * logq
    else:
        raise KeyError(name)
    loss = (wp * per_pixel).sum() / wp.sum()
    loss.backward()
    return float(loss.detach()), x.grad, den


# ---- label rasters ----------------------------------------------------------------------------------------------------------------
def blocks_raster(n, c, h, w, seed, ignore=False):
    """int64 numpy [n, h, w]: random rectangles of every class 0 .. c-1 painted over each other (several sizes, so that sets of 1, 2 and
    more classes occur at small radii), class c-1 always somewhere; ``ignore``: a few rectangles of 255 on top, one of them with a single
    valid pixel inside."""

    rng = np.random.RandomState(seed)
    t = np.zeros((n, h, w), dtype=np.int64)
    for i in range(n):
        for k in range(4 * c):
            cls = k % c
            y0, x0 = rng.randint(0, h), rng.randint(0, w)
            hh, ww = rng.randint(1, max(2, h // 2)), rng.randint(1, max(2, w // 2))
            t[i, y0:y0 + hh, x0:x0 + ww] = cls
        t[i, rng.randint(0, h), rng.randint(0, w)] = c - 1
        if ignore:
            for _ in range(3):
                y0, x0 = rng.randint(0, h), rng.randint(0, w)
                t[i, y0:y0 + rng.randint(1, max(2, h // 3)), x0:x0 + rng.randint(1, max(2, w // 3))] = IGNORE
    return t


def noise_raster(n, c, h, w, seed):
    """int64 numpy [n, h, w] of labels uniform over the classes: almost every set holds every class."""

    return np.random.RandomState(seed).randint(0, c, size=(n, h, w)).astype(np.int64)


def singleton_raster(n, c, h, w, radius, seed=0):
    """int64 numpy [n, h, w] whose every valid pixel has a set of its own label alone at ``radius``: vertical bands of the classes, each
    ``radius + 2`` columns wide, separated by ignored strips of ``radius + 1`` columns (wider than the reach), band order from the seed."""

    rng = np.random.RandomState(seed)
    t = np.full((n, h, w), IGNORE, dtype=np.int64)
    step = 2 * radius + 3
    for i in range(n):
        order = rng.permutation(c)
        for b, x0 in enumerate(range(0, w, step)):
            t[i, :, x0:x0 + radius + 2] = order[b % c]
    return t


def shape_truth(h, w, margin):
    """int64 numpy [h, w]: an L-shaped object of class 1 on background 0 that stays ``margin`` pixels away from every edge."""

    t = np.zeros((h, w), dtype=np.int64)
    t[margin:h - margin, margin:margin + max(3, (w - 2 * margin) // 3)] = 1
    t[h - margin - max(3, (h - 2 * margin) // 3):h - margin, margin:w - margin] = 1
    return t


def shifted_case(h, w, radius, dx, dy):
    """(logits float32 [1, 2, h, w] = 20 * onehot(truth), labels int64 [1, h, w] = the truth moved by (dx, dy)): a confident network
    that follows the true shape against labels that are off by the shift.  The object keeps ``radius + 2`` pixels from every edge, so the
    moved raster is the truth's translate with background coming in."""

    truth = shape_truth(h, w, radius + 2 + 1)
    labels = np.zeros_like(truth)
    ys, xs = np.nonzero(truth)
    labels[ys + dy, xs + dx] = 1
    logits = torch.zeros(1, 2, h, w)
    tt = torch.from_numpy(truth)
    logits[0, 0][tt == 0] = 20.0
    logits[0, 1][tt == 1] = 20.0
    return logits, torch.from_numpy(labels[None])


def logits_for(shape, seed, scale=2.0):
    """float32 randn * scale of ``shape`` = (N, C, H, W) and a class weight rand + 0.2, from the seed alone."""

    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale, torch.rand(shape[1], generator=g) + 0.2


def pixel_weights(n, h, w, seed):
    """float32 [n, h, w] in 0.5 .. 2.5 with about a tenth of the pixels at exactly 0."""

    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, h, w, generator=g) * 2.0 + 0.5
    m[torch.rand(n, h, w, generator=g) < 0.1] = 0.0
    return m


@functools.lru_cache(maxsize=None)
def loss_case(c, shape_key, ignore, seed=7):
    """The shared rasters of the loss tests: (targets int64 torch [N, H, W], sets uint8 numpy at radius 2) for ``shape_key`` in
    ("wide", "small") = (3, C, 33, 65) / (1, C, 7, 9), made once; asserts that sets of 1, 2 and (C >= 3) more classes occur."""

    n, h, w = (3, 33, 65) if shape_key == "wide" else (1, 7, 9)
    t = blocks_raster(n, c, h, w, seed + c, ignore=ignore)
    if shape_key == "small":
        t = np.zeros((n, h, w), dtype=np.int64)
        t[0, :, 6:] = 1  # columns 0 and 1 see class 0 alone, column 8 class 1 alone, the ones between them both
        for k in range(2, c):
            t[0, 0 if k % 2 == 0 else 6, 4 + (k - 2) // 2] = k  # single pixels of the other classes in columns 4 .. 6
        if ignore:
            t[0, 3, 4] = IGNORE
    ig = IGNORE if ignore else None
    s = sets_brute(t, 2, ig)
    cen = census(t, s, ig)
    assert cen["one"] > 0 and cen["two"] > 0 and (c < 3 or cen["more"] > 0) and (cen["ignored"] > 0) == bool(ignore), (c, shape_key, cen)
    return torch.from_numpy(t), s
