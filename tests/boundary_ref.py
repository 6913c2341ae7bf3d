"""Restatement in numpy of the boundary weight plane (include/robosat_hip.h, "BOUNDARY-WEIGHTED CrossEntropy / Focal") and the
float64 loss it weighs (TEST INFRASTRUCTURE ONLY; not a test module): the boundary set, ``edt_ref.edt`` on its complement, the table,
the plane, and loss and gradient through ``losses_ref.nll_family64(mult=plane)``.  Nothing here knows the kernels.

Also the label rasters the CPU and GPU tests share; each builder asserts -- on this reference -- the property it is there for."""

import math

import numpy as np
import torch

import edt_ref
import losses_ref as L

IGNORE = 255


def reach(sigma):
    return int(math.ceil(3.0 * sigma))


def boundary_set(labels, ignore=None):
    """bool [H, W]: a valid pixel with a valid 4-neighbour of another label inside the raster (one image)."""

    t = np.asarray(labels).astype(np.int64)
    valid = np.ones(t.shape, dtype=bool) if ignore is None else t != ignore
    out = np.zeros(t.shape, dtype=bool)
    # (each pair of neighbours once per direction: the slices are the pixels that HAVE that neighbour)
    for a, b in (((slice(None), slice(1, None)), (slice(None), slice(None, -1))),   # left neighbour
                 ((slice(None), slice(None, -1)), (slice(None), slice(1, None))),   # right
                 ((slice(1, None), slice(None)), (slice(None, -1), slice(None))),   # up
                 ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):  # down
        out[a] |= valid[a] & valid[b] & (t[a] != t[b])
    return out


def distance2(labels, sigma, ignore=None, brute=False):
    """int64 [H, W]: min(R^2, squared distance to the nearest boundary pixel of the raster) -- the capped transform of the
    COMPLEMENT of the boundary set (a boundary pixel is "unset" and reads 0)."""

    r = reach(sigma)
    return (edt_ref.edt_brute if brute else edt_ref.edt)(~boundary_set(labels, ignore), r)


def table(w0, sigma):
    """float32 [R * R], made in float64 and rounded once."""

    r = reach(sigma)
    return np.array([1.0 + float(w0) * math.exp(-k / (2.0 * float(sigma) * float(sigma))) for k in range(r * r)], dtype=np.float64).astype(np.float32)


def plane(targets, w0, sigma, ignore=None):
    """float32 torch [N, H, W] from int64 [N, H, W]: table[d2] below the cap, exactly 1 at it, exactly 0 at an ignored pixel; every
    image on its own."""

    t = targets.numpy() if torch.is_tensor(targets) else np.asarray(targets)
    r = reach(sigma)
    tab = np.concatenate([table(w0, sigma), np.ones(1, dtype=np.float32)])  # (index R^2: the cap)
    out = np.empty(t.shape, dtype=np.float32)
    for n in range(t.shape[0]):
        d2 = distance2(t[n], sigma, ignore)
        assert d2.min() >= 0 and d2.max() <= r * r
        out[n] = tab[d2]
        if ignore is not None:
            out[n][t[n] == ignore] = 0.0
    return torch.from_numpy(out)


def loss64(name, logits, targets, weight, mult, ignore=None, gamma=2):
    """(loss, gradient float64, denominator) of sum_valid m w l / sum_valid m w through ``losses_ref.nll_family64``: an ignored
    pixel gets multiplicity 0 and a label that can index (class 0); a denominator of 0 gives loss 0 and gradient 0."""

    t, m = targets, mult.double()
    if ignore is not None:
        bad = targets == ignore
        t = torch.where(bad, torch.zeros_like(targets), targets)
        m = torch.where(bad, torch.zeros_like(m), m)
    w = torch.ones(logits.shape[1], dtype=torch.float64) if weight is None else weight.double()
    if float((w[t] * m).sum()) == 0.0:
        return 0.0, torch.zeros(logits.shape, dtype=torch.float64), 0.0
    return L.nll_family64(name, logits, t, weight, gamma=gamma, mult=m)


# ---- label rasters --------------------------------------------------------------------------------------------------------------
def standard_raster(h, w, ignore=False):
    """int64 numpy [h, w]: class 1 on rows h/5..h/2, columns w/5..3w/5; class 2 on rows 13h/20..9h/10, columns w/10..2w/5; class 1 on
    rows 0..h/8, columns 3w/4..w (an object cut by the raster's edge); ``ignore``: a 255 block across the first rectangle's right edge."""

    t = np.zeros((h, w), dtype=np.int64)
    t[h // 5:h // 2, w // 5:3 * w // 5] = 1
    t[13 * h // 20:9 * h // 10, w // 10:2 * w // 5] = 2
    t[0:max(1, h // 8), 3 * w // 4:w] = 1
    if ignore:
        t[h // 4:2 * h // 5, w // 2:7 * w // 10] = IGNORE
    return t


def shares(plane_, labels, ignore=None):
    """(share of the valid pixels with m > 1, share with m == 1 exactly)."""

    p = plane_.numpy() if torch.is_tensor(plane_) else plane_
    valid = np.ones(p.shape, dtype=bool) if ignore is None else np.asarray(labels) != ignore
    return float((p[valid] > 1).mean()), float((p[valid] == 1).mean())


def standard_case(h, w, sigma, w0=4.0, ignore=False):
    """(targets int64 torch [1, h, w], reference plane) of the standard raster; asserts the condition on the inputs: at least 20 % of
    the valid pixels weigh more than 1 and at least 20 % exactly 1, and, ignore variant, another boundary set than the plain one."""

    t = standard_raster(h, w, ignore)
    ig = IGNORE if ignore else None
    m = plane(t[None], w0, sigma, ig)
    above, at = shares(m[0], t, ig)
    assert above >= 0.2 and at >= 0.2, (h, w, sigma, above, at)
    if ignore:
        plain = standard_raster(h, w)
        assert (boundary_set(t, IGNORE) != boundary_set(plain)).any()
        assert (boundary_set(t, IGNORE) != boundary_set(t)).any()  # (and 255 read as a class would make its rim a boundary)
    return torch.from_numpy(t[None]), m


def logits_for(targets, classes, seed, scale=2.0):
    """float32 [N, C, H, W] randn * scale and a class weight rand + 0.2, from the seed alone."""

    g = torch.Generator().manual_seed(seed)
    n, h, w = targets.shape
    return torch.randn(n, classes, h, w, generator=g) * scale, torch.rand(classes, generator=g) + 0.2
