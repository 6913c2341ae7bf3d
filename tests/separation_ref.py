"""Restatement in numpy of the separation weight plane (include/robosat_hip.h, "SEPARATION WEIGHT"), written straight from the
definition (TEST INFRASTRUCTURE ONLY; not a test module): a flood fill labels the objects, every object's squared distance to every
background pixel is found by brute force, the two smallest are taken, s2 = a + b + isqrt(4ab) with ``math.isqrt``, and the float64
table is rounded once to float32.  There are no separable passes here on purpose: nothing shares its reasoning with the kernels.

Also the label rasters the CPU and GPU tests share, and ``exercised``: what a raster actually puts to the test, on this reference."""

import math

import numpy as np
import torch

IGNORE = 255
FAR = np.iinfo(np.int64).max


def reach(sigma):
    return int(math.ceil(3.0 * sigma))


def table(ws, sigma):
    """float32 [D * D], made in float64 and rounded once."""

    d = reach(sigma)
    return np.array([float(ws) * math.exp(-k / (2.0 * float(sigma) * float(sigma))) for k in range(d * d)], dtype=np.float64).astype(np.float32)


def classes_of(labels, classes, ignore=None):
    """(object pixels, valid background pixels) of one image, two bool [H, W]."""

    t = np.asarray(labels).astype(np.int64)
    valid = np.ones(t.shape, dtype=bool) if ignore is None else t != ignore
    obj = valid & (t >= 1) & (t < classes)
    return obj, valid & ~obj


def objects(obj):
    """int64 [H, W]: the 4-connected components of the set pixels numbered 1, 2, ... in raster order of their first pixel; 0 elsewhere."""

    h, w = obj.shape
    out = np.zeros((h, w), dtype=np.int64)
    count = 0
    for y0 in range(h):
        for x0 in range(w):
            if not obj[y0, x0] or out[y0, x0]:
                continue
            count += 1
            out[y0, x0] = count
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < h and 0 <= xx < w and obj[yy, xx] and not out[yy, xx]:
                        out[yy, xx] = count
                        stack.append((yy, xx))
    return out


def nearest_two(labels, classes, ignore=None):
    """(a, b) int64 [H, W]: at a valid background pixel the smallest and the second smallest of the per-object squared distances
    (``FAR`` where there is no such object), ``FAR`` at every other pixel."""

    obj, bg = classes_of(labels, classes, ignore)
    comp = objects(obj)
    h, w = obj.shape
    a = np.full((h, w), FAR, dtype=np.int64)
    b = np.full((h, w), FAR, dtype=np.int64)
    py, px = np.nonzero(bg)
    if py.size == 0:
        return a, b
    best = np.full((2, py.size), FAR, dtype=np.int64)  # the two smallest per-object values so far, ascending
    for k in range(1, int(comp.max()) + 1):
        qy, qx = np.nonzero(comp == k)
        delta = np.full(py.size, FAR, dtype=np.int64)
        for lo in range(0, qy.size, 256):  # (pixels x object pixels, a slab at a time)
            dy = py[:, None] - qy[None, lo:lo + 256]
            dx = px[:, None] - qx[None, lo:lo + 256]
            delta = np.minimum(delta, (dy * dy + dx * dx).min(axis=1))
        best = np.sort(np.vstack([best, delta[None]]), axis=0)[:2]
    a[py, px], b[py, px] = best[0], best[1]
    return a, b


def s2_of(a, b):
    """int64 like ``a``: a + b + isqrt(4ab) where both are there, ``FAR`` elsewhere."""

    out = np.full(a.shape, FAR, dtype=np.int64)
    for i in zip(*np.nonzero(b != FAR)):
        out[i] = int(a[i]) + int(b[i]) + math.isqrt(4 * int(a[i]) * int(b[i]))
    return out


def term(labels, ws, sigma, classes, ignore=None):
    """float32 [H, W] of one image: table[s2] where s2 < D^2 at a valid background pixel, +0 elsewhere."""

    d = reach(sigma)
    tab = table(ws, sigma)
    s2 = s2_of(*nearest_two(labels, classes, ignore))
    out = np.zeros(s2.shape, dtype=np.float32)
    near = s2 < d * d
    out[near] = tab[s2[near]]
    return out


def base_of(targets, ignore=None):
    """float32 [N, H, W]: 1 at a valid pixel, 0 at an ignored one."""

    t = targets.numpy() if torch.is_tensor(targets) else np.asarray(targets)
    return (np.ones(t.shape, dtype=bool) if ignore is None else t != ignore).astype(np.float32)


def plane(targets, ws, sigma, classes, ignore=None, base=None):
    """float32 torch [N, H, W] from int64 [N, H, W]: base + term in one float32 addition, every image on its own."""

    t = targets.numpy() if torch.is_tensor(targets) else np.asarray(targets)
    b = base_of(t, ignore) if base is None else (base.numpy() if torch.is_tensor(base) else np.asarray(base)).astype(np.float32)
    out = np.empty(t.shape, dtype=np.float32)
    for n in range(t.shape[0]):
        out[n] = b[n] + term(t[n], ws, sigma, classes, ignore)
    return torch.from_numpy(out)


def exercised(labels, sigma, classes, ignore=None):
    """What one image puts to the test, as counts of pixels: ``term`` (s2 < D^2), ``far`` (two objects within D^2 but s2 >= D^2),
    ``same`` (a background pixel whose nearest object pixels to the left and to the right in its row, both within D - 1, are of ONE
    object) and ``ignored``."""

    d = reach(sigma)
    t = np.asarray(labels)
    obj, bg = classes_of(t, classes, ignore)
    comp = objects(obj)
    a, b = nearest_two(t, classes, ignore)
    s2 = s2_of(a, b)
    same = 0
    for y, x in zip(*np.nonzero(bg)):
        left = [comp[y, x - k] for k in range(1, d) if x - k >= 0 and comp[y, x - k]]
        right = [comp[y, x + k] for k in range(1, d) if x + k < t.shape[1] and comp[y, x + k]]
        same += bool(left and right and left[0] == right[0])
    return {"term": int((s2 < d * d).sum()), "far": int(((b < d * d) & (s2 >= d * d)).sum()), "same": same,
            "ignored": 0 if ignore is None else int((t == ignore).sum())}


# ---- label rasters --------------------------------------------------------------------------------------------------------------
def standard_raster(h, w, ignore=False):
    """int64 numpy [h, w], classes 0..2: two class-1 rectangles side by side with a gap of two columns, a slot in the first; below them a class-2 U whose
    courtyard opens upward; a class-1 rectangle cut by the top right corner; a single class-2 pixel in the bottom right corner.
    ``ignore``: a 255 band across the gap (and one pixel into either rectangle) and a 255 block in the bottom left corner."""

    t = np.zeros((h, w), dtype=np.int64)
    t[h // 8:h // 2, w // 10:w // 2] = 1
    t[h // 8:h // 2, w // 2 + 2:9 * w // 10] = 1
    t[h // 8:h // 4, w // 4:w // 4 + 3] = 0  # (a slot of three columns in the first one: the same object on both sides at any reach)
    t[5 * h // 8:7 * h // 8, w // 5:4 * w // 5] = 2
    t[5 * h // 8:3 * h // 4, 2 * w // 5:3 * w // 5] = 0
    t[0:max(1, h // 16), 15 * w // 16:w] = 1
    t[h - 1, w - 1] = 2
    if ignore:
        t[h // 4:3 * h // 8, w // 2 - 1:w // 2 + 3] = IGNORE
        t[15 * h // 16:h, 0:w // 8] = IGNORE
    return t


def small_raster(h, w, seed):
    """int64 numpy [h, w] for rasters smaller than the reach: seeded single pixels and short runs of the classes 1 and 2, an object at
    either end of the longer side."""

    rng = np.random.RandomState(seed)
    t = np.zeros((h, w), dtype=np.int64)
    for _ in range(max(2, (h * w) // 12)):
        y, x = rng.randint(h), rng.randint(w)
        t[y, x:x + rng.randint(1, 3)] = rng.randint(1, 3)
    if min(h, w) == 1 and h * w >= 3:
        flat = t.reshape(-1)  # (a view)
        flat[0], flat[1], flat[-2], flat[-1] = 1, 0, 0, 2
    elif h * w >= 4:
        t[0, 0], t[0, 1], t[h - 1, w - 1] = 1, 0, 2  # (two objects whatever the draws were, and a background pixel beside one)
    return t


def rectangles(h, w, boxes):
    """int64 numpy [h, w]: ``boxes`` = (y0, y1, x0, x1, class) with both ends inclusive, painted in order."""

    t = np.zeros((h, w), dtype=np.int64)
    for y0, y1, x0, x1, c in boxes:
        t[y0:y1 + 1, x0:x1 + 1] = c
    return t
