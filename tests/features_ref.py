"""Restatements of the ``rs features`` stage definitions (include/robosat_hip.h) in numpy, and the mask shapes the tests run
them on.  Not a test module; ``test_features_cpu.py`` pins these against scipy.ndimage where scipy imports."""

import math

import numpy as np


def disc(eps):
    k = np.zeros((eps, eps), dtype=np.uint8)
    r = c = eps // 2
    for i in range(eps):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * math.sqrt((r * r - dy * dy) / (r * r)))) if r else 0
            k[i, max(c - dx, 0):min(c + dx + 1, eps)] = 1
    return k


def offsets(eps):
    k = disc(eps)
    r = c = eps // 2
    return [(i - r, j - c) for i in range(eps) for j in range(eps) if k[i, j]]


def _shifted(m, dy, dx, fill):
    """out[y, x] = m[y + dy, x + dx], `fill` outside."""
    h, w = m.shape
    out = np.full((h, w), fill, dtype=bool)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = m[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def erode(m, eps):
    m = np.asarray(m, dtype=bool)
    if eps <= 1:
        return m.copy()
    out = np.ones_like(m)
    for dy, dx in offsets(eps):
        out &= _shifted(m, dy, dx, True)
    return out


def dilate(m, eps):
    m = np.asarray(m, dtype=bool)
    if eps <= 1:
        return m.copy()
    out = np.zeros_like(m)
    for dy, dx in offsets(eps):
        out |= _shifted(m, -dy, -dx, False)
    return out


def opening(m, eps):
    return dilate(erode(m, eps), eps)


def closing(m, eps):
    return erode(dilate(m, eps), eps)


def clean(image, index, eps_open, eps_close):
    return closing(opening(np.asarray(image) == index, eps_open), eps_close).astype(np.uint8)


def label(mask):
    """4-connected components, label = 1 + min(y * W + x): a small union-find over the rows' runs (numbered in raster order,
    the smaller root wins, so a component's root is the run holding its smallest pixel)."""

    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    parent, first = [], []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    rows, prev = [], []
    for y in range(h):
        d = np.diff(np.concatenate([[0], mask[y].astype(np.int8), [0]]))
        cur = []
        for s, e in zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()):
            cur.append((s, e, len(parent)))
            parent.append(len(parent))
            first.append(y * w + s)
        i = 0
        for s, e, k in cur:
            while i < len(prev) and prev[i][1] <= s:
                i += 1
            j = i
            while j < len(prev) and prev[j][0] < e:
                a, b = find(k), find(prev[j][2])
                if a != b:
                    parent[max(a, b)] = min(a, b)
                j += 1
        rows.append(cur)
        prev = cur
    out = np.zeros((h, w), dtype=np.int32)
    for y, cur in enumerate(rows):
        for s, e, k in cur:
            out[y, s:e] = first[find(k)] + 1
    return out


def canonical(labels):
    """Any labelling (0 = background) -> the canonical one."""

    labels = np.asarray(labels)
    h, w = labels.shape
    flat = labels.ravel()
    out = np.zeros(h * w, dtype=np.int32)
    fg = np.nonzero(flat)[0]
    if len(fg):
        smallest = np.full(int(flat.max()) + 1, h * w, dtype=np.int64)
        np.minimum.at(smallest, flat[fg], fg)
        out[fg] = smallest[flat[fg]] + 1
    return out.reshape(h, w)


def table(labels, min_area=0, tile=0):
    """Rows (tile, label, area, x0, y0, x1, y1) sorted by label."""

    rows = []
    ys, xs = np.nonzero(labels)
    lab = labels[ys, xs]
    order = np.argsort(lab, kind="stable")
    ys, xs, lab = ys[order], xs[order], lab[order]
    cuts = np.nonzero(np.diff(lab))[0] + 1
    for y, x, l in zip(np.split(ys, cuts), np.split(xs, cuts), np.split(lab, cuts)):
        if len(l) and len(l) >= min_area:
            rows.append((tile, int(l[0]), len(l), int(x.min()), int(y.min()), int(x.max()), int(y.max())))
    return np.array(rows, dtype=np.int32).reshape(-1, 7)


def filter_labels(labels, min_area):
    keep = table(labels, min_area)[:, 1]
    return np.where(np.isin(labels, keep), labels, 0).astype(np.int32)


def edges(labels, tile=0):
    """The edge rule by array comparison: rows (tile, label, x, y, dir), sorted."""

    p = np.pad(labels, 1)
    c = p[1:-1, 1:-1]
    rows = []
    for d, nb in enumerate((p[:-2, 1:-1], p[1:-1, 2:], p[2:, 1:-1], p[1:-1, :-2])):  # top, right, bottom, left
        ys, xs = np.nonzero((c != 0) & (nb != c))
        rows.append(np.stack([np.full(len(ys), tile), c[ys, xs], xs, ys, np.full(len(ys), d)], axis=1))
    return sort_rows(np.concatenate(rows).astype(np.int32))


def sort_rows(rows):
    rows = np.asarray(rows)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


def fill_even_odd(rings, h, w):
    """Even-odd fill of rings (float or int vertices [[x, y], ...], open or closed) sampled at the pixel centres."""

    out = np.zeros((h, w), dtype=bool)
    yc = np.arange(h) + 0.5
    xc = np.arange(w) + 0.5
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64)
        nxt = np.roll(ring, -1, axis=0)
        for (x0, y0), (x1, y1) in zip(ring, nxt):
            if y0 == y1:
                continue
            rows = np.nonzero((yc > min(y0, y1)) & (yc < max(y0, y1)))[0]
            xi = x0 + (yc[rows] - y0) * (x1 - x0) / (y1 - y0)
            out[rows] ^= xc[None, :] > xi[:, None]
    return out


# ---- masks ----------------------------------------------------------------------------------------------------------------
def blobs(h, w, seed, count=6):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w), dtype=bool)
    for _ in range(count):
        cy, cx = rng.randint(0, h), rng.randint(0, w)
        ry, rx = rng.randint(2, max(3, h // 5 + 2)), rng.randint(2, max(3, w // 5 + 2))
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    m ^= rng.rand(h, w) < 0.02  # salt and pepper for the opening / closing to remove
    return m


def noise(h, w, seed, density):
    return np.random.RandomState(seed).rand(h, w) < density


def border(h, w):
    m = np.zeros((h, w), dtype=bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    m[h // 2, :] = True
    return m


def checkerboard(h, w):
    yy, xx = np.mgrid[:h, :w]
    return (yy + xx) % 2 == 0


def spiral(n):
    """A one-pixel-wide square spiral filling n x n: a single component whose pixels form one chain of about n*n/2."""

    m = np.zeros((n, n), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        moved = False
        for _ in range(2):  # go on, or turn once
            ny, nx = y + dy, x + dx
            ay, ax = ny + dy, nx + dx  # the cell after next must be free as well (keeps the arms one pixel apart)
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = True
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return m


def comb(n):
    """Teeth hanging from a spine along the top row: one component, every other column a chain of n pixels."""

    m = np.zeros((n, n), dtype=bool)
    m[0, :] = True
    m[:, ::2] = True
    return m


def corner_touch():
    m = np.zeros((8, 9), dtype=bool)
    m[1:4, 1:4] = True
    m[4:7, 4:8] = True  # meets the first block only at the corner (4, 4)
    m[0, 8] = m[1, 7] = True  # two single pixels meeting at a corner
    return m


def nested():
    """A ring inside a hole inside a ring, and an island in the inner hole."""

    m = np.zeros((21, 23), dtype=bool)
    m[1:20, 1:22] = True
    m[3:18, 3:20] = False
    m[5:16, 5:18] = True
    m[7:14, 7:16] = False
    m[9:12, 9:14] = True
    return m


def self_touching():
    """One component whose pixels meet only at corners in several places (4-connected through a detour)."""

    m = np.zeros((9, 9), dtype=bool)
    m[1:8, 1:8] = True
    m[2:4, 2:4] = False
    m[4:6, 4:6] = False  # two holes touching at the corner (4, 4)
    m[6, 6] = False
    m[7, 7] = False  # a notch touching a hole at (7, 7)
    return m
