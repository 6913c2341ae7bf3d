"""Restatements in numpy of the centerline stage definitions (include/robosat_hip.h): Guo-Hall thinning, the skeleton link rule
and the lone-pixel rule, on ONE raster.  The stitched definitions are these applied to the tiles pasted into a zero canvas
(``stitch_ref.Grid``: an absent tile is 0).  Not a test module; ``test_centerline_cpu.py`` pins it with scipy.ndimage.label."""

import numpy as np

import features_ref as R

# (dx, dy) of a link's second pixel by dir
STEP = {0: (1, 0), 1: (1, 1), 2: (0, 1), 3: (-1, 1)}


def _neighbours(m):
    """p2..p9 = N, NE, E, SE, S, SW, W, NW of every pixel, outside 0."""

    p = np.pad(m, 1)
    h, w = m.shape

    def at(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    return at(-1, 0), at(-1, 1), at(0, 1), at(1, 1), at(1, 0), at(1, -1), at(0, -1), at(-1, -1)


def sub_iteration(m, second):
    """One sub-iteration on bool ``m``: (the raster after it, pixels deleted).  Every pixel is judged on ``m`` itself."""

    p2, p3, p4, p5, p6, p7, p8, p9 = _neighbours(m)
    i = np.int8
    c = (~p2 & (p3 | p4)).astype(i) + (~p4 & (p5 | p6)).astype(i) + (~p6 & (p7 | p8)).astype(i) + (~p8 & (p9 | p2)).astype(i)
    n1 = (p9 | p2).astype(i) + (p3 | p4).astype(i) + (p5 | p6).astype(i) + (p7 | p8).astype(i)
    n2 = (p2 | p3).astype(i) + (p4 | p5).astype(i) + (p6 | p7).astype(i) + (p8 | p9).astype(i)
    n = np.minimum(n1, n2)
    mm = ((p6 | p7 | ~p9) & p8) if second else ((p2 | p3 | ~p5) & p4)
    delete = m & (c == 1) & (n >= 2) & (n <= 3) & ~mm
    return m & ~delete, int(delete.sum())


def thin(mask, want_pairs=False):
    """The skeleton of ``mask`` (non-zero = set) as uint8 0/1: pairs of sub-iterations until a whole pair deletes nothing.
    ``want_pairs``: also the number of pairs run, the last (empty) one included."""

    m = np.asarray(mask) != 0
    pairs = 0
    while True:
        m, a = sub_iteration(m, False)
        m, b = sub_iteration(m, True)
        pairs += 1
        assert pairs <= m.size + 1
        if a + b == 0:
            out = m.astype(np.uint8)
            return (out, pairs) if want_pairs else out


def links(skeleton, labels, kept=None, tile=0):
    """Sorted rows (tile, label, x, y, dir) of the link rule on one raster.  ``labels``: the labels of the mask; ``kept``: the
    labels whose components are listed (None: all).  A link is emitted where either end's component is kept, under its first
    pixel's label where that is kept and the other end's otherwise; a kept set pixel without a set 8-neighbour gives dir -1."""

    s = np.asarray(skeleton) != 0
    labels = np.asarray(labels)
    ok = (labels != 0) if kept is None else np.isin(labels, np.asarray(list(kept), dtype=labels.dtype)) & (labels != 0)
    p2, p3, p4, p5, p6, p7, p8, p9 = _neighbours(s)
    exists = {0: s & p4, 2: s & p6, 1: s & p5 & ~p4 & ~p6, 3: s & p7 & ~p8 & ~p6}
    h, w = s.shape
    lab_pad, ok_pad = np.pad(labels, 1), np.pad(ok, 1)
    rows = []
    for d, (dx, dy) in STEP.items():
        ys, xs = np.nonzero(exists[d])
        other_lab, other_ok = lab_pad[ys + 1 + dy, xs + 1 + dx], ok_pad[ys + 1 + dy, xs + 1 + dx]
        own_lab, own_ok = labels[ys, xs], ok[ys, xs]
        emit = own_ok | other_ok
        lab = np.where(own_ok, own_lab, other_lab)
        rows.append(np.stack([np.full(len(ys), tile), lab, xs, ys, np.full(len(ys), d)], axis=1)[emit])
    lone = s & ok & ~(p2 | p3 | p4 | p5 | p6 | p7 | p8 | p9)
    ys, xs = np.nonzero(lone)
    rows.append(np.stack([np.full(len(ys), tile), labels[ys, xs], xs, ys, np.full(len(ys), -1)], axis=1))
    return R.sort_rows(np.concatenate(rows).astype(np.int64))


def link_components(rows, shape):
    """Number of connected components of the link graph of ``rows`` (every pixel that a row names is a vertex)."""

    h, w = shape
    parent = {}

    def find(a):
        while parent.setdefault(a, a) != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for _, _, x, y, d in np.asarray(rows).tolist():
        a = find((x, y))
        if d >= 0:
            b = find((x + STEP[d][0], y + STEP[d][1]))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return len({find(p) for p in list(parent)})


# ---- masks ----------------------------------------------------------------------------------------------------------------
def roads(h, w, seed, count=5, width=12):
    """Straight roads of ``width`` pixels at random angles through an h x w raster, crossing each other."""

    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w), dtype=bool)
    for _ in range(count):
        cy, cx, angle = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0, np.pi)
        m |= np.abs((xx - cx) * np.sin(angle) - (yy - cy) * np.cos(angle)) <= width / 2
    return m
