"""Restatement in numpy of ``rs features --split`` (include/robosat_hip.h: seeds, start raster, growth steps) on ONE raster, and of
its stitched form on the tiles pasted into one canvas (``stitch_ref.Grid``).  Not a test module; ``test_split_cpu.py`` pins it on
shapes whose answer can be written down by hand."""

import numpy as np

import edt_ref as E
import features_ref as R


def seeds(mask, radius, coded=False):
    """bool [H, W]: the pixels a disc of ``radius`` fits around -- d2 == radius^2 in the capped transform.  ``coded``: the raster
    holds ``edt_ref``'s UNSET / SET / UNKNOWN."""

    return E.edt(mask, radius, coded=coded) == radius * radius


def start(labels, seed_labels):
    """L0: the core's label on a seed pixel, -1 on the other pixels of a component that holds one, the component's own label where it
    holds none, 0 on background."""

    labels, seed_labels = np.asarray(labels, dtype=np.int64), np.asarray(seed_labels, dtype=np.int64)
    with_seed = np.isin(labels, np.unique(labels[seed_labels != 0]))
    return np.where(seed_labels != 0, seed_labels, np.where(labels == 0, 0, np.where(with_seed, -1, labels)))


def step(raster):
    """One growth step: every -1 pixel takes the first label > 0 among its N, W, E, S neighbours as they stood before the step
    (outside the raster reads 0)."""

    p = np.pad(raster, 1)
    n, w, e, s = p[:-2, 1:-1], p[1:-1, :-2], p[1:-1, 2:], p[2:, 1:-1]
    pick = np.where(n > 0, n, np.where(w > 0, w, np.where(e > 0, e, np.where(s > 0, s, -1))))
    return np.where(raster == -1, pick, raster)


def grow(raster, steps=None, want_steps=False):
    """Steps until no -1 is left (or ``steps`` of them).  A step that changes nothing with -1 pixels left raises."""

    raster = np.asarray(raster, dtype=np.int64)
    done = 0
    while (raster == -1).any() and (steps is None or done < steps):
        after = step(raster)
        if steps is None and (after == raster).all():
            raise RuntimeError("{} unassigned pixels that no label reaches".format(int((raster == -1).sum())))
        raster = after
        done += 1
    return (raster, done) if want_steps else raster


def start_of(mask, radius):
    """L0 of one raster (non-zero = set)."""

    mask = np.asarray(mask) != 0
    return start(R.label(mask), R.label(seeds(mask, radius)))


def split(mask, radius):
    """int32 [H, W]: the instance labels of one raster."""

    return grow(start_of(mask, radius)).astype(np.int32)


def start_stitched(grid, radius):
    """L0 [T, H, W] in slot order of the one raster the grid's tiles form: absent tiles are unknown to the seeds and read 0 in the
    growth; labels are named by the smallest global index."""

    mask = grid.canvas != 0
    core = seeds(E.canvas(grid), radius, coded=True)
    return grid.cut(start(grid.global_labels(mask), grid.global_labels(core)))


def split_stitched(grid, radius):
    """int32 [T, H, W] in slot order: the instance labels of the one raster."""

    mask = grid.canvas != 0
    core = seeds(E.canvas(grid), radius, coded=True)
    return grid.cut(grow(start(grid.global_labels(mask), grid.global_labels(core)))).astype(np.int32)


# ---- masks ----------------------------------------------------------------------------------------------------------------
def dumbbell(h=64, w=64, y0=8, x0=4, side=21, neck=9, thick=3, vertical=False):
    """Two ``side`` x ``side`` squares joined at mid-height by a neck ``neck`` long and ``thick`` wide; ``vertical``: transposed."""

    m = np.zeros((w, h) if vertical else (h, w), dtype=bool)
    m[y0:y0 + side, x0:x0 + side] = True
    m[y0:y0 + side, x0 + side + neck:x0 + 2 * side + neck] = True
    top = y0 + (side - thick) // 2
    m[top:top + thick, x0 + side:x0 + side + neck] = True
    return m.T.copy() if vertical else m


def touching_blobs(h, w, seed, radius=9, salt=0.01):
    """Discs of about ``radius`` pixels on a jittered grid whose pitch is a little under their diameter, some left out: chains and
    sheets of blobs that touch or overlap slightly.  ``salt``: that share of the pixels is flipped (specks no core fits into, holes)."""

    rng = np.random.RandomState(seed)
    pitch = 2 * radius - 2
    m = np.zeros((h, w), dtype=bool)
    for cy in range(radius // 2, h + radius, pitch):
        for cx in range(radius // 2, w + radius, pitch):
            if rng.rand() < 0.2:
                continue
            r = radius + rng.randint(-2, 2)
            cy_, cx_ = cy + rng.randint(-2, 3), cx + rng.randint(-2, 3)
            y0, y1, x0, x1 = max(cy_ - r, 0), min(cy_ + r + 1, h), max(cx_ - r, 0), min(cx_ + r + 1, w)
            if y0 < y1 and x0 < x1:
                yy, xx = np.mgrid[y0:y1, x0:x1]
                m[y0:y1, x0:x1] |= np.hypot(yy - cy_, xx - cx_) <= r
    return m ^ (rng.rand(h, w) < salt)


def spiral_corridor():
    """48 x 48: ``features_ref.spiral(15)`` drawn three pixels to the cell -- a corridor 3 wide, its arms 3 apart, a pixel or two
    clear of the raster's edge (which would not erode it) -- with the outer end widened to 5 x 5: at radius 3 its centre is the only
    seed pixel, and the far end lies hundreds of steps away."""

    m = np.zeros((48, 48), dtype=bool)
    m[1:46, 1:46] = np.kron(R.spiral(15), np.ones((3, 3), dtype=bool))
    m[1:6, 1:6] = True
    return m
