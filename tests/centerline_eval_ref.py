"""Restatement in numpy of ``rs evaluate --centerline`` (include/robosat_hip.h, rs_eval_centerline): the links of two skeletons by
the rule of ``thin_ref.links`` without its labels, the reach from ``edt_ref.edt`` on the complement of a skeleton, and the eight
counts; per tile, and for the tiles pasted into one canvas (``stitch_ref.Grid``) whose other pixels are unknown.  Not a test
module; ``test_evaluate_centerline_cpu.py`` pins the reach with a brute-force version."""

import numpy as np

import edt_ref as E
import thin_ref as T


def link_masks(skeleton):
    """{dir: bool [H, W]}: where the link of that direction starts (0 E, 1 SE, 2 S, 3 SW), a pixel outside reading 0."""

    s = np.asarray(skeleton) != 0
    _, _, p4, p5, p6, p7, p8, _ = T._neighbours(s)
    return {0: s & p4, 2: s & p6, 1: s & p5 & ~p4 & ~p6, 3: s & p7 & ~p8 & ~p6}


def near(skeleton, rho, known=None):
    """bool [H, W]: the pixels within ``rho`` of a pixel of ``skeleton``, by the transform of its complement with R = rho + 1.
    ``known`` (bool, stitched): the pixels that tiles cover; the others are unknown to the transform and are near nothing."""

    s = np.asarray(skeleton) != 0
    raster = np.where(s, E.UNSET, E.SET)
    if known is not None:
        raster = np.where(known, raster, E.UNKNOWN)
    d2 = E.edt(raster, rho + 1, coded=True)
    out = d2 <= rho * rho
    return out if known is None else out & known


def near_brute(skeleton, rho):
    """The definition itself on one raster: min over the skeleton's pixels p of |p - q|^2 <= rho^2."""

    s = np.asarray(skeleton) != 0
    ys, xs = np.nonzero(s)
    out = np.zeros(s.shape, dtype=bool)
    if len(ys):
        for y in range(s.shape[0]):
            for x in range(s.shape[1]):
                out[y, x] = int(((ys - y) ** 2 + (xs - x) ** 2).min()) <= rho * rho
    return out


def side_counts(skeleton, near_other):
    """(straight, diagonal, matched straight, matched diagonal) as bool rasters' sums would give them, but kept PER PIXEL of the
    link's first end: int64 [4, H, W], so that a caller can sum them per tile."""

    h, w = np.asarray(skeleton).shape
    padded = np.pad(near_other, 1)
    out = np.zeros((4, h, w), dtype=np.int64)
    for d, exists in link_masks(skeleton).items():
        dx, dy = T.STEP[d]
        both = near_other & padded[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        out[d & 1] += exists
        out[2 + (d & 1)] += exists & both
    return out


def counts(skel_p, skel_g, rho):
    """The eight counts of ONE raster as Python integers."""

    p = side_counts(skel_p, near(skel_g, rho)).sum(axis=(1, 2))
    g = side_counts(skel_g, near(skel_p, rho)).sum(axis=(1, 2))
    return [int(v) for v in list(p) + list(g)]


def counts_tiles(stack_p, stack_g, rho):
    """[B][8]: every tile a raster of its own."""

    return [counts(p, g, rho) for p, g in zip(stack_p, stack_g)]


def counts_grid(grid_p, grid_g, rho, per_tile=False):
    """The eight counts of the one raster two ``stitch_ref.Grid``s of the same tiles form; ``per_tile``: [T][8] in slot order, a link
    counted in the tile of its first pixel (their sum is the call's one group)."""

    known = grid_p.index >= 0
    p = side_counts(grid_p.canvas, near(grid_g.canvas, rho, known))
    g = side_counts(grid_g.canvas, near(grid_p.canvas, rho, known))
    both = np.concatenate([p, g])
    if not per_tile:
        return [int(v) for v in both.sum(axis=(1, 2))]
    return [[int(v) for v in plane.sum(axis=(1, 2))] for plane in np.stack([grid_p.cut(c) for c in both], axis=1)]
