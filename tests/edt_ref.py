"""Restatement in numpy of the capped squared distance transform (include/robosat_hip.h) on ONE raster, and of its stitched form on
the tiles pasted into one canvas (``stitch_ref.Grid``) whose other pixels are "unknown".  Not a test module;
``test_width_cpu.py`` pins it with a brute-force version and with ``scipy.ndimage.distance_transform_edt``.

A raster here is an integer array of UNSET (0), SET (1) and UNKNOWN (2) pixels.  Unknown pixels are neither: no distance comes from
them, and they have no result of their own (0 is written there).  Everything outside the array is unknown too."""

import numpy as np

UNSET, SET, UNKNOWN = 0, 1, 2


def _raster(mask, coded):
    """``coded``: the array holds UNSET / SET / UNKNOWN already; else it is a mask, non-zero = set."""

    return np.asarray(mask).astype(np.int64) if coded else (np.asarray(mask) != 0).astype(np.int64)


def row_distance(raster, radius):
    """g: per pixel, the horizontal distance to the nearest UNSET pixel of its row, capped at ``radius`` (``radius`` where the row has
    none within reach).  Set and unknown pixels alike are passed over."""

    h, w = raster.shape
    at = np.arange(w, dtype=np.int64)[None, :].repeat(h, 0)
    far = 4 * (w + radius)
    left = np.maximum.accumulate(np.where(raster == UNSET, at, -far), axis=1)  # column of the nearest unset pixel at or before x
    right = np.minimum.accumulate(np.where(raster == UNSET, at, far)[:, ::-1], axis=1)[:, ::-1]
    return np.minimum(np.minimum(at - left, right - at), radius)


def edt(mask, radius, coded=False):
    """int64 [H, W]: 0 at an unset (or unknown) pixel, min(radius^2, squared distance to the nearest unset pixel) at a set one, by
    the two passes of the definition: d2(x, y) = min(R*R, min over |dy| <= R of g(x, y + dy)^2 + dy^2), rows outside skipped."""

    raster = _raster(mask, coded)
    h, w = raster.shape
    g = row_distance(raster, radius)
    big = 2 * radius  # (a row that is not there: g^2 alone exceeds the cap)
    padded = np.full((h + 2 * radius, w), big, dtype=np.int64)
    padded[radius:radius + h] = g
    best = np.full((h, w), radius * radius, dtype=np.int64)
    for dy in range(-radius, radius + 1):
        best = np.minimum(best, padded[radius + dy:radius + dy + h] ** 2 + dy * dy)
    return np.where(raster == SET, best, 0)


def edt_brute(mask, radius, coded=False):
    """The definition itself, O(N^2): for rasters up to about 24 x 24."""

    raster = _raster(mask, coded)
    ys, xs = np.nonzero(raster == UNSET)
    out = np.zeros(raster.shape, dtype=np.int64)
    for y, x in zip(*np.nonzero(raster == SET)):
        nearest = int(((ys - y) ** 2 + (xs - x) ** 2).min()) if len(ys) else radius * radius
        out[y, x] = min(radius * radius, nearest)
    return out


def canvas(grid):
    """The grid's tiles (non-zero = set) pasted into one raster, UNKNOWN where no tile is."""

    return grid.paste((grid.stack != 0).astype(np.int64), fill=UNKNOWN)


def edt_stitched(grid, radius, brute=False):
    """int64 [T, H, W] in slot order: the transform of ``canvas(grid)``, cut back into the tiles."""

    return grid.cut((edt_brute if brute else edt)(canvas(grid), radius, coded=True))
