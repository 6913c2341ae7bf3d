"""Restatement in numpy of ``rs evaluate --type --ignored unknown`` (include/robosat_hip.h): the two rasters coded UNSET /
SET / UNKNOWN, and on them the boundary bands, the objects and the centre-line counts, per tile and for the tiles pasted into one
canvas (``stitch_ref.Grid``; a canvas pixel that no tile covers is UNKNOWN as well).  Not a test module;
``test_evaluate_ignore_cpu.py`` pins the coded band against ``edt_ref.edt_brute``.

a is the label raster, p the mask raster, t the class, I the ignore value: U = {a == I}, P = {p == t} \\ U, G = {a == t}."""

import numpy as np

import centerline_eval_ref as C
import edt_ref as E
import eval_ref as V
import features_ref as R
import stitch_ref as S
import thin_ref as T


def coded(p, a, t, I):
    """(cP, cG), int64 arrays of the rasters' shape: 2 on U, 1 on P (on G), 0 elsewhere."""

    p, a = np.asarray(p), np.asarray(a)
    unknown = a == I
    return (np.where(unknown, E.UNKNOWN, np.where(p == t, E.SET, E.UNSET)).astype(np.int64),
            np.where(unknown, E.UNKNOWN, np.where(a == t, E.SET, E.UNSET)).astype(np.int64))


def band(c, d):
    """bool [H, W]: the SET pixels of one coded raster with 1 <= d2 <= d*d, d2 = ``edt_ref.edt(c, d + 1, coded=True)``."""

    return V.band(c, d, coded=True)


def band_counts(cp, cg, d):
    """Coded rasters [B, H, W] twice -> int64 [B, 3]: (|P_D|, |G_D|, |P_D and G_D|) per tile."""

    return V.boundary(np.stack([band(c, d) for c in cp]), np.stack([band(c, d) for c in cg]))


def grid(tiles):
    """{(tx, ty): coded tile} -> a ``stitch_ref.Grid`` whose ``canvas`` is coded too: UNKNOWN where no tile is."""

    g = S.Grid(tiles, 0)
    g.canvas = g.paste(g.stack, fill=E.UNKNOWN)
    return g


def band_counts_grid(grid_p, grid_g, d):
    """int64 [3]: the counts of the one raster the tiles of two ``grid``s form."""

    return V.boundary(band(grid_p.canvas, d)[None], band(grid_g.canvas, d)[None], stitched=True)[0]


def objects(cp, cg, threshold, min_area=0):
    """Coded rasters [B, H, W] twice -> ``eval_ref.match`` of the 4-connected components of the SET pixels, every tile on its own."""

    return V.match([R.label(c == E.SET) for c in cp], [R.label(c == E.SET) for c in cg], threshold, min_area)


def objects_grid(grid_p, grid_g, threshold, min_area=0):
    return V.match([R.label(grid_p.canvas == E.SET)], [R.label(grid_g.canvas == E.SET)], threshold, min_area)


def _links(c_p, c_g, rho):
    """The eight counts of ONE pair of coded rasters: the SET pixels thinned, the reach taken with the unknown pixels coded
    unknown (``centerline_eval_ref.near`` with ``known``)."""

    known = c_g != E.UNKNOWN
    assert (known == (c_p != E.UNKNOWN)).all(), "U is the same on both sides"
    sk_p, sk_g = T.thin((c_p == E.SET).astype(np.uint8)), T.thin((c_g == E.SET).astype(np.uint8))
    p = C.side_counts(sk_p, C.near(sk_g, rho, known)).sum(axis=(1, 2))
    g = C.side_counts(sk_g, C.near(sk_p, rho, known)).sum(axis=(1, 2))
    return [int(v) for v in list(p) + list(g)]


def centerline_counts(cp, cg, rho):
    """[B][8]: every tile a raster of its own."""

    return [_links(p, g, rho) for p, g in zip(cp, cg)]


def centerline_counts_grid(grid_p, grid_g, rho):
    """[8]: of the one raster the tiles form."""

    return _links(grid_p.canvas, grid_g.canvas, rho)
