"""``rs features --stitch`` raster stages on the MI355X, through the ops wrappers.  Every expected value is a restatement of
tests/features_ref.py applied to ONE raster: the tiles pasted into a zero canvas with a margin of 2 * (eps_open + eps_close) + 2
pixels (tests/stitch_ref.py), where the restatement's own border rule cannot reach the content."""

import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import ops  # noqa: E402
from robosat_amd.features import featurize_stitched  # noqa: E402
from robosat_amd.tiles import Tile  # noqa: E402

pytestmark = pytest.mark.gpu

INDEX = 2


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _tables(grid):
    nbr, origin = grid.tables()
    return _dev(nbr), _dev(origin)


# ---- gather / crop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("apron", [1, 5, 16])
def test_gather_is_a_slice_of_the_canvas_and_crop_undoes_it(apron):
    rng = np.random.RandomState(apron)
    image = rng.randint(1, 256, size=(3 * 16, 3 * 24)).astype(np.uint8)  # no zeros: an absent neighbour's 0 cannot pass for content
    grid = S.Grid(S.split(image, 16, 24, absent={(2, 1)}, x0=7, y0=3), 16)
    nbr, _ = _tables(grid)
    got = ops.gather_halo(_dev(grid.stack), nbr, apron)
    assert got.shape == (8, 16 + 2 * apron, 24 + 2 * apron) and got.dtype == torch.uint8
    assert (got.cpu().numpy() == grid.cut(grid.canvas, apron)).all()
    assert (ops.crop_halo(got, apron).cpu().numpy() == grid.stack).all()
    filled = ops.gather_halo(_dev(grid.stack), nbr, apron, fill=255).cpu().numpy()
    want = grid.cut(np.where(grid.index < 0, 255, grid.canvas).astype(np.uint8), apron)
    assert (filled == want).all()


def test_gather_refuses_an_apron_beyond_the_tile():
    grid = S.Grid(S.split(np.ones((16, 48), np.uint8), 16, 24), 0)
    nbr, _ = _tables(grid)
    with pytest.raises(ValueError):
        ops.gather_halo(_dev(grid.stack), nbr, 17)
    big = S.Grid({(0, 0): np.zeros((4000, 4000), np.uint8)}, 0)
    with pytest.raises(ValueError):
        ops.gather_halo(_dev(big.stack), _dev(big.tables()[0]), 49)  # 4000 + 2 * 49 > 4096


# ---- clean -------------------------------------------------------------------------------------------------------------
def _clean_image():
    """64 x 96 (3 x 2 tiles of 32 x 32): blobs, several across seams, and speckle within 3 px of the seams."""

    h, w = 64, 96
    m = R.blobs(h, w, 11, 9)
    yy, xx = np.mgrid[:h, :w]
    for cy, cx, ry, rx in ((32, 20, 9, 7), (36, 62, 13, 15), (12, 32, 6, 9), (50, 63, 7, 8), (33, 33, 5, 5)):  # on the seams and the corner
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    near = (np.abs(yy - 31.5) < 3.5) | (np.abs(xx - 31.5) < 3.5) | (np.abs(xx - 63.5) < 3.5)
    m ^= R.noise(h, w, 12, 0.25) & near
    m |= ((yy - 36) / 13) ** 2 + ((xx - 62) / 15) ** 2 <= 1  # one solid blob on the four-tile corner that a 16-pixel disc fits in
    other = np.random.RandomState(13).choice(np.array([0, 1, 3], dtype=np.uint8), size=(h, w))
    return np.where(m, np.uint8(INDEX), other)


@pytest.mark.parametrize("eps_open,eps_close", [(0, 0), (3, 0), (0, 4), (5, 6), (16, 16)])
def test_clean_equals_the_restatement_on_the_canvas(eps_open, eps_close):
    grid = S.Grid(S.split(_clean_image(), 32, 32, absent={(1, 0)}, x0=4, y0=9), S.margin(eps_open, eps_close))
    nbr, _ = _tables(grid)
    want = grid.cut(R.clean(grid.canvas, INDEX, eps_open, eps_close))
    got = ops.clean_masks_stitched(_dev(grid.stack), nbr, INDEX, eps_open, eps_close).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert (got == want).all(), (eps_open, eps_close, int((got != want).sum()))
    # what the restatement leaves outside the tiles (the absent tile, the margin) is nobody's output: closing may grow into it
    if (eps_open, eps_close) == (5, 6):
        alone = ops.clean_masks(_dev(grid.stack), INDEX, eps_open, eps_close).cpu().numpy()
        assert (alone != want).any(), "the per-tile path agrees on this input: the test shows nothing"


def test_clean_of_class_zero_fills_the_apron_with_another_byte():
    image = np.where(R.blobs(32, 64, 5), 0, 1).astype(np.uint8)  # class 0 is the blobs
    grid = S.Grid(S.split(image, 32, 32, x0=0, y0=0), S.margin(3, 4))
    canvas = np.where(grid.index < 0, 1, grid.canvas)  # outside the tiles is "not the class"
    got = ops.clean_masks_stitched(_dev(grid.stack), _tables(grid)[0], 0, 3, 4).cpu().numpy()
    assert (got == grid.cut(R.clean(canvas, 0, 3, 4))).all()


# ---- labels ------------------------------------------------------------------------------------------------------------
def _u_shape():
    m = np.zeros((32, 32), dtype=bool)  # leaves tile (0, 0) downwards, runs through (0, 1), (1, 1) and (1, 0), and comes back into (0, 0)
    m[4:28, 5] = True
    m[27, 5:28] = True
    m[8:28, 27] = True
    m[8, 12:28] = True  # back across the seam x = 16 into the first tile, where it ends apart from the start
    return m


def _corner_pixels():
    m = np.zeros((32, 32), dtype=bool)
    m[15, 15] = m[16, 16] = True  # diagonal across the four-tile corner
    m[15, 17] = m[17, 15] = True  # and two more that touch those only diagonally
    m[15, 16] = m[16, 15] = False
    return m


def _label_cases():
    two = np.zeros((16, 48), dtype=bool)
    two[3:12, 2:16] = True  # reaches the seam of the absent middle tile
    two[3:12, 32:40] = True
    corner4 = np.zeros((32, 32), dtype=bool)
    corner4[15, 15] = corner4[16, 16] = corner4[15, 16] = corner4[16, 15] = True
    return {
        "spiral": (R.spiral(48), ()), "comb": (R.comb(48), ()), "checkerboard": (R.checkerboard(48, 48), ()),
        "u_shape": (_u_shape(), ()), "diagonals": (_corner_pixels(), ()), "corner_block": (corner4, ()),
        "absent_between": (two, {(1, 0)}), "blobs_with_a_hole": (R.blobs(48, 48, 2, 9), {(1, 1)}),
    }


@pytest.mark.parametrize("name", sorted(_label_cases()))
def test_stitched_labels_are_the_canonical_labels_of_the_canvas(name):
    mask, absent = _label_cases()[name]
    grid = S.Grid(S.split(mask.astype(np.uint8), 16, 16, absent=absent, x0=3, y0=5), 2)
    nbr, _ = _tables(grid)
    per_tile = ops.label_components(_dev(grid.stack))
    got = ops.stitch_labels(per_tile, nbr)  # (raises if the device's err word is non-zero)
    pasted = grid.paste(got.cpu().numpy())
    reference = R.label(grid.canvas)
    assert (R.canonical(pasted) == R.canonical(reference)).all(), "another partition"
    assert (pasted == grid.global_labels(grid.canvas)).all(), "label != 1 + min(global index)"
    assert torch.equal(ops.stitch_labels(ops.label_components(_dev(grid.stack)), nbr), got), "a second run differs"
    count = len(np.unique(reference)) - 1
    if name == "diagonals":
        assert count == 4
    if name == "corner_block":
        assert count == 1
    if name == "checkerboard":
        assert count == 48 * 48 // 2
    if name in ("spiral", "comb", "u_shape"):
        assert count == 1
    if name == "absent_between":
        assert count == 2


# ---- table, edges ------------------------------------------------------------------------------------------------------
def _stitched_labels(grid):
    nbr, origin = _tables(grid)
    return ops.stitch_labels(ops.label_components(_dev(grid.stack)), nbr), nbr, origin


def _area_mask():
    m = np.zeros((32, 48), dtype=bool)
    m[13:19, 13:19] = True  # 36 pixels, 9 in each of four tiles
    m[2:7, 34:43] = True  # 45 pixels inside one tile
    m[20:23, 40:44] = True  # 12 pixels inside one tile
    m[15:17, 30:34] = True  # 8 pixels, 2 in each of four tiles
    return m


@pytest.mark.parametrize("min_area", [0, 10, 20, 40])
def test_table_has_whole_areas_and_mosaic_boxes(min_area):
    grid = S.Grid(S.split(_area_mask().astype(np.uint8), 16, 16, x0=1, y0=1), 2)
    labels, nbr, origin = _stitched_labels(grid)
    want = grid.table(grid.global_labels(grid.canvas), min_area)
    got = ops.component_table_stitched(labels, origin, min_area).cpu().numpy()
    assert got.dtype == np.int32 and (got == want).all(), (got, want)
    areas = sorted(got[:, 1].tolist())
    assert areas == [a for a in (8, 12, 36, 45) if a >= min_area]
    if min_area == 20:  # four parts of 9 each: the per-tile rule drops the square, the stitched rule keeps it
        per_tile = ops.component_table(ops.label_components(_dev(grid.stack)), min_area).cpu().numpy()
        assert 36 in areas and sorted(per_tile[:, 2].tolist()) == [45]
    if min_area == 40:  # the reverse: the whole square is below the threshold and goes, whatever its parts
        assert 36 not in areas


@pytest.mark.parametrize("name", ["areas", "blobs", "spiral", "absent"])
def test_edges_are_the_boundary_of_the_canvas_labels(name):
    mask, absent, min_area = {"areas": (_area_mask(), (), 10), "blobs": (R.blobs(48, 48, 4, 9), (), 0), "spiral": (R.spiral(32), (), 0),
                              "absent": (R.blobs(48, 48, 6, 12), {(1, 1), (2, 0)}, 5)}[name]
    grid = S.Grid(S.split(mask.astype(np.uint8), 16, 16, absent=absent, x0=10, y0=20), 2)
    labels, nbr, origin = _stitched_labels(grid)
    reference = R.filter_labels(grid.global_labels(grid.canvas), min_area)
    table = ops.component_table_stitched(labels, origin, min_area)
    got = R.sort_rows(ops.boundary_edges_stitched(labels, nbr, origin, table).cpu().numpy())
    want = grid.edges(reference)
    assert got.shape == want.shape and (got == want).all()
    # no edge on a seam between two pixels of one component
    lab, x, y, d = got.T.astype(np.int64)
    step_x, step_y = np.array([0, 1, 0, -1])[d], np.array([-1, 0, 1, 0])[d]
    across = reference[y + step_y + grid.pad, x + step_x + grid.pad]  # (the margin keeps this inside the canvas)
    assert (reference[y + grid.pad, x + grid.pad] == lab).all() and (across != lab).all()
    # (and the input has such pairs: the per-tile kernels would emit two edges for each)
    inner = reference[grid.pad:-grid.pad, grid.pad:-grid.pad]
    assert ((inner[:, 15:-1:16] != 0) & (inner[:, 15:-1:16] == inner[:, 16::16])).any()
    assert ((inner[15:-1:16, :] != 0) & (inner[15:-1:16, :] == inner[16::16, :])).any()
    assert len(ops.boundary_edges_stitched(labels, nbr, origin, table[:0])) == 0


# ---- decomposition invariance ------------------------------------------------------------------------------------------
def test_the_polygons_do_not_depend_on_how_the_raster_is_tiled():
    """One 96 x 96 raster as 1 x 1, 2 x 2 and 3 x 3 tiles through every stage and ``featurize_stitched`` with simplify = 0.  The
    geometries are compared in mosaic pixels (georeference=False): a 96-pixel tile and a 32-pixel tile at one zoom level are not
    the same place on the map.  Labels, hence the order of the features, follow the slot order; the lists are compared sorted."""

    rng = np.random.RandomState(21)
    image = np.where(R.blobs(96, 96, 20, 14), np.uint8(INDEX), rng.choice(np.array([0, 1, 3], dtype=np.uint8), size=(96, 96)))
    results = []
    for n in (1, 2, 3):
        size = 96 // n
        grid = S.Grid(S.split(image, size, size, x0=40, y0=50), 0)
        nbr, origin = _tables(grid)
        table, edges = ops.stitched_features(_dev(grid.stack), nbr, origin, INDEX, 5, 6, min_area=9)
        feats = featurize_stitched(edges.cpu().numpy(), table.cpu().numpy(), [Tile(x, y, 18) for x, y in grid.coords], (size, size),
                                   simplify=0, georeference=False)
        assert all(f["properties"]["stitched"] is True for f in feats)
        results.append(sorted(json.dumps(f["geometry"]) for f in feats))
        areas = sorted(f["properties"]["area_px"] for f in feats)
        assert n == 1 or areas == first_areas
        first_areas = areas
    assert len(results[0]) >= 3 and results[0] == results[1] == results[2]
    # and they are the restated components of the raster
    pad = S.margin(5, 6)
    cleaned = R.clean(np.pad(image, pad), INDEX, 5, 6)[pad:-pad, pad:-pad]  # (what closing grows beyond the raster is no tile's pixel)
    reference = R.filter_labels(R.label(cleaned), 9)
    assert len(results[0]) == len(np.unique(reference)) - 1
