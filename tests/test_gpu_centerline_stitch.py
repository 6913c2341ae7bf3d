"""The stitched centerline stages on the MI355X: ``ops.thin_masks`` and ``ops.skeleton_links`` with the neighbour table equal the
restatements of tests/thin_ref.py applied to the ONE raster the tiles form (tests/stitch_ref.py: the tiles pasted into a zero
canvas, an absent tile 0), byte for byte and row for row."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 2  # thinning reads one pixel away and never grows: any margin does


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _content(h, w, seed):
    """Blobs and two roads at random angles; the caller adds the bars and the ring that sit on the seams."""

    return R.blobs(h, w, seed, 5) | T.roads(h, w, seed, count=2, width=9)


def _mosaic(layout, th, tw):
    """(image, absent) of a layout: bars through every seam, a ring round the first four-tile corner, blobs."""

    cols, rows, absent = {"2x2": (2, 2, ()), "3x3 hole": (3, 3, {(1, 1)}), "L": (2, 2, {(1, 0)}), "1x4": (4, 1, ())}[layout]
    h, w = rows * th, cols * tw
    m = _content(h, w, cols * 10 + rows)
    yy, xx = np.mgrid[:h, :w]
    m |= np.abs(yy - (th // 2 + 1)) <= 5  # a thick bar through every vertical seam of the first tile row
    if rows > 1:
        m |= np.abs(xx - (tw // 2 - 2)) <= 4  # and one through every horizontal seam of the first column
        r = np.hypot(yy - th + 0.5, xx - tw + 0.5)
        m |= (r >= 9) & (r <= 15)  # a ring round the four-tile corner
    if layout == "L":  # tiles (0, 0) and (1, 1) touch only at the corner: a one-pixel diagonal line through it, in a cleared window
        m[th - 7:th + 7, tw - 7:tw + 7] = np.eye(14, dtype=bool)
    return m.astype(np.uint8), absent


CASES = [(layout, th, tw) for layout in ("2x2", "3x3 hole", "L", "1x4") for th, tw in ((64, 64), (40, 50))]


def _run(grid, min_area=0):
    nbr, origin = grid.tables()
    nbr, origin = _dev(nbr), _dev(origin)
    masks = _dev(grid.stack)
    skeleton = ops.thin_masks(masks, nbr)
    labels = ops.stitch_labels(ops.label_components(masks), nbr)
    table = ops.component_table_stitched(labels, origin, min_area)
    links = ops.skeleton_links(skeleton, labels, table, nbr, origin)
    return skeleton.cpu().numpy(), links.cpu().numpy().astype(np.int64), table.cpu().numpy()


def _want_links(grid, skeleton_canvas, min_area):
    labels = grid.global_labels(grid.canvas)
    kept = grid.table(labels, min_area)[:, 0]
    rows = T.links(skeleton_canvas, labels, kept=kept)[:, 1:]
    rows[:, 1:3] -= grid.pad
    return R.sort_rows(rows)


@pytest.mark.parametrize("layout,th,tw", CASES)
def test_stitched_thinning_and_links_equal_the_restatement_on_the_canvas(layout, th, tw):
    image, absent = _mosaic(layout, th, tw)
    grid = S.Grid(S.split(image, th, tw, absent=absent, x0=5, y0=7), PAD)
    want = T.thin(grid.canvas)
    for min_area in (0, 60):
        got, links, table = _run(grid, min_area)
        assert got.dtype == np.uint8 and (got == grid.cut(want)).all(), int((got != grid.cut(want)).sum())
        want_links = _want_links(grid, want, min_area)
        links = R.sort_rows(links)
        assert links.shape == want_links.shape and (links == want_links).all()
    # the skeleton crosses seams: a link whose two pixels lie in different tiles (every component kept: the diagonal line is small)
    want_links = _want_links(grid, want, 0)
    lab, x, y, d = want_links[want_links[:, 3] >= 0].T
    x2, y2 = x + np.array([1, 1, 0, -1])[d], y + np.array([0, 1, 1, 1])[d]
    assert ((x // tw != x2 // tw) | (y // th != y2 // th)).any(), "no link across a seam: the test shows nothing"
    if layout == "L":
        assert ((x // tw != x2 // tw) & (y // th != y2 // th)).any(), "no link across the corner"


def test_the_stitched_skeleton_differs_from_the_per_tile_one():
    """A bar through a seam: per tile it stops half its width short of the seam on either side, stitched it runs through.  A
    stitched thinning that ignored ``nbr`` would give the per-tile bytes."""

    image = np.zeros((64, 128), np.uint8)
    image[20:40, :] = 1
    grid = S.Grid(S.split(image, 64, 64), PAD)
    nbr = _dev(grid.tables()[0])
    stitched = ops.thin_masks(_dev(grid.stack), nbr).cpu().numpy()
    per_tile = ops.thin_masks(_dev(grid.stack)).cpu().numpy()
    assert (stitched == grid.cut(T.thin(grid.canvas))).all()
    assert (per_tile == np.stack([T.thin(t) for t in grid.stack])).all()
    assert stitched[0, :, 63].any() and stitched[1, :, 0].any(), "the stitched skeleton crosses the seam"
    assert not per_tile[0, :, 55:].any() and not per_tile[1, :, :9].any(), "the per-tile skeleton stops short of it"


def test_a_mosaic_of_512_pixel_tiles():
    h = w = 1024
    yy, xx = np.mgrid[:h, :w]
    m = (np.abs(yy - 500) <= 12) | (np.abs(xx - 520) <= 10) | (np.abs((xx - yy) - 40) <= 14)
    r = np.hypot(yy - 511.5, xx - 511.5)
    m |= (r >= 150) & (r <= 170)
    grid = S.Grid(S.split(m.astype(np.uint8), 512, 512), PAD)
    want = T.thin(grid.canvas)
    got, links, _ = _run(grid)
    assert (got == grid.cut(want)).all()
    assert (R.sort_rows(links) == _want_links(grid, want, 0)).all()


def test_stitched_centerlines_runs_every_stage():
    image, absent = _mosaic("2x2", 64, 64)
    other = np.where(image != 0, np.uint8(2), np.uint8(1))
    grid = S.Grid(S.split(other, 64, 64, x0=1, y0=1), S.margin(3, 4))
    nbr, origin = grid.tables()
    table, links = ops.stitched_centerlines(_dev(grid.stack), _dev(nbr), _dev(origin), 2, 3, 4, min_area=40)
    cleaned = R.clean(grid.canvas, 2, 3, 4) * (grid.index >= 0)
    labels = grid.global_labels(cleaned)
    assert (table.cpu().numpy() == grid.table(labels, 40)).all()
    rows = T.links(T.thin(cleaned), labels, kept=grid.table(labels, 40)[:, 0])[:, 1:]
    rows[:, 1:3] -= grid.pad
    assert (R.sort_rows(links.cpu().numpy().astype(np.int64)) == R.sort_rows(rows)).all()
