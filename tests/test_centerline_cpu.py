"""Pins the centerline restatements (tests/thin_ref.py) with scipy.ndimage.label, and covers the host half of
``rs features --geometry centerline`` (robosat_amd/features.py: link_lines, prune_lines, simplify_line, georeferencing).  No GPU."""

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd.features import (centerlines, centerlines_stitched, line_length, link_lines, mosaic_centre_location, prune_lines,  # noqa: E402
                                  simplify_line)
from robosat_amd.tiles import Tile, pixel_to_location  # noqa: E402

ndimage = pytest.importorskip("scipy.ndimage")
EIGHT = np.ones((3, 3), dtype=int)


def _masks():
    out = {}
    for h, w in ((1, 1), (2, 2), (7, 5), (31, 33), (64, 64), (65, 63), (100, 130)):
        size = "{}x{}".format(h, w)
        out["blobs " + size] = R.blobs(h, w, h + w)
        out["noise .5 " + size] = R.noise(h, w, h, 0.5)
        out["noise .9 " + size] = R.noise(h, w, w, 0.9)
        out["full " + size] = np.ones((h, w), dtype=bool)
        if h > 2 and w > 2:
            out["border " + size] = R.border(h, w)
        out["cleaned noise " + size] = R.clean(R.noise(h, w, 3, 0.6).astype(np.uint8), 1, 3, 3).astype(bool)
    out["roads 128x128"] = T.roads(128, 128, 1)
    return out


@pytest.mark.parametrize("name", sorted(_masks()))
def test_the_five_invariants_of_the_restated_skeleton(name):
    mask = _masks()[name]
    skeleton = T.thin(mask).astype(bool)
    assert (skeleton <= mask).all(), "the skeleton is part of the mask"
    count = ndimage.label(skeleton, EIGHT)[1]
    assert ndimage.label(mask, EIGHT)[1] == count, "8-connected foreground components"
    assert ndimage.label(~np.pad(mask, 1))[1] == ndimage.label(~np.pad(skeleton, 1))[1], "4-connected background components (holes)"
    assert (T.thin(skeleton) == skeleton).all(), "thinning a skeleton changes nothing"
    rows = T.links(skeleton, R.label(mask))
    assert T.link_components(rows, mask.shape) == count, "the link graph's components are the skeleton's"
    # every skeleton pixel is named by a row, and each link appears once
    named = set()
    for _, _, x, y, d in rows.tolist():
        named.add((x, y))
        if d >= 0:
            named.add((x + T.STEP[d][0], y + T.STEP[d][1]))
    assert len(named) == int(skeleton.sum()) and len({tuple(r) for r in rows.tolist()}) == len(rows)


def test_fixed_points_and_the_figures_of_the_design_notes():
    assert T.thin(np.ones((2, 2), bool)).sum() == 1, "a 2 x 2 block ends as one pixel"
    assert (T.thin(np.ones((1, 1), bool)) == 1).all()
    line = np.zeros((9, 40), bool)
    line[4, 3:37] = True
    assert (T.thin(line) == line).all(), "a one-pixel-wide line is a skeleton"
    thinned = T.thin(R.spiral(24))  # (its square corners go: an L's corner pixel is redundant for 8-connectivity)
    assert (thinned <= R.spiral(24)).all() and (R.spiral(24) != thinned).any() and ndimage.label(thinned, EIGHT)[1] == 1
    assert T.thin(np.ones((256, 256), bool), want_pairs=True)[1] == 129  # S/2 + 1 pairs for a full S x S tile
    bar = np.zeros((60, 200), bool)
    bar[20:40, :] = True
    ys, xs = np.nonzero(T.thin(bar))
    assert (xs.min(), xs.max()) == (9, 189) and len(set(ys.tolist())) == 1  # ends half the width short of the borders it touches


def test_links_with_a_dropped_component_keep_what_touches_a_kept_one():
    s = np.zeros((6, 8), bool)
    s[1, 1:4] = True  # component A (3 pixels), meets B only diagonally
    s[2, 4:7] = True  # component B
    s[4, 1] = True  # a lone pixel
    labels = R.label(s)
    a, b, lone = int(labels[1, 1]), int(labels[2, 4]), int(labels[4, 1])
    every = T.links(s, labels)
    assert len(every) == 6 and [-1] == [r[4] for r in every.tolist() if r[1] == lone]
    only_b = T.links(s, labels, kept=[b])
    assert sorted(map(tuple, only_b[:, 1:].tolist())) == [(b, 3, 1, 1), (b, 4, 2, 0), (b, 5, 2, 0)]  # the diagonal link survives under B's label
    assert len(T.links(s, labels, kept=[a])) == 3 and len(T.links(s, labels, kept=[])) == 0


# ---- link_lines ----------------------------------------------------------------------------------------------------------------
def _rows(skeleton):
    skeleton = np.asarray(skeleton, dtype=bool)
    return T.links(skeleton, R.label(skeleton))


def _draw(h, w, *runs):
    m = np.zeros((h, w), bool)
    for y0, y1, x0, x1 in runs:
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def _points(lines):
    return [line[2].tolist() for line in lines]


def test_a_straight_line_an_l_and_a_staircase_are_one_line_each():
    straight = link_lines(_rows(_draw(5, 12, (2, 2, 1, 10))))
    assert _points(straight) == [[[x, 2] for x in range(1, 11)]]
    corner = link_lines(_rows(_draw(8, 8, (1, 6, 2, 2), (6, 6, 2, 6))))
    assert len(corner) == 1 and len(corner[0][2]) == 10 and corner[0][2][0].tolist() == [2, 1] and corner[0][2][-1].tolist() == [6, 6]
    stairs = np.zeros((8, 8), bool)
    for i in range(6):
        stairs[i + 1, i + 1] = stairs[i + 1, i + 2] = True  # every corner has an orthogonal detour: no diagonal links, no junction
    got = link_lines(_rows(stairs))
    assert len(got) == 1 and len(got[0][2]) == 12
    diagonal = link_lines(_rows(np.eye(6, dtype=bool)))
    assert _points(diagonal) == [[[i, i] for i in range(6)]] and line_length(diagonal[0][2]) == pytest.approx(5 * math.sqrt(2))


def test_t_and_plus_give_three_and_four_lines_at_one_node():
    tee = link_lines(_rows(_draw(9, 9, (1, 1, 1, 7), (1, 7, 4, 4))))
    assert len(tee) == 3 and sum(1 for p in _points(tee) if [4, 1] in (p[0], p[-1])) == 3
    plus = link_lines(_rows(_draw(9, 9, (4, 4, 0, 8), (0, 8, 4, 4))))
    assert len(plus) == 4 and all([4, 4] in (p[0], p[-1]) for p in _points(plus))
    assert all(not (line[2][0] == line[2][-1]).all() for line in plus)


def _ring():
    m = _draw(9, 9, (1, 1, 1, 6), (6, 6, 1, 6), (1, 6, 1, 1), (1, 6, 6, 6))
    return m


def test_a_ring_is_one_closed_line_and_a_tail_hangs_it_on_a_node():
    ring = link_lines(_rows(_ring()))
    assert len(ring) == 1
    points = ring[0][2].tolist()
    assert points[0] == points[-1] == [1, 1] and points[1] == [1, 2] and len(points) == 21  # smallest pixel, towards the smaller neighbour
    tailed = _ring()
    tailed[6, 6:9] = True
    lines = link_lines(_rows(tailed))
    assert len(lines) == 2
    loop = [p for p in _points(lines) if p[0] == p[-1]]
    tail = [p for p in _points(lines) if p[0] != p[-1]]
    assert len(loop) == 1 and loop[0][0] == [6, 6] and len(tail) == 1 and tail[0] == [[6, 6], [7, 6], [8, 6]]


def test_an_isolated_pixel_is_a_line_of_one_point():
    m = np.zeros((5, 5), bool)
    m[2, 3] = True
    lines = link_lines(_rows(m))
    assert _points(lines) == [[[3, 2]]] and lines[0][1] == 2 * 5 + 3 + 1


def test_lines_do_not_depend_on_the_order_of_the_rows():
    mask = T.roads(96, 96, 4, count=4, width=8) | R.blobs(96, 96, 2, 3)
    rows = T.links(T.thin(mask), R.label(mask))
    rows = np.concatenate([rows, rows + np.array([1, 0, 0, 0, 0])])  # a second tile with the same content
    want = link_lines(rows)
    assert {line[0] for line in want} == {0, 1} and len(want) > 6
    for seed in range(3):
        got = link_lines(rows[np.random.RandomState(seed).permutation(len(rows))])
        assert [(t, l, p.tolist()) for t, l, p in got] == [(t, l, p.tolist()) for t, l, p in want]
        pruned, pruned_want = prune_lines(got, 12), prune_lines(want, 12)
        assert [(t, l, p.tolist()) for t, l, p in pruned] == [(t, l, p.tolist()) for t, l, p in pruned_want]
    stitched = link_lines(rows[rows[:, 0] == 0][:, 1:])  # rows of four are tile 0
    assert [p.tolist() for _, _, p in stitched] == [p.tolist() for t, _, p in want if t == 0]


# ---- prune_lines ---------------------------------------------------------------------------------------------------------------
def _y_shape():
    m = _draw(40, 40, (20, 20, 2, 20))  # west arm, 18 links
    for i in range(1, 16):
        m[20 - i, 20 + i] = True  # north-east arm, 15 diagonal links
    m[21:25, 20] = True  # south arm: 4 links
    return m


def test_a_y_loses_its_short_arm_and_becomes_one_line():
    lines = link_lines(_rows(_y_shape()))
    assert len(lines) == 3
    pruned = prune_lines(lines, 10)
    assert len(pruned) == 1 and len(pruned[0][2]) == 19 + 15
    assert pruned[0][2][0].tolist() == [2, 20] and pruned[0][2][-1].tolist() == [35, 5]
    assert line_length(pruned[0][2]) == pytest.approx(18 + 15 * math.sqrt(2))
    assert len(prune_lines(lines, 4)) == 3, "a spur of length 4 is not below 4"
    # every arm below the threshold: the junction keeps its two longest line ends
    assert len(prune_lines(lines, 100)) == 1 and len(prune_lines(lines, 100)[0][2]) == 19 + 15


def test_prune_is_idempotent_keeps_every_component_and_zero_is_the_identity():
    mask = T.roads(128, 128, 1) | R.blobs(128, 128, 3, 4)
    skeleton = T.thin(mask)
    lines = link_lines(T.links(skeleton, R.label(mask)))
    same = prune_lines(lines, 0)
    assert [(t, l, p.tolist()) for t, l, p in same] == [(t, l, p.tolist()) for t, l, p in lines]
    components = ndimage.label(skeleton, EIGHT)[1]
    for prune in (5, 20, 1000):
        pruned = prune_lines(lines, prune)
        again = prune_lines(pruned, prune)
        assert [p.tolist() for _, _, p in again] == [p.tolist() for _, _, p in pruned]
        assert len(pruned) <= len(lines)
        left = np.zeros(mask.shape, bool)
        for _, _, points in pruned:
            left[points[:, 1], points[:, 0]] = True
        assert (left <= skeleton.astype(bool)).all() and ndimage.label(left, EIGHT)[1] == components, "a component vanished or fell apart"
    assert len(prune_lines(lines, 20)) < len(lines), "nothing was pruned: the test shows nothing"
    ring = link_lines(_rows(_ring()))
    assert [p.tolist() for _, _, p in prune_lines(ring, 1000)] == _points(ring), "a cycle is never a spur"
    both_ends = link_lines(_rows(_draw(3, 9, (1, 1, 1, 6))))
    assert _points(prune_lines(both_ends, 1000)) == _points(both_ends), "a line between two ends is never a spur"


# ---- simplify_line -------------------------------------------------------------------------------------------------------------
def test_simplify_keeps_the_ends_and_drops_what_the_tolerance_allows():
    run = np.array([[x, 3] for x in range(12)])
    assert simplify_line(run, 1.5).tolist() == [[0, 3], [11, 3]]
    assert simplify_line(run, 0).tolist() == [[0, 3], [11, 3]]
    bent = np.array([[0, 0], [1, 0], [2, 0], [3, 1], [4, 2], [5, 2], [6, 2]])
    assert simplify_line(bent, 0).tolist() == [[0, 0], [2, 0], [4, 2], [6, 2]], "tolerance 0 drops collinear vertices only"
    coarse = simplify_line(bent, 1.5)
    assert coarse[0].tolist() == [0, 0] and coarse[-1].tolist() == [6, 2] and len(coarse) == 2
    wiggle = np.array([[x, (x // 3) % 2] for x in range(30)])
    for tolerance in (0.4, 1.0):
        kept = simplify_line(wiggle, tolerance)
        assert kept[0].tolist() == [0, 0] and kept[-1].tolist() == [29, 1]
        assert {tuple(p) for p in kept.tolist()} <= {tuple(p) for p in wiggle.tolist()}
    assert len(simplify_line(wiggle, 0.4)) > len(simplify_line(wiggle, 1.0)) == 2
    closed = np.array(link_lines(_rows(_ring()))[0][2])
    kept = simplify_line(closed, 0.5)
    assert kept[0].tolist() == kept[-1].tolist() == [1, 1] and sorted(map(tuple, kept[:-1].tolist())) == [(1, 1), (1, 6), (6, 1), (6, 6)]
    assert simplify_line(np.array([[1, 1], [2, 2]]), 5).tolist() == [[1, 1], [2, 2]] and simplify_line(np.array([[1, 1]]), 5).tolist() == [[1, 1]]


# ---- features ------------------------------------------------------------------------------------------------------------------
def test_vertices_are_pixel_centres_and_agree_across_a_seam():
    z, size = 18, 64
    left, right = Tile(69623, 104945, z), Tile(69624, 104945, z)
    m = np.zeros((size, size), bool)
    m[10, 5:60] = True
    rows = _rows(m)
    table = R.table(R.label(m))
    feats = centerlines(rows, table, [left], (size, size), prune=0, tolerance=0)
    assert len(feats) == 1 and feats[0]["geometry"]["type"] == "LineString"
    assert feats[0]["geometry"]["coordinates"] == [list(pixel_to_location(left, 5.5 / size, 10.5 / size)), list(pixel_to_location(left, 59.5 / size, 10.5 / size))]
    assert feats[0]["properties"] == {"tile": [69623, 104945, z], "component": 10 * size + 5 + 1, "length_px": 54.0, "area_px": 55}
    # a line through the seam of two tiles: the stitched feature's vertices are the floats either tile gives its own pixels
    wide = np.zeros((size, 2 * size), bool)
    wide[10, 40:100] = True
    links = T.links(wide, R.label(wide))[:, 1:]
    label = 10 * size + 40 + 1  # (canonical pixel in slot 0: the global index is the tile's own)
    links[:, 0] = label
    stitched = centerlines_stitched(links, np.array([[label, 60, 40, 10, 99, 10]]), [left, right], (size, size), prune=0, tolerance=0)
    assert len(stitched) == 1 and stitched[0]["properties"]["stitched"] is True and stitched[0]["properties"]["tile"] == [69623, 104945, z]
    first, last = stitched[0]["geometry"]["coordinates"]
    assert first == list(pixel_to_location(left, 40.5 / size, 10.5 / size)) and last == list(pixel_to_location(right, 35.5 / size, 10.5 / size))
    # the two pixels either side of the seam are one pixel apart on the map, whichever tile locates them
    a = mosaic_centre_location(z, left.x * size + size - 1, left.y * size + 10, (size, size))
    b = mosaic_centre_location(z, left.x * size + size, left.y * size + 10, (size, size))
    assert a == pixel_to_location(left, (size - 0.5) / size, 10.5 / size) and b == pixel_to_location(right, 0.5 / size, 10.5 / size)
    pixel = 360.0 / 2 ** z / size
    assert b[0] - a[0] == pytest.approx(pixel, rel=1e-6) and a[1] == pytest.approx(b[1], abs=1e-12)
    # a skeleton of one pixel is still a feature
    dot = np.zeros((size, size), bool)
    dot[7, 9] = True
    lone = centerlines(_rows(dot), R.table(R.label(dot)), [left], (size, size))
    assert len(lone) == 1 and len(lone[0]["geometry"]["coordinates"]) == 2 and lone[0]["properties"]["length_px"] == 0
