"""``ops.centerline_counts`` (rs_eval_centerline) on the MI355X against the numpy restatement of tests/centerline_eval_ref.py: exact
integer equality, per tile and stitched, at the edges of the link rule and of the reach, with ``ops.skeleton_links`` as a second
witness for the totals."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import centerline_eval_ref as C  # noqa: E402
import stitch_ref as S  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

# (40, 8, 8): many tiles per workgroup; the others hold workgroups that straddle tiles; W = 1, H = 1, W no multiple of 16 or 64
SHAPES = [(1, 1, 1), (1, 1, 7), (1, 5, 1), (3, 17, 33), (2, 64, 64), (5, 67, 130), (40, 8, 8)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _shift(m, dy, dx):
    """``m`` moved by (dy, dx) >= 0, zeros coming in."""

    out = np.zeros_like(m)
    h, w = m.shape
    out[dy:, dx:] = m[:h - dy, :w - dx]
    return out


def pair(b, h, w, kind):
    """(skel_p, skel_g) uint8 [B, H, W], both non-empty.  ``roads``: thinned narrow roads, the prediction the label moved by (1, 2)
    with one road more; ``noise``: hand-made 0/1 rasters (the op takes any), dense enough for every kind of link."""

    if h * w < 8:
        p = np.ones((b, h, w), dtype=np.uint8)
        g = np.ones((b, h, w), dtype=np.uint8)
        p.reshape(b, -1)[:, 3::4] = 0
        g.reshape(b, -1)[:, 1::3] = 0
        return p, g
    ps, gs = [], []
    for i in range(b):
        if kind == "roads":
            g = T.roads(h, w, 100 + i, count=3, width=3)
            p = _shift(g, min(1, h - 1), min(2, w - 1)) | T.roads(h, w, 200 + i, count=1, width=4)
            ps.append(T.thin(p))
            gs.append(T.thin(g))
        else:
            rng = np.random.RandomState(300 + i)
            ps.append((rng.rand(h, w) < 0.3).astype(np.uint8))
            gs.append((rng.rand(h, w) < 0.15).astype(np.uint8))
    return np.stack(ps), np.stack(gs)


_CACHE = {}


def _case(b, h, w, kind, rho):
    """(skel_p, skel_g, the restatement's [B][8]), computed once and left unchanged."""

    key = (b, h, w, kind, rho)
    if key not in _CACHE:
        p, g = pair(b, h, w, kind)
        assert p.any() and g.any()
        _CACHE[key] = p, g, C.counts_tiles(p, g, rho)
    return _CACHE[key]


def _counts(p, g, rho, nbr=None):
    got = ops.centerline_counts(_dev(p), _dev(g), rho, None if nbr is None else _dev(nbr))
    assert got.dtype == torch.int64 and got.shape == (len(p) if nbr is None else 1, 8)
    return got.cpu().tolist()


@pytest.mark.parametrize("kind", ["roads", "noise"])
@pytest.mark.parametrize("b,h,w", SHAPES)
def test_the_counts_equal_the_restatement_per_tile(b, h, w, kind):
    for rho in (3, 1):
        p, g, want = _case(b, h, w, kind, rho)
        assert _counts(p, g, rho) == want, rho
    if h * w >= 64:
        total = np.array(want).sum(axis=0)
        assert total[0] and total[4], "a side without links: the test shows nothing"
        if kind == "noise":
            assert total[1] and total[5] and 0 < total[2] < total[0] and 0 < total[6] < total[4]


# ---- the link rule at its edges ------------------------------------------------------------------------------------------------
PATTERNS = [
    ([[1, 1, 0], [0, 1, 1], [0, 0, 1]], (4, 0)),  # a staircase: no diagonal where a detour exists
    ([[1, 0, 0], [0, 1, 0], [0, 0, 1]], (0, 2)),  # a pure diagonal
    ([[1, 0, 1], [0, 1, 0], [1, 0, 1]], (0, 4)),  # an X crossing
    ([[0, 0, 0], [0, 1, 0], [0, 0, 0]], (0, 0)),  # a lone pixel has no length
    ([[0, 0, 1], [0, 0, 1], [1, 1, 1]], (4, 0)),  # links in the last row and the last column
    ([[0, 0, 1], [1, 0, 0], [0, 0, 0]], (0, 0)),  # the row's last pixel and the next row's first: it must not wrap
]


def test_the_link_rule_at_its_edges():
    s = np.array([rows for rows, _ in PATTERNS], dtype=np.uint8)
    want = [[a, b, a, b, a, b, a, b] for _, (a, b) in PATTERNS]  # identical sides: every link is matched
    assert _counts(s, s, 1) == want == C.counts_tiles(s, s, 1)
    # the same patterns across the ends of the threads' runs (x = 15 | 16, 31 | 32) and in the last columns of a 35-wide raster
    wide = np.zeros((1, 13, 35), dtype=np.uint8)
    for i, (rows, _) in enumerate(PATTERNS):
        x, y = (14, 30, 15, 31, 32, 9)[i], 1 + (i % 3) * 4
        wide[0, y:y + 3, x:x + 3] |= np.array(rows, dtype=np.uint8)
    wide[0, 12, 30:] = 1
    wide[0, 3:, 34] = 1
    wide[0, 4, 0] = 1  # beside (34, 3): the flat neighbour of the last column is no neighbour
    other = _shift(wide[0], 2, 0)[None]
    assert _counts(wide, other, 1) == C.counts_tiles(wide, other, 1)


# ---- the reach at its edges ----------------------------------------------------------------------------------------------------
def test_the_reach_at_its_edges():
    p = np.zeros((4, 16, 40), dtype=np.uint8)
    g = np.zeros((4, 16, 40), dtype=np.uint8)
    p[:, 6, 10:12] = 1             # one E link (10, 6) - (11, 6) in every tile
    g[0, 10:12, 13] = 1            # (13, 10): offset (3, 4) from the first end, d2 = 25, and 20 from the second: matched
    g[1, 7, 15] = 1                # (15, 7): offset (5, 1) from the first end, d2 = 26, but 17 from the second: one end only
    g[2, 15, 39] = 1               # far from both
    want = [[1, 0, 1, 0, 1, 0, 0, 0],  # (the label's S link (13, 10) - (13, 11): its second end is at d2 = 29 of the prediction)
            [1, 0, 0, 0, 0, 0, 0, 0],
            [1, 0, 0, 0, 0, 0, 0, 0],
            [1, 0, 0, 0, 0, 0, 0, 0]]  # the other side empty: nothing matched
    assert C.counts_tiles(p, g, 5) == want
    assert _counts(p, g, 5) == want
    assert _counts(g, p, 5) == [row[4:] + row[:4] for row in want]
    empty = np.zeros_like(p)
    assert _counts(empty, empty, 5) == [[0] * 8] * 4


@pytest.mark.parametrize("rho", [1, 127])
def test_the_smallest_and_the_largest_tolerance(rho):
    p, g = pair(2, 40, 130, "roads")
    want = C.counts_tiles(p, g, rho)
    assert _counts(p, g, rho) == want
    if rho == 127:
        assert want[0][2] == want[0][0] and want[0][6] == want[0][4]  # 40 x 130: everything is within 127 of something


# ---- cross-checks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["roads", "noise"])
def test_the_totals_are_what_skeleton_links_emits(kind):
    p, g = pair(5, 67, 130, kind)
    got = np.array(_counts(p, g, 3))
    for side, column in ((p, 0), (g, 4)):
        skeleton = _dev(side)
        labels = ops.label_components(skeleton)  # (the skeleton as its own mask: every component is listed)
        rows = ops.skeleton_links(skeleton, labels, ops.component_table(labels, 0)).cpu().numpy()
        for tile in range(len(side)):
            dirs = rows[rows[:, 0] == tile][:, 4]
            assert got[tile, column] == np.isin(dirs, (0, 2)).sum() and got[tile, column + 1] == np.isin(dirs, (1, 3)).sum()


def test_identical_sides_are_matched_entirely():
    for kind in ("roads", "noise"):
        p, _ = pair(3, 17, 33, kind)
        got = np.array(_counts(p, p, 1))
        assert (got[:, 0:2] == got[:, 2:4]).all() and (got[:, :4] == got[:, 4:]).all() and got[:, 0].all()


def test_any_non_zero_byte_is_set():
    p, g, want = _case(2, 64, 64, "noise", 3)
    values = np.random.RandomState(1).choice([1, 2, 127, 128, 255], size=p.shape).astype(np.uint8)
    assert _counts(p * values, g * np.uint8(128), 3) == want


# ---- stitched ------------------------------------------------------------------------------------------------------------------
def _grids(image_p, image_g, th, tw, absent=()):
    return (S.Grid(S.split(image_p, th, tw, absent=absent, x0=3, y0=9), 2), S.Grid(S.split(image_g, th, tw, absent=absent, x0=3, y0=9), 2))


def _raster(seed=0):
    g = T.thin(T.roads(96, 128, 40 + seed, count=6, width=5))
    p = T.thin(_shift(T.roads(96, 128, 40 + seed, count=6, width=5), 1, 2) | T.roads(96, 128, 50 + seed, count=2, width=4))
    return p, g


def test_a_grid_of_tiles_counts_what_the_single_raster_does():
    p, g = _raster()
    gp, gg = _grids(p, g, 32, 32)
    assert len(gp.coords) == 12
    for rho in (3, 31):
        want = C.counts(p, g, rho)
        assert C.counts_grid(gp, gg, rho) == want
        assert _counts(gp.stack, gg.stack, rho, gp.tables()[0]) == [want]
        assert _counts(p[None], g[None], rho) == [want]
    per_tile = np.array(_counts(gp.stack, gg.stack, 3)).sum(axis=0)
    assert per_tile.tolist() == np.array(C.counts_tiles(gp.stack, gg.stack, 3)).sum(axis=0).tolist() != C.counts(p, g, 3)


def test_an_absent_tile_reads_zero_and_is_near_nothing():
    p, g = _raster(1)
    # a diagonal line through the corner (64, 32) into the absent tile (column 2, row 1), and a pixel that would be its detour there
    for image in (p, g):
        image[24:40, 56:72] = 0
    p[24:40, 56:72] = np.eye(16, dtype=np.uint8)
    g[24:40, 56:72] = np.eye(16, dtype=np.uint8)[:, ::-1]
    # the label's anti-diagonal has the link (64, 31) -> SW (63, 32) from tile (2, 0) to tile (1, 1); its detour pixel (64, 32) lies in
    # the absent tile: set in the whole raster, where it takes the link away, and gone with the tile
    g[32, 64] = 1
    absent = {(2, 1)}
    gp, gg = _grids(p, g, 32, 32, absent)
    assert len(gp.coords) == 11
    want = C.counts_grid(gp, gg, 4)
    assert _counts(gp.stack, gg.stack, 4, gp.tables()[0]) == [want]
    full = C.counts(p, g, 4)
    assert want != full and want[1] < full[1], "the absent tile changed nothing: the test shows nothing"


def test_a_match_across_a_seam_needs_the_stitched_form():
    p = np.zeros((32, 64), dtype=np.uint8)
    g = np.zeros((32, 64), dtype=np.uint8)
    p[4:28, 30] = 1  # a road down the last but one column of the left tile
    g[4:28, 33] = 1  # its reference three pixels east, in the right tile
    gp, gg = _grids(p, g, 32, 32)
    assert _counts(gp.stack, gg.stack, 3, gp.tables()[0]) == [[23, 0, 23, 0, 23, 0, 23, 0]] == [C.counts_grid(gp, gg, 3)]
    assert _counts(gp.stack, gg.stack, 3) == [[23, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 23, 0, 0, 0]]


# ---- reproducibility -----------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_order_of_the_tiles_has_no_say():
    p, g = _raster(2)
    gp, gg = _grids(p, g, 32, 32, absent={(0, 0)})
    nbr = gp.tables()[0]
    first = _counts(gp.stack, gg.stack, 3, nbr)
    assert first == _counts(gp.stack, gg.stack, 3, nbr) == [C.counts_grid(gp, gg, 3)]
    order = np.random.RandomState(0).permutation(len(nbr))  # new slot i holds old slot order[i]
    new_slot = np.empty(len(nbr), dtype=np.int64)
    new_slot[order] = np.arange(len(nbr))
    moved = np.where(nbr[order] >= 0, new_slot[np.maximum(nbr[order], 0)], -1).astype(np.int32)
    assert _counts(gp.stack[order], gg.stack[order], 3, moved) == first
    pp, gg2 = pair(5, 67, 130, "noise")
    assert _counts(pp, gg2, 3) == _counts(pp, gg2, 3)


def test_bad_arguments_raise():
    p, g = (_dev(a) for a in pair(2, 8, 8, "noise"))
    for rho in (0, 128, -1):
        with pytest.raises(ValueError):
            ops.centerline_counts(p, g, rho)
    with pytest.raises(ValueError):
        ops.centerline_counts(p, g[:1], 3)
    with pytest.raises(ValueError):
        ops.centerline_counts(p[0], g[0], 3)
    with pytest.raises(RuntimeError):
        ops.centerline_counts(p.cpu(), g.cpu(), 3)
    with pytest.raises(TypeError):
        ops.centerline_counts(p.to(torch.int32), g.to(torch.int32), 3)
    nbr = torch.full((2, 8), -1, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError):
        ops.centerline_counts(p, g, 8, nbr)  # (rho + 1 does not fit 8 x 8 stitched tiles: the transform says so)
    with pytest.raises(ValueError):
        ops.centerline_counts(p, g, 3, nbr[:1])
    assert ops.centerline_counts(p, g, 7, nbr).shape == (1, 8)
