"""Host half of ``rs features --stitch`` (robosat_amd/features.py) without a GPU: tile clusters and their slot / neighbour /
origin tables, packing of clusters into device calls, ring linking in mosaic coordinates, seam-consistent georeferencing, the
flag, and the new entry points' declarations."""

import argparse
import io
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import features as F  # noqa: E402
from robosat_amd.tiles import Tile  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rs_features_halo", "rs_features_stitch_labels", "rs_features_components_stitched", "rs_features_edges_stitched"]


def test_clusters_are_8_connected_per_zoom():
    tiles = [Tile(5, 5, 18), Tile(6, 6, 18),  # touch only at a corner: one cluster (the halo crosses diagonals)
             Tile(9, 5, 18),  # two columns away: its own
             Tile(5, 5, 17), Tile(5, 6, 17),  # the same x / y at another zoom never join zoom 18
             Tile(20, 20, 18), Tile(21, 20, 18), Tile(22, 20, 18), Tile(20, 21, 18), Tile(22, 21, 18), Tile(20, 22, 18), Tile(21, 22, 18),
             Tile(22, 22, 18)]  # a ring round a hole
    got = F.group_clusters(reversed(tiles))
    assert got == [[Tile(5, 5, 17), Tile(5, 6, 17)], [Tile(5, 5, 18), Tile(6, 6, 18)], [Tile(9, 5, 18)],
                   [Tile(20, 20, 18), Tile(20, 21, 18), Tile(20, 22, 18), Tile(21, 20, 18), Tile(21, 22, 18), Tile(22, 20, 18),
                    Tile(22, 21, 18), Tile(22, 22, 18)]]


def test_tables_of_a_grid_with_a_hole_and_a_diagonal():
    ring = F.group_clusters([Tile(20 + x, 20 + y, 18) for x in range(3) for y in range(3) if (x, y) != (1, 1)])[0]
    nbr, origin, corner = F.stitch_tables(ring, (16, 24))
    assert corner == (20, 20) and nbr.dtype == np.int32 and origin.dtype == np.int32
    # slots (x-major): 0 (20,20) 1 (20,21) 2 (20,22) 3 (21,20) 4 (21,22) 5 (22,20) 6 (22,21) 7 (22,22); order NW N NE W E SW S SE
    assert nbr.tolist() == [[-1, -1, -1, -1, 3, -1, 1, -1], [-1, 0, 3, -1, -1, -1, 2, 4], [-1, 1, -1, -1, 4, -1, -1, -1],
                            [-1, -1, -1, 0, 5, 1, -1, 6], [1, -1, 6, 2, 7, -1, -1, -1], [-1, -1, -1, 3, -1, -1, 6, -1],
                            [3, 5, -1, -1, -1, 4, 7, -1], [-1, 6, -1, 4, -1, -1, -1, -1]]
    assert origin.tolist() == [[0, 0], [0, 16], [0, 32], [24, 0], [24, 32], [48, 0], [48, 16], [48, 32]]  # (X, Y): W = 24, H = 16
    nbr, origin, corner = F.stitch_tables([Tile(5, 6, 18), Tile(6, 5, 18)], (8, 8))  # diagonal only: NE of the first, SW of the second
    assert nbr.tolist() == [[-1, -1, 1, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, 0, -1, -1]] and origin.tolist() == [[0, 8], [8, 0]]
    assert corner == (5, 5)
    g = S.Grid({(t.x, t.y): np.zeros((16, 24)) for t in ring}, 0)  # the tests' own tables agree
    assert (g.tables()[0] == F.stitch_tables(ring, (16, 24))[0]).all() and (g.tables()[1] == F.stitch_tables(ring, (16, 24))[1]).all()


def test_clusters_are_packed_whole_under_the_call_limit():
    clusters = F.group_clusters([Tile(10 * c + i, 0, 18) for c, n in enumerate([3, 2, 4, 1]) for i in range(n)])
    assert [len(c) for c in clusters] == [3, 2, 4, 1]
    calls = F.pack_clusters(clusters, 100, limit=500)
    assert [len(c) for c in calls] == [5, 5]  # 3 + 2, then 4 + 1: never a part of a cluster
    assert all(call == sorted(call, key=lambda t: (t.z, t.x, t.y)) for call in calls)
    assert [len(c) for c in F.pack_clusters(clusters, 100, limit=400)] == [3, 2, 4, 1]
    assert [len(c) for c in F.pack_clusters(clusters, 100, limit=1000)] == [10]
    assert [len(c) for c in F.pack_clusters(clusters, 100, limit=1000, max_tiles=6)] == [5, 5]
    with pytest.raises(ValueError, match="cannot be split"):
        F.pack_clusters(clusters, 100, limit=399)
    # the default limit is the library's: 2^29 - 1 pixels
    assert len(F.pack_clusters(clusters, 512 * 512)) == 1 and F.CALL_PIXELS == (1 << 29) - 1
    # far apart in x: the mosaic coordinates of one call must stay below 2^31
    far = F.group_clusters([Tile(0, 0, 22), Tile((1 << 22) - 1, 0, 22)])
    assert [len(c) for c in F.pack_clusters(far, 512 * 512, side=512)] == [1, 1]
    with pytest.raises(AssertionError):
        F.stitch_tables([Tile(0, 0, 22), Tile((1 << 22) - 1, 0, 22)], (512, 512))


def _shifted(rings, dx, dy):
    return [r + np.array([dx, dy]) for r in rings]


@pytest.mark.parametrize("name", ["nested", "self_touching", "corner_touch"])
def test_mosaic_linking_equals_the_tile_linking_far_from_the_origin(name):
    labels = R.label(getattr(R, name)())
    rows = R.edges(labels).astype(np.int64)
    want = F.link_rings(rows)
    for dx, dy, dl in ((0, 0, 0), (5000, 70000, (1 << 24) + 5), ((1 << 31) - 100, 1 << 30, (1 << 29) - int(labels.max()))):
        moved = np.stack([rows[:, 1] + dl, rows[:, 2] + dx, rows[:, 3] + dy, rows[:, 4]], axis=1)
        got = F.link_rings_mosaic(moved[::-1])
        assert sorted(got) == sorted(label + dl for _, label in want)
        for (_, label), rings in want.items():
            assert len(got[label + dl]) == len(rings)
            for a, b in zip(got[label + dl], _shifted(rings, dx, dy)):
                assert a.dtype == np.int64 and (a == b).all()


def test_mosaic_linking_takes_components_up_to_65536_a_side_and_refuses_more():
    def frame(side):  # the boundary of a side x side square: 4 * side edges, no pixels needed
        k = np.arange(side)
        z, s = np.zeros(side, dtype=np.int64), np.full(side, side - 1)
        return np.concatenate([np.stack([z + 7, k, z, z], 1), np.stack([z + 7, s, k, z + 1], 1), np.stack([z + 7, k, s, z + 2], 1),
                               np.stack([z + 7, z, k, z + 3], 1)])

    rings = F.link_rings_mosaic(frame(1 << 16))
    assert list(rings) == [7] and len(rings[7]) == 1 and F.signed_area(rings[7][0]) == (1 << 16) ** 2
    with pytest.raises(ValueError, match="2\\^16"):
        F.link_rings_mosaic(frame((1 << 16) + 1))
    assert F.link_rings_mosaic(np.zeros((0, 4))) == {}


def test_featurize_stitched_maps_back_to_the_raster():
    """The host half alone, on the restated edges of a raster cut into 3 x 2 tiles: properties, order, and the rings filled
    even-odd give the components back."""

    image = R.blobs(32, 48, 3, 7)
    g = S.Grid(S.split(image, 16, 16, x0=100, y0=200), 2)
    labels = g.global_labels(g.canvas)
    tiles = [Tile(x, y, 18) for x, y in g.coords]
    feats = F.featurize_stitched(g.edges(labels), g.table(labels), tiles, (16, 16), simplify=0, georeference=False)
    want = g.table(labels)
    assert [f["properties"]["area_px"] for f in feats] == want[:, 1].tolist()
    rebuilt = np.zeros(image.shape, dtype=bool)
    for f, row in zip(feats, want):
        assert f["properties"]["stitched"] is True
        assert f["properties"]["tile"] == list(tiles[(row[0] - 1) // 256])
        inside = R.fill_even_odd([np.array(r[:-1]) for r in f["geometry"]["coordinates"]], *image.shape)
        assert inside.sum() == row[1] and not (inside & rebuilt).any()
        rebuilt |= inside
    assert (rebuilt == image).all()
    geo = F.featurize_stitched(g.edges(labels), g.table(labels), tiles, (16, 16), simplify=0)
    assert len(geo) == len(feats) and all(-180 <= lon <= 180 for f in geo for r in f["geometry"]["coordinates"] for lon, _ in r)


def test_a_seam_vertex_has_one_location_whichever_tile_it_is_taken_from():
    shape = (48, 80)
    for z, x, y in ((18, 69623, 104945), (18, 69624, 104946), (3, 2, 5), (1, 0, 0), (22, 12345, 4000001 % (1 << 22))):
        for p in (0, 1, 17, 47):
            east = F.tile_vertex_location(Tile(x, y, z), 80, p, shape)
            west = F.tile_vertex_location(Tile(x + 1, y, z), 0, p, shape)
            assert east == west == F.mosaic_location(z, (x + 1) * 80, y * 48 + p, shape)
            south = F.tile_vertex_location(Tile(x, y, z), p, 48, shape)
            north = F.tile_vertex_location(Tile(x, y + 1, z), p, 0, shape)
            assert south == north == F.mosaic_location(z, x * 80 + p, (y + 1) * 48, shape)
        corner = {F.tile_vertex_location(Tile(x + i, y + j, z), 80 * (1 - i), 48 * (1 - j), shape) for i in (0, 1) for j in (0, 1)}
        assert len(corner) == 1
    # inside a tile it is the per-tile path's own formula
    from robosat_amd.tiles import pixel_to_location

    assert F.mosaic_location(18, 69623 * 80 + 13, 104945 * 48 + 7, shape) == pixel_to_location(Tile(69623, 104945, 18), 13 / 80, 7 / 48)
    # the last column / row of the world has no tile to its east / south
    assert F.mosaic_location(1, 2 * 80, 2 * 48, shape) == F.tile_vertex_location(Tile(1, 1, 1), 80, 48, shape)


def test_the_stitch_flag_parses_and_defaults_off():
    from robosat_amd.tools import features as tool

    parser = argparse.ArgumentParser()
    tool.add_parser(parser.add_subparsers())
    base = ["features", "masks", "--type", "parking", "--dataset", "d.toml", "out.geojson"]
    assert parser.parse_args(base).stitch is False
    assert parser.parse_args(base + ["--stitch"]).stitch is True


def test_the_new_entry_points_are_declared_additively():
    from robosat_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(", header), name
    assert _lib.ABI_VERSION == 24
    assert ops.halo_apron(20, 20) == 40 and ops.halo_apron(1, 3) == 3 and ops.halo_apron(0, 1) == 0
    for name in ("gather_halo", "crop_halo", "stitch_labels", "component_table_stitched", "boundary_edges_stitched", "stitched_features"):
        assert callable(getattr(ops, name))


def test_warnings_go_where_the_caller_says():
    """A sliver that simplification flattens is skipped with the per-tile path's warning."""

    rows = np.array([[1, x, 0, d] for x in range(40) for d in (0, 2)] + [[1, 39, 0, 1], [1, 0, 0, 3]])
    out = io.StringIO()
    feats = F.featurize_stitched(rows, np.array([[1, 40, 0, 0, 39, 0]]), [Tile(0, 0, 1)], (64, 64), simplify=0.2, warn=out)
    assert feats == [] and "Warning" in out.getvalue()
