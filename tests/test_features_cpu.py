"""``rs features`` without a GPU: the stage definitions' restatements (tests/features_ref.py) pinned against scipy.ndimage, and the host
half -- ring linking, simplification, validity, georeferencing, GeoJSON output -- on restated edges.  Everything is integer- or
byte-exact; there is no tolerance anywhere."""

import io
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402

from robosat_amd import features as F  # noqa: E402
from robosat_amd import ops  # noqa: E402
from robosat_amd.tiles import Tile, pixel_to_location, tile_bounds  # noqa: E402

DISC_WIDTHS = {
    1: [1],
    2: [1, 2],
    3: [1, 3, 1],
    4: [1, 4, 4, 4],
    5: [1, 5, 5, 5, 1],
    20: [1, 9, 13, 15, 17, 19, 19, 20, 20, 20, 20, 20, 20, 20, 19, 19, 17, 15, 13, 9],
}


def _masks():
    out = {"corner_touch": R.corner_touch(), "nested": R.nested(), "self_touching": R.self_touching(), "checkerboard": R.checkerboard(9, 10),
           "spiral": R.spiral(17), "comb": R.comb(12), "full": np.ones((5, 7), dtype=bool), "single": np.ones((1, 1), dtype=bool),
           "border": R.border(11, 13)}
    for seed in range(12):
        out["noise{}".format(seed)] = R.noise(48, 48, seed, (0.3, 0.5, 0.7)[seed % 3])
        out["opened{}".format(seed)] = R.opening(R.noise(48, 48, 100 + seed, 0.8), 3 + seed % 3)
    return out


MASKS = _masks()


@pytest.mark.parametrize("eps", sorted(DISC_WIDTHS))
def test_disc_rows_are_the_documented_ellipse(eps):
    c = eps // 2
    widths = [min(c + dx + 1, eps) - max(c - dx, 0) for dx in ops.disc_rows(eps)]
    assert widths == DISC_WIDTHS[eps]
    assert R.disc(eps).sum(axis=1).tolist() == DISC_WIDTHS[eps]
    for i, dx in enumerate(ops.disc_rows(eps)):  # the rows sit where the definition puts them
        assert R.disc(eps)[i].tolist() == [int(max(c - dx, 0) <= j < min(c + dx + 1, eps)) for j in range(eps)]
    assert R.disc(20).sum() == 325
    assert ops.disc_rows(0) == []


@pytest.mark.parametrize("eps", [2, 3, 4, 5, 20, 21])
def test_open_close_identities(eps):
    for seed, density in enumerate((0.3, 0.6, 0.9)):
        m = R.noise(70, 90, seed, density) | R.blobs(70, 90, seed)
        o, c = R.opening(m, eps), R.closing(m, eps)
        assert (o <= m).all() and (m <= c).all()
        assert (R.opening(o, eps) == o).all() and (R.closing(c, eps) == c).all()
    m = R.noise(9, 9, 0, 0.5)
    assert (R.opening(m, 0) == m).all() and (R.closing(m, 1) == m).all()


def test_restatements_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for eps in (3, 5, 21):
        m = R.noise(60, 75, eps, 0.7)
        k = R.disc(eps).astype(bool)
        assert (R.erode(m, eps) == ndimage.binary_erosion(m, k, border_value=1)).all()
        assert (R.dilate(m, eps) == ndimage.binary_dilation(m, k)).all()
    for name, m in MASKS.items():
        assert (R.label(m) == R.canonical(ndimage.label(m)[0])).all(), name  # (the default structure is 4-connectivity)


def test_label_restatement_is_canonical():
    lab = R.label(R.corner_touch())
    assert lab[1, 1] == 1 + 1 * 9 + 1 and lab[4, 4] == 1 + 4 * 9 + 4 and lab[0, 8] == 9 and lab[1, 7] == 1 + 9 + 7
    assert len(np.unique(R.label(R.checkerboard(9, 10)))) - 1 == 45
    assert len(np.unique(R.label(R.spiral(17)))) == 2 and len(np.unique(R.label(R.comb(12)))) == 2


@pytest.mark.parametrize("name", sorted(MASKS))
def test_link_rings_invariants(name):
    labels = R.label(MASKS[name])
    h, w = labels.shape
    edges = R.edges(labels)
    rings = F.link_rings(edges)
    areas = {int(r[1]): int(r[2]) for r in R.table(labels)}
    assert sorted(label for _, label in rings) == sorted(areas)
    rebuilt = np.zeros_like(labels)
    for (tile, label), group in rings.items():
        assert tile == 0
        signed = [F.signed_area(r) for r in group]
        assert signed[0] > 0 and all(a < 0 for a in signed[1:]), "exactly one ring of positive area, first"
        assert sum(signed) == areas[label]
        for ring in group:
            assert len({(int(x), int(y)) for x, y in ring}) == len(ring), "a ring touches itself"
            steps = np.abs(np.roll(ring, -1, axis=0) - ring).sum(axis=1)
            assert (steps == 1).all()
            assert tuple(ring[0]) == min(map(tuple, ring.tolist()))
        inside = R.fill_even_odd(group, h, w)
        assert not (rebuilt[inside] != 0).any()
        rebuilt[inside] = label
    assert (rebuilt == labels).all(), "even-odd fill of every component's rings is the label image"


def test_link_rings_does_not_depend_on_the_edge_order():
    edges = R.edges(R.label(MASKS["self_touching"] ))
    want = F.link_rings(edges)
    got = F.link_rings(edges[np.random.RandomState(0).permutation(len(edges))])
    assert want.keys() == got.keys()
    for k in want:
        assert len(want[k]) == len(got[k]) and all((a == b).all() for a, b in zip(want[k], got[k]))


def test_the_other_turn_makes_rings_touch_themselves():
    """Why the left turn: linked with the right turn first (round the pixel the walk is on), a component that meets itself at a corner
    gives rings that pass through that corner twice; the areas still sum to the pixel count.  With the left turn no ring does."""
    labels = R.label(R.self_touching())
    edges = R.edges(labels)

    def repeated(rings):
        return sum(len(r) - len({(int(x), int(y)) for x, y in r}) for group in rings.values() for r in group)

    right = F.link_rings(edges, turns=(1, 0, 3))
    assert repeated(right) > 0
    assert sum(F.signed_area(r) for group in right.values() for r in group) == (labels != 0).sum()
    assert repeated(F.link_rings(edges)) == 0


def test_simplify_zero_rasterises_back_exactly():
    for name, m in MASKS.items():
        labels = R.label(m)
        h, w = labels.shape
        for (_, label), group in F.link_rings(R.edges(labels)).items():
            simple = [F.simplify_ring(r, 0) for r in group]
            for r in simple:
                a, b = r - np.roll(r, 1, axis=0), np.roll(r, -1, axis=0) - r
                assert (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] != 0).all(), "a collinear vertex is left"
            assert (R.fill_even_odd(simple, h, w) == (labels == label)).all(), name


def test_simplification_is_independent_of_the_starting_vertex():
    labels = R.label(R.blobs(96, 96, 3) & ~R.noise(96, 96, 3, 0.01))
    for group in F.link_rings(R.edges(labels)).values():
        for ring in group:
            want = F.simplify_ring(ring, 0.01)
            for shift in (1, len(ring) // 3, len(ring) - 1):
                got = F.simplify_ring(np.roll(ring, shift, axis=0), 0.01)
                assert got.shape == want.shape and (got == want).all()
            assert len(want) <= len(F.simplify_ring(ring, 0))


def test_simplify_drops_rings_below_three_vertices():
    square = np.array([[0, 0], [1, 0], [1, 1], [0, 1]])
    assert len(F.simplify_ring(square, 0)) == 4
    assert len(F.simplify_ring(square, 10.0)) < 3


def test_polygon_is_valid_rejects_a_self_crossing_ring():
    assert F.polygon_is_valid([np.array([[0, 0], [4, 0], [4, 4], [0, 4]])])
    assert not F.polygon_is_valid([np.array([[0, 0], [4, 4], [4, 0], [0, 4]])])  # a bow tie
    assert F.polygon_is_valid([np.array([[0, 0], [9, 0], [9, 9], [0, 9]]), np.array([[2, 2], [2, 5], [5, 5], [5, 2]])])
    assert not F.polygon_is_valid([np.array([[0, 0], [9, 0], [9, 9], [0, 9]]), np.array([[2, 2], [2, 12], [5, 12], [5, 2]])])  # hole leaves
    assert F.polygon_is_valid([np.array([[0, 0], [4, 0], [4, 4], [2, 0], [0, 4]])])  # touching at a vertex is not a proper crossing


def test_tile_bounds_closed_form():
    west, south, east, north = tile_bounds(Tile(0, 0, 0))
    assert (west, east) == (-180.0, 180.0)
    assert north == -south == math.degrees(math.atan(math.sinh(math.pi)))
    assert abs(north - 85.0511287798066) < 1e-12
    for x, y, z in ((69623, 104945, 18), (0, 0, 18), (2 ** 18 - 1, 2 ** 18 - 1, 18), (5, 9, 4)):
        n = 2.0 ** z
        want = (x / n * 360.0 - 180.0, math.degrees(math.atan(math.sinh(math.pi * (1.0 - 2.0 * (y + 1) / n)))),
                (x + 1) / n * 360.0 - 180.0, math.degrees(math.atan(math.sinh(math.pi * (1.0 - 2.0 * y / n)))))
        assert tile_bounds(Tile(x, y, z)) == want
        west, south, east, north = want
        assert pixel_to_location(Tile(x, y, z), 0.0, 0.0) == (west, north)
        assert pixel_to_location(Tile(x, y, z), 1.0, 1.0) == (west + (east - west), north + (south - north))
        assert pixel_to_location(Tile(x, y, z), 0.25, 0.5) == (west + 0.25 * (east - west), north + 0.5 * (south - north))


def _features(mask, tile, simplify, min_area=0):
    labels = R.filter_labels(R.label(mask), min_area)
    warn = io.StringIO()
    return F.featurize(R.edges(labels), R.table(labels), [tile], labels.shape, simplify, warn=warn), warn.getvalue()


def _ring_area(ring):
    ring = np.asarray(ring[:-1])
    return float(np.sum(ring[:, 0] * np.roll(ring[:, 1], -1) - np.roll(ring[:, 0], -1) * ring[:, 1]) / 2)


def test_features_follow_rfc7946_and_map_back_to_pixels(tmp_path):
    tile = Tile(69623, 104945, 18)
    mask = R.nested()
    h, w = mask.shape
    features, _ = _features(mask, tile, 0)
    assert len(features) == 3  # outer ring with its hole, inner ring with its hole, the island
    west, south, east, north = tile_bounds(tile)
    labels = R.label(mask)
    rebuilt = np.zeros_like(labels)
    for f in features:
        coords = f["geometry"]["coordinates"]
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon" and f["properties"]["tile"] == [69623, 104945, 18]
        assert _ring_area(coords[0]) > 0 and all(_ring_area(r) < 0 for r in coords[1:]), "outer counter-clockwise, holes clockwise"
        pixel_rings = []
        for ring in coords:
            assert ring[0] == ring[-1] and len(ring) >= 4
            px = np.array([[(lon - west) / (east - west) * w, (lat - north) / (south - north) * h] for lon, lat in ring[:-1]])
            assert np.abs(px - np.rint(px)).max() < 1e-6
            pixel_rings.append(np.rint(px))
        inside = R.fill_even_odd(pixel_rings, h, w)
        assert f["properties"]["area_px"] == inside.sum()
        rebuilt[inside] = labels[inside].max()
    assert (rebuilt == labels).all()

    writer = F.FeatureWriter()
    writer.add(features)  # (a tile's features arrive in label order, the tiles in any order)
    writer.add(_features(R.corner_touch(), Tile(1, 2, 3), 0)[0])
    writer.save(str(tmp_path / "a.geojson"))
    again = F.FeatureWriter()
    again.add(_features(R.corner_touch(), Tile(1, 2, 3), 0)[0])
    again.add(features)
    again.save(str(tmp_path / "b.geojson"))
    a, b = (tmp_path / "a.geojson").read_bytes(), (tmp_path / "b.geojson").read_bytes()
    assert a == b
    doc = json.loads(a)
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == 7
    keys = [(f["properties"]["tile"][2], f["properties"]["tile"][0], f["properties"]["tile"][1]) for f in doc["features"]]
    assert keys == sorted(keys)
    assert all(set(f) == {"type", "geometry", "properties"} and set(f["properties"]) == {"tile", "area_px"} for f in doc["features"])
    in_tile = [f["properties"]["area_px"] for f in doc["features"] if f["properties"]["tile"] == [1, 2, 3]]
    assert in_tile == R.table(R.label(R.corner_touch()))[:, 2].tolist(), "label order inside a tile"
    assert repr(doc["features"][0]["geometry"]["coordinates"][0][0][0]).encode() in a  # floats printed by repr


def test_featurize_warns_and_drops_what_simplification_destroys():
    features, warnings = _features(np.ones((1, 1), dtype=bool), Tile(0, 0, 1), 10.0)
    assert features == [] and "no longer valid polygon" in warnings
    features, _ = _features(R.corner_touch(), Tile(0, 0, 1), 0, min_area=2)
    assert sorted(f["properties"]["area_px"] for f in features) == [9, 12]


def test_header_lists_the_feature_entry_points():
    from robosat_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "robosat_hip.h")).read()
    for name in ("rs_features_clean_form", "rs_features_clean_workspace_bytes", "rs_features_clean", "rs_features_label",
                 "rs_features_components", "rs_features_edges"):
        assert name in _lib.SIGNATURES and name + "(" in header
    assert _lib.ABI_VERSION == 24
