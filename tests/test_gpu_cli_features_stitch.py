"""``./rs features --stitch`` end to end on the MI355X: a synthetic slippy-map directory of 3 x 3 tiles with one missing -> GeoJSON
-> back to pixels, against the CPU restatement (tests/features_ref.py) applied to the one raster the tiles form."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import png  # noqa: E402
from robosat_amd.colors import make_palette  # noqa: E402
from robosat_amd.tiles import Tile, tile_bounds  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["background", "parking", "building"]
DENOISE, GROW, MIN_AREA = 5, 4, 30
Z, X0, Y0, SIZE = 18, 69623, 104945, 64


def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _write(root, tiles, palette):
    for (x, y), image in tiles.items():
        os.makedirs(os.path.join(root, str(Z), str(x)), exist_ok=True)
        png.write_png(os.path.join(root, str(Z), str(x), str(y) + ".png"), image, "P", palette)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("features_stitch")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking", "building"]\ncolors = ["denim", "orange", "green"]\n')
    palette = make_palette("denim", "orange", "green")
    side = 3 * SIZE
    image = np.where(R.blobs(side, side, 31, 16), 2, 0).astype(np.uint8)
    image[R.blobs(side, side, 32, 4)] = 1  # the other foreground class, over it
    image[70:120, 40:150][:, :] = 2
    image[85:105, 60:130] = 0  # a polygon with a hole, across two seams
    image[118:138, 118:138] = 0
    image[123:133, 123:133] = 2  # 25 pixels in each of four tiles: above MIN_AREA only as a whole
    tiles = S.split(image, SIZE, SIZE, absent={(2, 0)}, x0=X0, y0=Y0)
    _write(str(tmp / "masks"), tiles, palette)
    grid = S.Grid(tiles, S.margin(DENOISE, GROW))
    cleaned = R.clean(grid.canvas, CLASSES.index("building"), DENOISE, GROW) * (grid.index >= 0)  # no tile, no pixel
    reference = R.filter_labels(grid.global_labels(cleaned), MIN_AREA)
    return {"tmp": tmp, "dataset": str(dataset), "masks": str(tmp / "masks"), "grid": grid, "reference": reference, "palette": palette}


def _run(s, name, extra):
    out = str(s["tmp"] / name)
    done = _rs(["features", s["masks"], "--type", "building", "--dataset", s["dataset"], out, "--denoise", str(DENOISE), "--grow", str(GROW),
                "--min_area", str(MIN_AREA)] + extra)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(out, "rb") as fp:
        return fp.read()


def _to_canvas(grid, ring):
    """lon / lat vertices -> canvas pixel corners: longitude is linear over the whole zoom level, latitude inside a tile row."""

    out = []
    for lon, lat in ring:
        gx = (lon + 180.0) / 360.0 * 2 ** Z * SIZE
        for ty in range(grid.y_min, grid.y_min + grid.ny):
            _, south, _, north = tile_bounds(Tile(grid.x_min, ty, Z))
            if south <= lat <= north:
                gy = (ty + (lat - north) / (south - north)) * SIZE
                break
        else:
            raise AssertionError("latitude {} outside the tile rows".format(lat))
        out.append([gx - grid.x_min * SIZE + grid.pad, gy - grid.y_min * SIZE + grid.pad])
    px = np.array(out)
    assert np.abs(px - np.rint(px)).max() < 1e-3, "vertices are pixel corners"
    return np.rint(px)


def test_stitched_polygons_map_back_to_the_restated_raster(setup):
    grid, reference = setup["grid"], setup["reference"]
    doc = json.loads(_run(setup, "exact.geojson", ["--stitch", "--simplify", "0"]))
    assert doc["type"] == "FeatureCollection"
    keys = [(f["properties"]["tile"][2], f["properties"]["tile"][0], f["properties"]["tile"][1]) for f in doc["features"]]
    assert keys == sorted(keys)
    want_labels = np.unique(reference[reference != 0])
    assert len(doc["features"]) == len(want_labels)
    hw = SIZE * SIZE
    assert [f["properties"]["tile"] for f in doc["features"]] == [list(grid.coords[(l - 1) // hw]) + [Z] for l in want_labels.tolist()]
    rebuilt = np.zeros(reference.shape, dtype=bool)
    for f, label in zip(doc["features"], want_labels):
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon" and f["properties"]["stitched"] is True
        rings = [_to_canvas(grid, ring[:-1]) for ring in f["geometry"]["coordinates"]]
        assert all(ring[0] == ring[-1] and len(ring) >= 5 for ring in f["geometry"]["coordinates"])
        inside = R.fill_even_odd(rings, *reference.shape)
        assert inside.sum() == f["properties"]["area_px"] == (reference == label).sum() and not (rebuilt & inside).any()
        assert (inside == (reference == label)).all()
        rebuilt |= inside
        ring = np.array(f["geometry"]["coordinates"][0][:-1])  # RFC 7946: the outer ring counter-clockwise in lon / lat
        assert np.sum(ring[:, 0] * np.roll(ring[:, 1], -1) - np.roll(ring[:, 0], -1) * ring[:, 1]) > 0
    assert (rebuilt == (reference != 0)).all()
    assert any(len(f["geometry"]["coordinates"]) > 1 for f in doc["features"]), "no feature with a hole"
    # one of them is kept only because --min_area sees the whole component: every part of it inside one tile is below the threshold
    parts = [max(int((grid.cut(reference)[slot] == label).sum()) for slot in range(len(grid.coords))) for label in want_labels]
    assert min(parts) < MIN_AREA

    per_tile = json.loads(_run(setup, "per_tile.geojson", ["--simplify", "0"]))
    assert len(doc["features"]) < len(per_tile["features"])
    assert all("stitched" not in f["properties"] for f in per_tile["features"])


def test_defaults_simplify_to_valid_rings_and_repeat_byte_for_byte(setup):
    first = _run(setup, "default.geojson", ["--stitch"])
    assert first == _run(setup, "default_again.geojson", ["--stitch"])
    doc = json.loads(first)
    assert 0 < len(doc["features"]) <= len(np.unique(setup["reference"])) - 1
    for f in doc["features"]:
        for ring in f["geometry"]["coordinates"]:
            assert len(ring) >= 4 and ring[0] == ring[-1]


def test_mixed_shapes_and_oversized_discs_are_error_messages(setup):
    out = str(setup["tmp"] / "bad.geojson")
    done = _rs(["features", setup["masks"], "--type", "building", "--dataset", setup["dataset"], out, "--stitch", "--denoise", "40", "--grow", "40"])
    assert done.returncode != 0 and "Error" in done.stderr and "Traceback" not in done.stderr and not os.path.exists(out)
    mixed = str(setup["tmp"] / "mixed")
    _write(mixed, {(X0, Y0): np.zeros((64, 64), np.uint8), (X0 + 1, Y0): np.zeros((32, 64), np.uint8)}, setup["palette"])
    done = _rs(["features", mixed, "--type", "building", "--dataset", setup["dataset"], out, "--stitch"])
    assert done.returncode != 0 and "Error" in done.stderr and "Traceback" not in done.stderr and not os.path.exists(out)
