"""``./rs features --geometry centerline`` end to end on the MI355X: mask PNGs of one road through three tiles in a row, with a
short side bump, -> GeoJSON LineStrings, with and without ``--stitch``; and ``--geometry polygon`` is the default path."""

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
Z, X0, Y0, SIZE = 18, 69623, 104945, 64
TOP, WIDTH = 26, 12  # the road: rows 26..37 of all three tiles


def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


def road_image():
    image = np.zeros((SIZE, 3 * SIZE), np.uint8)
    image[TOP:TOP + WIDTH, :] = 1
    image[TOP - 8:TOP, 90:96] = 1  # the bump: 6 wide, 8 long, in the middle tile
    return image


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("centerline")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "road"]\ncolors = ["denim", "orange"]\n')
    palette = make_palette("denim", "orange")
    for (x, y), tile in S.split(road_image(), SIZE, SIZE, x0=X0, y0=Y0).items():
        os.makedirs(os.path.join(str(tmp / "masks"), str(Z), str(x)), exist_ok=True)
        png.write_png(os.path.join(str(tmp / "masks"), str(Z), str(x), str(y) + ".png"), tile, "P", palette)
    return {"tmp": tmp, "dataset": str(dataset), "masks": str(tmp / "masks")}


def _run(s, name, extra):
    out = str(s["tmp"] / name)
    done = _rs(["features", s["masks"], "--type", "road", "--dataset", s["dataset"], out, "--denoise", "3", "--grow", "3"] + extra)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(out, "rb") as fp:
        return fp.read()


def _pixels(coordinates):
    """lon / lat -> mosaic pixels (float): longitude is linear over the zoom level, latitude inside the one tile row."""

    _, south, _, north = tile_bounds(Tile(X0, Y0, Z))
    return np.array([[(lon + 180.0) / 360.0 * 2 ** Z * SIZE - X0 * SIZE, (lat - north) / (south - north) * SIZE] for lon, lat in coordinates])


def _check_line(feature, stitched):
    assert feature["type"] == "Feature" and feature["geometry"]["type"] == "LineString"
    props = feature["properties"]
    assert set(props) == {"tile", "component", "length_px", "area_px"} | ({"stitched"} if stitched else set())
    assert props["component"] >= 1 and props["length_px"] > 0 and props["area_px"] > 0
    px = _pixels(feature["geometry"]["coordinates"])
    assert np.abs(px - 0.5 - np.rint(px - 0.5)).max() < 1e-3, "vertices are pixel centres"
    cells = np.rint(px - 0.5).astype(int)
    assert (road_image()[cells[:, 1], cells[:, 0]] == 1).all(), "a vertex outside the road"
    return px


def test_stitched_road_is_one_linestring_through_three_tiles(setup):
    first = _run(setup, "stitched.geojson", ["--geometry", "centerline", "--stitch"])
    doc = json.loads(first)
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == 1, "one road, its spur pruned"
    feature = doc["features"][0]
    px = _check_line(feature, True)
    assert feature["properties"]["stitched"] is True and feature["properties"]["tile"] == [X0, Y0, Z]
    # the component's area is that of the CLEANED mask on the one raster: the discs round the road's free ends and the bump's corners
    grid = S.Grid(S.split(road_image(), SIZE, SIZE, x0=X0, y0=Y0), S.margin(3, 3))
    assert feature["properties"]["area_px"] == int((R.clean(grid.canvas, 1, 3, 3) * (grid.index >= 0)).sum())
    assert px[:, 0].min() < SIZE / 2 and px[:, 0].max() > 2.5 * SIZE, "it spans all three tiles"
    assert feature["properties"]["length_px"] > 2.5 * SIZE
    assert np.abs(px[:, 1] - (TOP + WIDTH / 2)).max() <= 2, "the line stays within two pixels of the road's axis: the bump's branch is gone"
    # with --prune 0 the bump's branch is there
    unpruned = json.loads(_run(setup, "unpruned.geojson", ["--geometry", "centerline", "--stitch", "--prune", "0"]))
    assert len(unpruned["features"]) == 3


def test_per_tile_road_is_three_lines_that_stop_short_of_the_seams(setup):
    doc = json.loads(_run(setup, "per_tile.geojson", ["--geometry", "centerline"]))
    assert len(doc["features"]) == 3
    assert [f["properties"]["tile"] for f in doc["features"]] == [[X0 + i, Y0, Z] for i in range(3)]
    for i, feature in enumerate(doc["features"]):
        px = _check_line(feature, False)
        # about half the road's width short of either border of its own tile
        assert px[:, 0].min() >= i * SIZE + WIDTH / 2 - 2 and px[:, 0].max() <= (i + 1) * SIZE - WIDTH / 2 + 2


@pytest.mark.parametrize("stitch", [[], ["--stitch"]], ids=["per_tile", "stitch"])
def test_polygon_geometry_is_the_default_path_byte_for_byte(setup, stitch):
    """The centerline flags beside ``--geometry polygon`` change nothing either."""

    default = _run(setup, "default.geojson", stitch)
    assert default == _run(setup, "polygon.geojson", stitch + ["--geometry", "polygon", "--prune", "5", "--tolerance", "3"])
    doc = json.loads(default)
    assert len(doc["features"]) == (1 if stitch else 3) and all(f["geometry"]["type"] == "Polygon" for f in doc["features"])
