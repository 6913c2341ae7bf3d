"""``./rs features`` end to end on the MI355X: synthetic slippy-map mask directories -> GeoJSON -> back to pixels, against the CPU
restatement of select -> open -> close -> min_area (tests/features_ref.py)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402

from robosat_amd import png  # noqa: E402
from robosat_amd.colors import make_palette  # noqa: E402
from robosat_amd.tiles import Tile, tile_bounds  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["background", "parking", "building"]
DENOISE, GROW, MIN_AREA = 5, 4, 12


def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("features")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking", "building"]\ncolors = ["denim", "orange", "green"]\n')
    palette = make_palette("denim", "orange", "green")
    tiles = {}
    shapes = [(128, 128)] * 5 + [(96, 160)] * 3  # two shapes; 5 tiles of one shape with --batch_size 2 leaves a ragged batch
    coords = [(69623, 104945, 18), (69623, 104946, 18), (69624, 104945, 18), (3, 5, 4), (0, 0, 0), (69625, 104945, 18), (2, 5, 4), (1, 1, 1)]
    for i, ((x, y, z), (h, w)) in enumerate(zip(coords, shapes)):
        rng = np.random.RandomState(i)
        image = np.where(R.blobs(h, w, i, 5), 2, 0).astype(np.uint8)
        image[R.blobs(h, w, 50 + i, 3)] = 1  # the other foreground class, over it
        if i == 2:
            image[:] = 2  # a full tile
        if i == 3:
            image[image == 2] = 0  # a tile without the class
        if i == 4:
            image[20:100, 24:110] = 2
            image[45:75, 50:85] = 0  # a polygon with a hole
        os.makedirs(str(tmp / "masks" / str(z) / str(x)), exist_ok=True)
        png.write_png(str(tmp / "masks" / str(z) / str(x) / (str(y) + ".png")), image, "P", palette)
        tiles[(x, y, z)] = image
    return {"tmp": tmp, "dataset": str(dataset), "masks": str(tmp / "masks"), "tiles": tiles}


def _run(s, name, extra):
    out = str(s["tmp"] / name)
    done = _rs(["features", s["masks"], "--type", "building", "--dataset", s["dataset"], out, "--denoise", str(DENOISE), "--grow", str(GROW),
                "--min_area", str(MIN_AREA), "--batch_size", "2"] + extra)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(out, "rb") as fp:
        return fp.read()


def _check_rings(doc):
    for f in doc["features"]:
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon"
        for ring in f["geometry"]["coordinates"]:
            assert len(ring) >= 4 and ring[0] == ring[-1]


def test_simplify_zero_maps_back_to_the_restated_mask(setup):
    doc = json.loads(_run(setup, "exact.geojson", ["--simplify", "0"]))
    assert doc["type"] == "FeatureCollection"
    _check_rings(doc)
    keys = [(f["properties"]["tile"][2], f["properties"]["tile"][0], f["properties"]["tile"][1]) for f in doc["features"]]
    assert keys == sorted(keys)
    seen = set()
    for (x, y, z), image in setup["tiles"].items():
        h, w = image.shape
        labels = R.filter_labels(R.label(R.clean(image, CLASSES.index("building"), DENOISE, GROW)), MIN_AREA)
        west, south, east, north = tile_bounds(Tile(x, y, z))
        rebuilt = np.zeros((h, w), dtype=bool)
        features = [f for f in doc["features"] if f["properties"]["tile"] == [x, y, z]]
        assert len(features) == len(np.unique(labels[labels != 0]))
        for f in features:
            rings = []
            for ring in f["geometry"]["coordinates"]:
                px = np.array([[(lon - west) / (east - west) * w, (lat - north) / (south - north) * h] for lon, lat in ring[:-1]])
                assert np.abs(px - np.rint(px)).max() < 1e-4, "vertices are pixel corners"
                rings.append(np.rint(px))
            inside = R.fill_even_odd(rings, h, w)
            assert inside.sum() == f["properties"]["area_px"] and not (rebuilt & inside).any()
            rebuilt |= inside
        assert (rebuilt == (labels != 0)).all(), (x, y, z)
        seen.add((x, y, z))
        if features:
            # RFC 7946: the outer ring counter-clockwise in lon / lat
            ring = np.array(features[0]["geometry"]["coordinates"][0][:-1])
            assert np.sum(ring[:, 0] * np.roll(ring[:, 1], -1) - np.roll(ring[:, 0], -1) * ring[:, 1]) > 0
    assert len(seen) == 8 and any(len(f["geometry"]["coordinates"]) > 1 for f in doc["features"]), "no feature with a hole"


def test_defaults_simplify_and_repeat_byte_for_byte(setup):
    exact = json.loads(_run(setup, "exact2.geojson", ["--simplify", "0"]))
    first = _run(setup, "default.geojson", [])
    second = _run(setup, "default_again.geojson", [])
    assert first == second
    doc = json.loads(first)
    _check_rings(doc)
    assert 0 < len(doc["features"]) <= len(exact["features"])

    def identity(f):
        # the outer ring's lexicographically smallest pixel vertex (smallest lon, then largest lat): simplification starts there and keeps it
        return tuple(f["properties"]["tile"]), min((lon, -lat) for lon, lat in f["geometry"]["coordinates"][0])

    count = {}
    for f in exact["features"]:
        assert identity(f) not in count
        count[identity(f)] = sum(len(r) for r in f["geometry"]["coordinates"])
    for f in doc["features"]:
        assert sum(len(r) for r in f["geometry"]["coordinates"]) <= count[identity(f)]


def test_an_oversized_batch_size_is_clamped(setup):
    assert _run(setup, "huge_batch.geojson", ["--simplify", "0", "--batch_size", "5000"]) == _run(setup, "exact3.geojson", ["--simplify", "0"])


def test_a_bad_type_is_an_error_message_not_a_traceback(setup):
    for bad in ("road", "background"):
        done = _rs(["features", setup["masks"], "--type", bad, "--dataset", setup["dataset"], str(setup["tmp"] / "bad.geojson")])
        assert done.returncode != 0 and "Error" in done.stderr and "Traceback" not in done.stderr
        assert not os.path.exists(str(setup["tmp"] / "bad.geojson"))
