"""``./rs features --split`` end to end on the MI355X: synthetic slippy-map directories of 64 x 64 mask tiles holding the dumbbell of
tests/split_ref.py (two 21 x 21 squares joined by a neck 3 wide and 9 long) -> GeoJSON.  Cleaning is the identity here
(``--denoise 0 --grow 0``) and nothing is simplified: what is under test is which polygons come out, and where the cut lies."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import split_ref as P  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import png  # noqa: E402
from robosat_amd.colors import make_palette  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX = 2  # "building"
Z, X0, Y0, SIZE = 18, 69623, 104945, 64
SQUARE, NECK = 21 * 21, 3


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
    tmp = tmp_path_factory.mktemp("features_split")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking", "building"]\ncolors = ["denim", "orange", "green"]\n')
    palette = make_palette("denim", "orange", "green")
    one = P.dumbbell().astype(np.uint8) * INDEX  # squares at columns 4..24 and 34..54, the neck's middle column 29
    one[45:50, 5:60] = INDEX  # a bar 5 high: no disc of radius 4 fits, it stays what it is
    _write(str(tmp / "one"), {(X0, Y0): one}, palette)
    reference = np.zeros_like(one)
    reference[8:29, 4:25] = INDEX  # the left square alone is mapped already
    _write(str(tmp / "labels"), {(X0, Y0): reference}, palette)
    two = P.dumbbell(h=64, w=128, x0=37).astype(np.uint8) * INDEX  # squares at 37..57 and 67..87, the neck 58..66: the seam at 64 cuts it
    _write(str(tmp / "two"), S.split(two, SIZE, SIZE, x0=X0, y0=Y0), palette)
    # the blob tiles of test_gpu_cli_features.py (features_ref.blobs, both foreground classes), for the run that must not change
    blobs = {}
    for i in range(2):
        image = np.where(R.blobs(128, 128, i, 5), 2, 0).astype(np.uint8)
        image[R.blobs(128, 128, 50 + i, 3)] = 1
        blobs[(X0, Y0 + i)] = image
    _write(str(tmp / "blobs"), blobs, palette)
    return {"tmp": tmp, "dataset": str(dataset), "one": str(tmp / "one"), "two": str(tmp / "two"), "labels": str(tmp / "labels"),
            "blobs": str(tmp / "blobs")}


def _run(s, masks, name, extra, raw=False, discs=("--denoise", "0", "--grow", "0", "--simplify", "0")):
    out = str(s["tmp"] / name)
    done = _rs(["features", s[masks], "--type", "building", "--dataset", s["dataset"], out] + list(discs) + extra)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(out, "rb") as fp:
        data = fp.read()
    return data if raw else (json.loads(data), done.stderr)


def _areas(doc):
    return sorted(f["properties"]["area_px"] for f in doc["features"])


def _columns(feature):
    """Mosaic pixel columns of the outer ring's vertices, the closing one left out (longitude is linear over the zoom level)."""

    gx = np.array([(lon + 180.0) / 360.0 * 2 ** Z * SIZE - X0 * SIZE for lon, _ in feature["geometry"]["coordinates"][0][:-1]])
    assert np.abs(gx - np.rint(gx)).max() < 1e-3, "vertices are pixel corners"
    return np.rint(gx).astype(int)


def test_the_dumbbell_is_one_feature_without_the_flag_and_two_with_it(setup):
    doc, _ = _run(setup, "one", "plain.geojson", [])
    assert _areas(doc) == [5 * 55, 2 * SQUARE + 9 * NECK]
    doc, _ = _run(setup, "one", "split.geojson", ["--split", "4"])
    assert _areas(doc) == [5 * 55, SQUARE + 4 * NECK, SQUARE + 5 * NECK], "the neck's middle column goes to the left instance"
    assert all(set(f["properties"]) == {"tile", "area_px"} and f["geometry"]["type"] == "Polygon" for f in doc["features"])
    left, right = (f for f in doc["features"] if f["properties"]["area_px"] > 5 * 55)
    if left["properties"]["area_px"] < right["properties"]["area_px"]:
        left, right = right, left
    assert _columns(left).max() == 30 == _columns(right).min(), "both outlines run along the cut behind column 29"


def test_stitched_the_cut_is_where_the_fronts_meet_not_on_the_seam(setup):
    doc, _ = _run(setup, "two", "stitched.geojson", ["--stitch", "--split", "4"])
    assert _areas(doc) == [SQUARE + 4 * NECK, SQUARE + 5 * NECK]
    assert all(f["properties"]["stitched"] is True for f in doc["features"])
    left, right = sorted(doc["features"], key=lambda f: -f["properties"]["area_px"])
    assert _columns(left).max() == 63 == _columns(right).min(), "the cut behind the neck's middle column 62"
    for f in doc["features"]:
        gx = _columns(f)
        assert not ((gx == SIZE) & (np.roll(gx, -1) == SIZE)).any(), "a straight edge on the seam"
    doc, _ = _run(setup, "two", "stitched_plain.geojson", ["--stitch"])
    assert _areas(doc) == [2 * SQUARE + 9 * NECK]
    doc, _ = _run(setup, "two", "per_tile.geojson", ["--split", "4"])
    assert _areas(doc) == [SQUARE + 3 * NECK, SQUARE + 6 * NECK], "tile by tile the seam is the cut: that is what --stitch is for"


def test_dedupe_sees_instances_the_mapped_square_goes_and_the_other_gains_iou(setup):
    doc, stderr = _run(setup, "one", "dedupe.geojson", ["--split", "4", "--dedupe", setup["labels"], "--dedupe_threshold", "0.5"])
    assert _areas(doc) == [5 * 55, SQUARE + 4 * NECK]
    assert all(f["properties"]["iou"] == 0 for f in doc["features"])
    assert "3 components examined, 1 dropped" in stderr
    doc, stderr = _run(setup, "one", "dedupe_whole.geojson", ["--dedupe", setup["labels"], "--dedupe_threshold", "0.5"])
    assert _areas(doc) == [5 * 55, 2 * SQUARE + 9 * NECK], "unsplit, the square is less than half of the blob: nothing is dropped"
    assert sorted(f["properties"]["iou"] for f in doc["features"]) == [0, SQUARE / (2 * SQUARE + 9 * NECK)]


def test_min_area_between_the_two_instances_keeps_one(setup):
    doc, _ = _run(setup, "one", "min_area.geojson", ["--split", "4", "--min_area", str(SQUARE + 5 * NECK)])
    assert _areas(doc) == [SQUARE + 5 * NECK]


def test_split_0_is_the_flag_left_out_byte_for_byte(setup):
    for masks, extra in (("one", []), ("two", ["--stitch", "--dedupe", setup["labels"], "--dedupe_threshold", "0.5"])):
        assert _run(setup, masks, "absent.geojson", extra, raw=True) == _run(setup, masks, "zero.geojson", extra + ["--split", "0"], raw=True)
    discs = ("--denoise", "5", "--grow", "4", "--min_area", "12")  # (the discs test_gpu_cli_features.py runs these tiles with)
    plain = _run(setup, "blobs", "absent.geojson", [], raw=True, discs=discs)
    assert plain == _run(setup, "blobs", "zero.geojson", ["--split", "0"], raw=True, discs=discs) and len(json.loads(plain)["features"]) > 2
