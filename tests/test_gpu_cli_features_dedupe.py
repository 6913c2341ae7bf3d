"""``./rs features --dedupe`` end to end on the MI355X: a synthetic slippy-map directory of 64 x 64 mask tiles and one of reference
labels -> GeoJSON, against the rule (``robosat_amd.features.dedupe_keep``'s definition) written out in numpy on the rasters the
tiles form.  Cleaning is the identity here (``--denoise 0 --grow 0``): what is under test is which polygons are left."""

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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["background", "parking", "building"]
INDEX = CLASSES.index("building")
Z, X0, Y0, SIZE = 18, 69623, 104945, 64
THRESHOLD = 0.5


def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _write(root, tiles, palette):
    for (x, y), image in tiles.items():
        os.makedirs(os.path.join(root, str(Z), str(x)), exist_ok=True)
        png.write_png(os.path.join(root, str(Z), str(x), str(y) + ".png"), image, "P", palette)


def _rasters():
    """Masks and reference over the columns X0 .. X0 + 3 of one tile row (column 2 has no tile at all); columns 0 | 1 share a seam."""

    masks = np.zeros((SIZE, 4 * SIZE), dtype=np.uint8)
    ref = np.zeros_like(masks)
    masks[4:14, 4:20] = INDEX
    ref[4:14, 4:20] = INDEX  # the same object: IoU 1
    masks[4:14, 30:40] = INDEX  # nothing under it ...
    ref[2:16, 28:42] = 1  # ... but another class
    masks[40:56, 4:20] = INDEX
    ref[52:60, 16:28] = INDEX  # a corner of it: 16 / (256 + 96 - 16)
    masks[24:34, 44:84] = INDEX  # across the seam, 200 pixels either side
    ref[24:34, 40:70] = INDEX  # under it: 240 pixels left of the seam, 60 right
    masks[10:30, 3 * SIZE + 10:3 * SIZE + 31] = INDEX  # in the tile whose reference file is missing
    ref[10:30, 3 * SIZE + 10:3 * SIZE + 31] = INDEX  # (what the missing file would have held: never written)
    masks[50:60, 100:120] = 1  # the other class is nobody's polygon
    return masks, ref


def _rule(pred, ref):
    """[(area, iou)] of the kept components of one raster, from label images."""

    kept = []
    for label in np.unique(pred[pred != 0]).tolist():
        mask = pred == label
        touched = np.unique(ref[mask & (ref != 0)]).tolist()
        inter = int((mask & (ref != 0)).sum())
        union = int(mask.sum()) + sum(int((ref == q).sum()) for q in touched) - inter
        if not touched:
            kept.append((int(mask.sum()), 0.0))
        elif inter < THRESHOLD * union:
            kept.append((int(mask.sum()), inter / union))
    return kept


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("features_dedupe")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking", "building"]\ncolors = ["denim", "orange", "green"]\n')
    palette = make_palette("denim", "orange", "green")
    masks, ref = _rasters()
    mask_tiles = S.split(masks, SIZE, SIZE, absent={(2, 0)}, x0=X0, y0=Y0)
    ref_tiles = S.split(ref, SIZE, SIZE, absent={(2, 0), (3, 0)}, x0=X0, y0=Y0)
    _write(str(tmp / "masks"), mask_tiles, palette)
    _write(str(tmp / "labels"), ref_tiles, palette)
    seen = ref.copy()
    seen[:, 3 * SIZE:] = 0  # no file, nothing mapped
    columns = [slice(c * SIZE, (c + 1) * SIZE) for c in (0, 1, 3)]
    per_tile = sorted(row for c in columns for row in _rule(R.label(masks[:, c] == INDEX), R.label(seen[:, c] == INDEX)))
    whole = sorted(_rule(R.label(masks == INDEX), R.label(seen == INDEX)))
    components = {"per_tile": sum(len(np.unique(R.label(masks[:, c] == INDEX))) - 1 for c in columns),
                  "whole": len(np.unique(R.label(masks == INDEX))) - 1}
    return {"tmp": tmp, "dataset": str(dataset), "masks": str(tmp / "masks"), "labels": str(tmp / "labels"), "palette": palette,
            "per_tile": per_tile, "whole": whole, "components": components, "ref_tiles": ref_tiles}


def _run(s, name, extra):
    out = str(s["tmp"] / name)
    done = _rs(["features", s["masks"], "--type", "building", "--dataset", s["dataset"], out, "--denoise", "0", "--grow", "0", "--simplify", "0"]
               + extra)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(out) as fp:
        return json.load(fp), done.stderr


def _found(doc):
    return sorted((f["properties"]["area_px"], f["properties"]["iou"]) for f in doc["features"])


def test_the_expectations_show_something(setup):
    """What the two runs below are held to, from the rule alone: with the objects whole the one across the seam is a duplicate; tile
    by tile its right half is not (60 of its 200 pixels are mapped there), so the two runs must differ."""

    assert setup["components"] == {"per_tile": 6, "whole": 5}
    assert setup["whole"] == [(100, 0.0), (256, 16 / 336), (420, 0.0)]
    assert setup["per_tile"] == [(100, 0.0), (200, 60 / 200), (256, 16 / 336), (420, 0.0)]
    assert setup["whole"] != setup["per_tile"]


def test_per_tile_drops_what_is_mapped_and_keeps_the_unmapped_half(setup):
    doc, stderr = _run(setup, "per_tile.geojson", ["--dedupe", setup["labels"], "--dedupe_threshold", str(THRESHOLD)])
    assert _found(doc) == setup["per_tile"]  # floats to the last bit
    assert all(set(f["properties"]) == {"tile", "area_px", "iou"} for f in doc["features"])
    by_area = {f["properties"]["area_px"]: f["properties"] for f in doc["features"]}
    assert by_area[100]["iou"] == 0 and 0 < by_area[256]["iou"] < THRESHOLD  # no counterpart; a slight overlap
    assert by_area[420]["tile"] == [X0 + 3, Y0, Z] and by_area[420]["iou"] == 0  # the tile without a reference file
    assert by_area[200]["tile"] == [X0 + 1, Y0, Z]  # the right half of the object on the seam
    assert "6 components examined, 2 dropped" in stderr


def test_stitched_compares_whole_objects_across_the_seam(setup):
    doc, stderr = _run(setup, "stitched.geojson", ["--stitch", "--dedupe", setup["labels"], "--dedupe_threshold", str(THRESHOLD)])
    assert _found(doc) == setup["whole"]
    assert all(set(f["properties"]) == {"tile", "area_px", "iou", "stitched"} for f in doc["features"])
    assert "5 components examined, 2 dropped" in stderr


def test_without_the_flag_every_component_is_a_feature_and_none_has_an_iou(setup):
    doc, stderr = _run(setup, "plain.geojson", [])
    assert len(doc["features"]) == setup["components"]["per_tile"]
    assert all(set(f["properties"]) == {"tile", "area_px"} for f in doc["features"])
    assert "examined" not in stderr


def test_a_reference_tile_of_another_size_and_centerlines_are_error_messages(setup):
    out = str(setup["tmp"] / "bad.geojson")
    wrong = str(setup["tmp"] / "wrong")
    tiles = dict(setup["ref_tiles"])
    tiles[(X0 + 1, Y0)] = np.zeros((32, 64), dtype=np.uint8)
    _write(wrong, tiles, setup["palette"])
    base = ["features", setup["masks"], "--type", "building", "--dataset", setup["dataset"], out, "--denoise", "0", "--grow", "0"]
    done = _rs(base + ["--dedupe", wrong, "--dedupe_threshold", "0.5"])
    assert done.returncode != 0 and "Error" in done.stderr and "Traceback" not in done.stderr and not os.path.exists(out)
    assert os.path.join(wrong, str(Z), str(X0 + 1), str(Y0) + ".png") in done.stderr
    done = _rs(base + ["--dedupe", setup["labels"], "--dedupe_threshold", "0.5", "--geometry", "centerline"])
    assert done.returncode != 0 and "Error" in done.stderr and "centerline" in done.stderr and "Traceback" not in done.stderr
    assert not os.path.exists(out)
