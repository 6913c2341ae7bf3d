"""``./rs evaluate`` end to end on the MI355X: a 2 x 2 block of 64 x 64 tiles, three classes, masks and labels cut from one pair of
128 x 128 rasters (one label tile missing), with ``--type building --boundary 3 --tiles``, once per tile and once with ``--stitch``,
against the restatement (tests/eval_ref.py) on the tiles and on the raster they form."""

import csv
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_ref as V  # noqa: E402
import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import png  # noqa: E402
from robosat_amd.colors import make_palette  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["background", "parking", "building"]
INDEX = CLASSES.index("building")
Z, X0, Y0, SIZE = 18, 69623, 104945, 64
D, T = 3, 0.5
MISSING = (0, 1)  # (column, row) of the tile without a label


def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _write(root, tiles, palette):
    for (x, y), image in tiles.items():
        os.makedirs(os.path.join(root, str(Z), str(x)), exist_ok=True)
        png.write_png(os.path.join(root, str(Z), str(x), str(y) + ".png"), image, "P", palette)


def _rasters():
    masks = np.zeros((2 * SIZE, 2 * SIZE), dtype=np.uint8)
    labels = np.zeros_like(masks)
    masks[10:20, 56:76] = INDEX
    labels[10:20, 54:74] = INDEX  # one object across the vertical seam (x = 64) on both sides
    masks[30:46, 50:64] = INDEX  # only in the masks; it ends at the seam, so its last column is in the band on the whole raster alone
    labels[44:54, 30:40] = INDEX  # only in the labels
    masks[80:100, 80:100] = INDEX
    labels[83:103, 80:100] = INDEX  # a pair moved by three pixels: 340 / 460
    masks[90:110, 20:40] = INDEX  # in the tile without a label: never evaluated
    labels[90:110, 20:40] = INDEX  # (what the missing file would have held: never written)
    masks[40:60, 90:120] = 1
    labels[44:60, 90:116] = 1  # the other class, for the matrix alone
    masks[110:120, 70:90] = 1
    labels[110:120, 70:90] = INDEX  # one class taken for the other
    return masks, labels


def _iou(table, k):
    inter = int(table[k, k])
    union = int(table[k, :].sum() + table[:, k].sum()) - inter
    return inter / union if union else None


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("evaluate")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking", "building"]\ncolors = ["denim", "orange", "green"]\n')
    palette = make_palette("denim", "orange", "green")
    masks, labels = _rasters()
    mask_tiles = S.split(masks, SIZE, SIZE, x0=X0, y0=Y0)
    label_tiles = S.split(labels, SIZE, SIZE, absent={MISSING}, x0=X0, y0=Y0)
    _write(str(tmp / "masks"), mask_tiles, palette)
    _write(str(tmp / "labels"), label_tiles, palette)
    keys = sorted(label_tiles)  # the evaluated tiles, in (x, y) order: the slots of a stitched call
    stack_p, stack_g = np.stack([mask_tiles[k] for k in keys]), np.stack([label_tiles[k] for k in keys])
    want = {"keys": keys}
    counts, bad = V.confusion(stack_p, stack_g, 3)
    assert not bad.any()
    want["per_tile_confusion"] = counts
    want["confusion"] = counts.sum(axis=0)
    # per tile
    tile_labels_p, tile_labels_g = [R.label(t == INDEX) for t in stack_p], [R.label(t == INDEX) for t in stack_g]
    want["objects"] = V.match(tile_labels_p, tile_labels_g, T)
    want["boundary"] = V.boundary(np.stack([V.band(t == INDEX, D) for t in stack_p]), np.stack([V.band(t == INDEX, D) for t in stack_g])).sum(axis=0)
    # the raster the three tiles form: the missing tile is absent (unknown to the transform), not background
    grid_p = S.Grid({k: (mask_tiles[k] == INDEX).astype(np.uint8) for k in keys}, 0)
    grid_g = S.Grid({k: (label_tiles[k] == INDEX).astype(np.uint8) for k in keys}, 0)
    want["objects_stitched"] = V.match([R.label(grid_p.canvas)], [R.label(grid_g.canvas)], T)
    want["boundary_stitched"] = V.boundary(V.band_stitched(grid_p, D), V.band_stitched(grid_g, D), stitched=True)[0]
    return {"tmp": tmp, "dataset": str(dataset), "masks": str(tmp / "masks"), "labels": str(tmp / "labels"), "palette": palette,
            "mask_tiles": mask_tiles, "want": want}


def _run(s, name, extra):
    out, tiles = str(s["tmp"] / (name + ".json")), str(s["tmp"] / (name + ".csv"))
    done = _rs(["evaluate", s["masks"], s["labels"], "--dataset", s["dataset"], out, "--type", "building", "--boundary", str(D), "--tiles",
                tiles] + extra)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(out) as fp:
        report = json.load(fp)
    with open(tiles, newline="") as fp:
        rows = list(csv.reader(fp))
    return report, rows, done.stderr


def _close(got, want):
    return (got is None and want is None) or abs(got - want) <= 1e-12


def _check_objects(got, want, stitched):
    matched, predicted, actual, ious = want
    assert (got["predicted"], got["actual"], got["matched"]) == (predicted, actual, matched)
    assert got["threshold"] == T and got["min_area"] == 0 and got["stitched"] is stitched
    assert _close(got["precision"], matched / predicted) and _close(got["recall"], matched / actual)
    assert _close(got["f1"], 2 * matched / (predicted + actual))
    assert _close(got["mean_matched_iou"], float(sum(ious) / len(ious)))


def _check_common(s, report, rows, stderr):
    want = s["want"]
    assert report["classes"] == CLASSES and report["tiles"] == 3 and report["tiles_without_label"] == 1 and report["type"] == "building"
    assert report["confusion"] == want["confusion"].tolist() and report["pixels"] == 3 * SIZE * SIZE
    assert "1 mask tiles without a label" in stderr
    for k, name in enumerate(CLASSES):
        assert _close(report["iou"][name], _iou(want["confusion"], k))
    assert _close(report["miou"], float(np.mean([_iou(want["confusion"], k) for k in range(3)])))
    assert _close(report["fg_iou"], _iou(want["confusion"], 1))
    assert _close(report["accuracy"], int(np.trace(want["confusion"])) / (3 * SIZE * SIZE)) and -1 <= report["mcc"] <= 1
    # the list: worst building IoU first, then (z, x, y)
    assert rows[0] == ["z", "x", "y", "pixels", "iou_background", "iou_parking", "iou_building", "miou", "predicted_share", "actual_share"]
    expected = sorted(((_iou(table, INDEX), Z, x, y, table) for (x, y), table in zip(want["keys"], want["per_tile_confusion"])),
                      key=lambda e: e[:4])
    assert all(e[0] is not None for e in expected) and len({e[0] for e in expected}) == 3  # (three different values: the order shows)
    assert [(int(r[0]), int(r[1]), int(r[2])) for r in rows[1:]] == [(z, x, y) for _, z, x, y, _ in expected]
    for row, (iou, _, _, _, table) in zip(rows[1:], expected):
        assert int(row[3]) == SIZE * SIZE and _close(float(row[6]), iou)
        assert _close(float(row[8]), int(table[:, 1:].sum()) / SIZE ** 2) and _close(float(row[9]), int(table[1:, :].sum()) / SIZE ** 2)


def test_the_expectations_show_something(setup):
    """From the restatement alone: the object on the seam is two objects per tile and one on the raster, on both sides."""

    want = setup["want"]
    assert want["objects"][:3] == (3, 4, 5) and want["objects_stitched"][:3] == (2, 3, 4)
    assert sorted(want["objects_stitched"][3]) == [Fraction(340, 460), Fraction(18, 22)]
    assert (want["boundary"] != want["boundary_stitched"]).any() and want["boundary"][2] > 0
    assert all(want["confusion"][a, p] > 0 for a, p in ((0, 0), (1, 1), (2, 2), (0, 2), (2, 0), (2, 1), (0, 1)))


def test_per_tile(setup):
    report, rows, stderr = _run(setup, "per_tile", [])
    _check_common(setup, report, rows, stderr)
    want = setup["want"]
    _check_objects(report["objects"], want["objects"], False)
    predicted, actual, shared = (int(v) for v in want["boundary"])
    assert report["boundary"] == {"d": D, "predicted": predicted, "actual": actual, "shared": shared, "iou": report["boundary"]["iou"]}
    assert _close(report["boundary"]["iou"], shared / (predicted + actual - shared))


def test_stitched(setup):
    report, rows, stderr = _run(setup, "stitched", ["--stitch"])
    _check_common(setup, report, rows, stderr)
    want = setup["want"]
    _check_objects(report["objects"], want["objects_stitched"], True)
    predicted, actual, shared = (int(v) for v in want["boundary_stitched"])
    assert report["boundary"] == {"d": D, "predicted": predicted, "actual": actual, "shared": shared, "iou": report["boundary"]["iou"]}
    assert _close(report["boundary"]["iou"], shared / (predicted + actual - shared))
    # the object on the seam: twice per tile, once here, on each side
    assert report["objects"]["predicted"] == want["objects"][1] - 1 and report["objects"]["actual"] == want["objects"][2] - 1


def test_a_byte_that_is_no_class_ends_the_run_and_names_the_tile(setup):
    out = str(setup["tmp"] / "bad.json")
    wrong = str(setup["tmp"] / "wrong")
    tiles = {k: v.copy() for k, v in setup["mask_tiles"].items()}
    tiles[(X0 + 1, Y0 + 1)][5, 6] = 7
    _write(wrong, tiles, setup["palette"])
    done = _rs(["evaluate", wrong, setup["labels"], "--dataset", setup["dataset"], out])
    assert done.returncode != 0 and "Error" in done.stderr and "Traceback" not in done.stderr and not os.path.exists(out)
    assert "{}/{}/{}".format(Z, X0 + 1, Y0 + 1) in done.stderr
