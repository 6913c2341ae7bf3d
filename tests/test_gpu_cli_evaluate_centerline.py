"""``./rs evaluate --type road --centerline RHO`` end to end on the MI355X: a 2 x 2 block of 64 x 64 tiles with roads, the masks being
the labels moved by two pixels, per tile and with ``--stitch``, against the restatement (tests/centerline_eval_ref.py) computed
from the same PNGs; the ``--tiles`` columns; and a run without the flag, whose report does not know the key."""

import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import centerline_eval_ref as C  # noqa: E402
import stitch_ref as S  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import evaluate as H  # noqa: E402
from robosat_amd import png  # noqa: E402
from robosat_amd.colors import make_palette  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["background", "road"]
Z, X0, Y0, SIZE = 18, 69623, 104945, 64
COLUMNS = ["centerline_completeness", "centerline_correctness", "centerline_quality"]


def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _write(root, tiles, palette):
    for (x, y), image in tiles.items():
        os.makedirs(os.path.join(root, str(Z), str(x)), exist_ok=True)
        png.write_png(os.path.join(root, str(Z), str(x), str(y) + ".png"), image, "P", palette)


def _read(root, keys):
    return {(x, y): np.array(Image.open(os.path.join(root, str(Z), str(x), str(y) + ".png"))) for x, y in keys}


def _want(tiles_p, tiles_g, rho):
    """(the eight counts per tile in (x, y) order, the eight counts of the raster the tiles form) of class 1."""

    keys = sorted(tiles_p)
    masks_p, masks_g = [(tiles_p[k] == 1).astype(np.uint8) for k in keys], [(tiles_g[k] == 1).astype(np.uint8) for k in keys]
    per_tile = C.counts_tiles([T.thin(m) for m in masks_p], [T.thin(m) for m in masks_g], rho)
    grids = []
    for masks in (masks_p, masks_g):
        grid = S.Grid(dict(zip(keys, masks)), 0)
        grids.append(S.Grid(dict(zip(keys, grid.cut(T.thin(grid.canvas)))), 0))
    return per_tile, C.counts_grid(grids[0], grids[1], rho)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("evaluate_centerline")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "road"]\ncolors = ["denim", "orange"]\n')
    palette = make_palette("denim", "orange")
    labels = T.roads(2 * SIZE, 2 * SIZE, 11, count=4, width=7).astype(np.uint8)
    masks = np.zeros_like(labels)
    masks[:, 2:] = labels[:, :-2]  # the labels moved two pixels east
    _write(str(tmp / "masks"), S.split(masks, SIZE, SIZE, x0=X0, y0=Y0), palette)
    _write(str(tmp / "labels"), S.split(labels, SIZE, SIZE, x0=X0, y0=Y0), palette)
    keys = sorted(S.split(masks, SIZE, SIZE, x0=X0, y0=Y0))
    tiles_p, tiles_g = _read(str(tmp / "masks"), keys), _read(str(tmp / "labels"), keys)
    state = {"tmp": tmp, "dataset": str(dataset), "masks": str(tmp / "masks"), "labels": str(tmp / "labels"), "keys": keys, "runs": {},
             "want": {rho: _want(tiles_p, tiles_g, rho) for rho in (1, 3)}}
    return state


def _run(s, name, extra):
    """One run per name, shared by the tests: (report, the CSV's rows, the report's text)."""

    if name not in s["runs"]:
        out, tiles = str(s["tmp"] / (name + ".json")), str(s["tmp"] / (name + ".csv"))
        done = _rs(["evaluate", s["masks"], s["labels"], "--dataset", s["dataset"], out, "--type", "road", "--tiles", tiles] + extra)
        assert done.returncode == 0, done.stderr[-2000:]
        with open(out) as fp:
            text = fp.read()
        with open(tiles, newline="") as fp:
            rows = list(csv.reader(fp))
        s["runs"][name] = json.loads(text), rows, text
    return s["runs"][name]


def _check(report, rho, counts):
    got = report["centerline"]
    want = H.centerline_report(rho, counts)
    assert [got[side][k] for side in ("predicted", "actual") for k in ("straight", "diagonal", "matched_straight", "matched_diagonal")] == counts
    assert got == want  # (the floats too: formed from the same integers by the same expressions)
    keys = list(report)
    assert keys.index("centerline") == keys.index("objects") + 1  # (no --boundary, no --probs here: behind the objects, the last key)


def test_the_expectations_show_something(setup):
    per_tile, whole = setup["want"][3]
    total = np.array(per_tile).sum(axis=0)
    assert total[0] and total[4] and 0 < total[2] and 0 < total[6]
    assert whole != total.tolist() and whole[0] > total[0]  # (per tile the skeletons stop short of the seams)
    assert setup["want"][1][1][2:4] != whole[2:4]  # a shift of two pixels: a tolerance of one matches less


def test_per_tile(setup):
    report, rows, _ = _run(setup, "per_tile_3", ["--centerline", "3"])
    per_tile, _ = setup["want"][3]
    _check(report, 3, np.array(per_tile).sum(axis=0).tolist())
    assert rows[0][-3:] == COLUMNS and len(rows) == 5
    by_tile = {(int(r[1]), int(r[2])): r[-3:] for r in rows[1:]}
    for key, counts in zip(setup["keys"], per_tile):
        want = H.centerline_scores(counts)
        assert by_tile[key] == ["" if v is None else repr(v) for v in want]


def test_stitched(setup):
    report, rows, _ = _run(setup, "stitched_3", ["--centerline", "3", "--stitch"])
    _check(report, 3, setup["want"][3][1])
    assert not set(COLUMNS) & set(rows[0]) and len(rows) == 5  # a stitched call has no per-tile counts


@pytest.mark.parametrize("extra, which", [([], 0), (["--stitch"], 1)], ids=["per_tile", "stitched"])
def test_a_smaller_tolerance_matches_no_more(setup, extra, which):
    wide, _, _ = _run(setup, ("stitched_3" if which else "per_tile_3"), ["--centerline", "3"] + extra)
    narrow, _, _ = _run(setup, ("stitched_1" if which else "per_tile_1"), ["--centerline", "1"] + extra)
    want = setup["want"][1][which]
    _check(narrow, 1, want if which else np.array(want).sum(axis=0).tolist())
    for side in ("predicted", "actual"):
        assert narrow["centerline"][side]["matched_length"] <= wide["centerline"][side]["matched_length"]
        assert narrow["centerline"][side]["length"] == wide["centerline"][side]["length"]


def test_without_the_flag_the_report_does_not_know_the_key(setup):
    report, rows, text = _run(setup, "plain", [])
    assert "centerline" not in report and "centerline" not in text and not set(COLUMNS) & set(rows[0])
    rebuilt = H.build_report(CLASSES, report["confusion"], report["tiles"], report["tiles_without_label"], kind="road",
                             objects=report["objects"])
    assert text == json.dumps(rebuilt, indent=2, allow_nan=False) + "\n"
    with_flag, _, _ = _run(setup, "per_tile_3", ["--centerline", "3"])
    assert {k: v for k, v in with_flag.items() if k != "centerline"} == report  # the other views did not move
