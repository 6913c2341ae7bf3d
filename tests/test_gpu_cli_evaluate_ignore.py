"""``./rs evaluate --type T --boundary 2 --centerline 2 --ignored unknown`` end to end on the MI355X: six 64 x 64 tiles of one zoom
level (three columns, two rows) whose labels hold ignored rectangles that cut an object, swallow a predicted object whole and
cross a tile seam; per tile and with ``--stitch`` against the restatement (tests/eval_ignore_ref.py); a three-class copy with
``--probs``, which ends the run without the flag; a copy without ignored pixels, on which the flag changes nothing but its own
key; and the ``--tiles`` rows."""

import csv
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_ignore_ref as N  # noqa: E402
import prob_ref as P  # noqa: E402
import stitch_ref as S  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import evaluate as H  # noqa: E402
from robosat_amd import png  # noqa: E402
from robosat_amd.colors import continuous_palette_for_color  # noqa: E402

pytestmark = pytest.mark.gpu

Z, X0, Y0, SIZE = 18, 69623, 104945, 64
IGNORE, D, RHO, MATCH = 255, 2, 2, 0.5
SHADES = continuous_palette_for_color("pink", 256)  # 256 entries: a label tile holds the byte 255
TYPED = ["--boundary", str(D), "--centerline", str(RHO)]


def _rs(args):
    """``./rs`` with these arguments, through the entry point's own parser, in this process (a process per call costs seconds)."""

    from robosat_amd.tools import __main__ as entry

    argv, sys.argv = sys.argv, ["./rs"] + list(args)
    try:
        entry.main()
    finally:
        sys.argv = argv


def _write(root, tiles, mode="P", palette=SHADES):
    for (x, y), image in tiles.items():
        os.makedirs(os.path.join(root, str(Z), str(x)), exist_ok=True)
        png.write_png(os.path.join(root, str(Z), str(x), str(y) + ".png"), image, mode, palette)
    return root


def _rasters():
    """(masks, labels, labels before the ignored rectangles) uint8 [128, 192], class 1."""

    labels = np.zeros((2 * SIZE, 3 * SIZE), dtype=np.uint8)
    labels[8:24, 8:40] = 1        # cut in two by an ignored rectangle
    labels[40:56, 56:72] = 1      # across the seam x = 64, with an ignored rectangle across the same seam beside it
    labels[70:90, 100:120] = 1    # left whole
    labels[100:120, 20:50] = 1
    labels[30:50, 150:180] = 1
    labels |= T.roads(2 * SIZE, 3 * SIZE, 4, count=2, width=5).astype(np.uint8)  # two roads through everything, seams and rectangles
    masks = np.roll(labels, (2, 1), axis=(0, 1))
    masks[100:110, 150:160] = 1   # a predicted object that an ignored rectangle swallows whole
    masks[4:10, 170:180] = 1      # and one that matches nothing
    before = labels.copy()
    labels[4:30, 20:28] = IGNORE      # through the first object, top to bottom
    labels[96:114, 146:164] = IGNORE  # round the predicted object
    labels[60:68, 56:72] = IGNORE     # across the seams x = 64 and y = 64
    labels[30:60, 60:68] = IGNORE     # across the seam x = 64, through the object on it
    return masks, labels, before


def _split(raster):
    return S.split(raster, SIZE, SIZE, x0=X0, y0=Y0)


def _want(masks, labels, index):
    """The restatement's numbers, per tile (tiles in (x, y) order) and of the raster the tiles form."""

    tiles_p, tiles_a = _split(masks), _split(labels)
    keys = sorted(tiles_p)
    coded = [N.coded(tiles_p[k], tiles_a[k], index, IGNORE) for k in keys]
    cp, cg = np.stack([c[0] for c in coded]), np.stack([c[1] for c in coded])
    links = N.centerline_counts(cp, cg, RHO)
    gp, gg = N.grid(dict(zip(keys, cp))), N.grid(dict(zip(keys, cg)))
    return {
        "keys": keys,
        "boundary": N.band_counts(cp, cg, D).sum(axis=0).tolist(),
        "objects": N.objects(cp, cg, MATCH),
        "tile_links": links,
        "links": np.array(links).sum(axis=0).tolist(),
        "boundary_stitched": N.band_counts_grid(gp, gg, D).tolist(),
        "objects_stitched": N.objects_grid(gp, gg, MATCH),
        "links_stitched": N.centerline_counts_grid(gp, gg, RHO),
        "ignored": int((labels == IGNORE).sum()),
        "tile_ignored": {k: int((tiles_a[k] == IGNORE).sum()) for k in keys},
    }


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("evaluate_ignore")
    masks, labels, before = _rasters()
    two = tmp / "two.toml"
    two.write_text('[common]\nclasses = ["background", "building"]\ncolors = ["denim", "orange"]\nignore = 255\n')
    three = tmp / "three.toml"
    three.write_text('[common]\nclasses = ["background", "parking", "building"]\ncolors = ["denim", "orange", "green"]\nignore = 255\n')
    masks3, labels3 = (2 * masks).astype(np.uint8), np.where(labels == IGNORE, IGNORE, 2 * labels).astype(np.uint8)
    masks3[60:70, 130:150] = 1
    labels3[62:72, 130:150] = np.where(labels3[62:72, 130:150] == 0, 1, labels3[62:72, 130:150])  # the other class, for the matrix alone
    rng = np.random.RandomState(3)
    probs = np.stack([np.clip(np.rint(np.where(labels3 == c, 170.0, 70.0) + rng.normal(0, 50, size=labels3.shape)), 0, 255) for c in (1, 2)],
                     axis=-1).astype(np.uint8)
    return {
        "tmp": tmp, "two": str(two), "three": str(three), "runs": {},
        "masks": _write(str(tmp / "masks"), _split(masks)), "labels": _write(str(tmp / "labels"), _split(labels)),
        "known": _write(str(tmp / "known"), _split(before)),
        "masks3": _write(str(tmp / "masks3"), _split(masks3)), "labels3": _write(str(tmp / "labels3"), _split(labels3)),
        "probs3": _write(str(tmp / "probs3"), {(X0 + c, Y0 + r): np.ascontiguousarray(probs[r * SIZE:(r + 1) * SIZE, c * SIZE:(c + 1) * SIZE])
                                               for r in range(2) for c in range(3)}, "LA", None),
        "want": _want(masks, labels, 1), "want_known": _want(masks, before, 1), "want3": _want(masks3, labels3, 2),
        "arrays3": (probs, labels3),
    }


def _run(s, name, masks, labels, dataset, extra):
    """One run per name, shared by the tests: (report, the CSV's rows as dicts)."""

    if name not in s["runs"]:
        out, tiles = str(s["tmp"] / (name + ".json")), str(s["tmp"] / (name + ".csv"))
        _rs(["evaluate", s[masks], s[labels], "--dataset", s[dataset], out, "--tiles", tiles] + extra)
        with open(out) as fp:
            report = json.load(fp)
        with open(tiles, newline="") as fp:
            rows = list(csv.DictReader(fp))
        s["runs"][name] = report, rows
    return s["runs"][name]


def _check(report, want, stitched, kind="building"):
    suffix = "_stitched" if stitched else ""
    predicted, actual, shared = want["boundary" + suffix]
    assert report["boundary"] == H.boundary_report(D, (predicted, actual, shared))
    matched, n_predicted, n_actual, ious = want["objects" + suffix]
    got = report["objects"]
    assert (got["matched"], got["predicted"], got["actual"], got["stitched"]) == (matched, n_predicted, n_actual, stitched)
    # (the one float of the objects: the exactly rounded sum of the matches' IoUs, each the float nearest its fraction, over their number)
    assert got["mean_matched_iou"] == math.fsum(float(f) for f in ious) / len(ious) and got["threshold"] == MATCH and got["min_area"] == 0
    assert report["centerline"] == H.centerline_report(RHO, want["links" + suffix])
    assert report["type"] == kind and report["ignore"] == IGNORE and report["ignored"] == want["ignored"] and report["ignored_as"] == "unknown"
    keys = list(report)
    assert keys.index("ignored_as") == keys.index("ignored") + 1


def test_the_expectations_show_something(setup):
    want, known = setup["want"], setup["want_known"]
    assert want["ignored"] == 26 * 8 + 18 * 18 + 8 * 16 + 30 * 8 and sum(n > 0 for n in want["tile_ignored"].values()) >= 4
    for key in ("boundary", "links", "boundary_stitched", "links_stitched"):
        assert want[key] != known[key] and all(v > 0 for v in want[key][:3])
    assert want["objects"][:3] != known["objects"][:3] and want["objects_stitched"][:3] != known["objects_stitched"][:3]
    assert want["objects"][0] > 0 and want["objects_stitched"][0] > 0
    assert want["objects"][:3] != want["objects_stitched"][:3]  # objects across the seams
    # the swallowed object: predicted pixels all of which are unknown, so none of them is in P
    masks, labels, _ = _rasters()
    assert (masks[100:110, 150:160] == 1).all() and (N.coded(masks, labels, 1, IGNORE)[0][100:110, 150:160] == 2).all()


def test_per_tile(setup):
    report, rows = _run(setup, "per_tile", "masks", "labels", "two", ["--type", "building", "--ignored", "unknown"] + TYPED)
    _check(report, setup["want"], False)
    pixel_view, _ = _run(setup, "pixels", "masks", "labels", "two", [])
    assert "ignored_as" not in pixel_view and "objects" not in pixel_view
    for key in ("ignore", "ignored", "pixels", "confusion", "tiles", "iou", "miou"):
        assert report[key] == pixel_view[key]


def test_stitched(setup):
    report, _ = _run(setup, "stitched", "masks", "labels", "two", ["--type", "building", "--ignored", "unknown", "--stitch"] + TYPED)
    _check(report, setup["want"], True)
    per_tile, _ = _run(setup, "per_tile", "masks", "labels", "two", ["--type", "building", "--ignored", "unknown"] + TYPED)
    assert report["confusion"] == per_tile["confusion"] and report["ignored"] == per_tile["ignored"]


def test_the_tile_list_has_its_rows(setup):
    _, rows = _run(setup, "per_tile", "masks", "labels", "two", ["--type", "building", "--ignored", "unknown"] + TYPED)
    _, plain = _run(setup, "pixels", "masks", "labels", "two", [])
    want = setup["want"]
    assert len(rows) == 6 and list(rows[0])[:5] == ["z", "x", "y", "pixels", "ignored"]
    by_tile = {(int(r["x"]), int(r["y"])): r for r in rows}
    for key, counts in zip(want["keys"], want["tile_links"]):
        row = by_tile[key]
        assert int(row["ignored"]) == want["tile_ignored"][key] and int(row["pixels"]) == SIZE * SIZE - want["tile_ignored"][key]
        scores = H.centerline_scores(counts)
        assert [row[c] for c in H.CENTERLINE_COLUMNS] == ["" if v is None else repr(v) for v in scores]
    # every column the pixel view's list has holds what it held there
    plain_by_tile = {(int(r["x"]), int(r["y"])): r for r in plain}
    for key, row in by_tile.items():
        assert {k: row[k] for k in plain_by_tile[key]} == plain_by_tile[key]


def test_without_the_flag_the_run_ends_as_it_did(setup):
    out = str(setup["tmp"] / "refused.json")
    with pytest.raises(SystemExit) as exc:
        _rs(["evaluate", setup["masks"], setup["labels"], "--dataset", setup["two"], out, "--type", "building"] + TYPED)
    message = str(exc.value)
    assert message.startswith("Error: the label of tile 18/") and "ignore value 255" in message and "--type" in message
    assert "--ignored unknown" in message and not os.path.exists(out)


def test_three_classes_get_their_probability_view(setup):
    extra = ["--type", "building", "--probs", setup["probs3"]] + TYPED
    out = str(setup["tmp"] / "probs_refused.json")
    with pytest.raises(SystemExit) as exc:  # today's run
        _rs(["evaluate", setup["masks3"], setup["labels3"], "--dataset", setup["three"], out] + extra)
    assert "ignore value 255" in str(exc.value) and not os.path.exists(out)
    report, _ = _run(setup, "three", "masks3", "labels3", "three", extra + ["--ignored", "unknown"])
    _check(report, setup["want3"], False)
    probs, labels3 = setup["arrays3"]
    hist, bad, ignored = P.histogram(probs[None, :, :, 1], labels3[None], 3, 2, ignore=IGNORE)
    got = report["probability"]
    assert not bad.any() and (got["class"], got["pixels"], got["positives"], got["ignored"]) == ("building", int(hist.sum()), int(hist[0, 1].sum()),
                                                                                               int(ignored[0]))
    assert got["ignored"] == report["ignored"] == setup["want3"]["ignored"] and got["pixels"] == report["pixels"]
    want = P.scores(probs[None, :, :, 1], labels3[None], 3, 2, ignore=IGNORE)
    for key in ("ap", "auc", "brier", "at_half"):
        assert got[key] == want[key], key


@pytest.mark.parametrize("stitch", [[], ["--stitch"]], ids=["per_tile", "stitched"])
def test_without_ignored_pixels_the_flag_changes_nothing_but_its_key(setup, stitch):
    name = "known_" + ("stitched" if stitch else "per_tile")
    typed = ["--type", "building"] + TYPED + stitch
    plain, plain_rows = _run(setup, name, "masks", "known", "two", typed)
    flagged, flagged_rows = _run(setup, name + "_flagged", "masks", "known", "two", typed + ["--ignored", "unknown"])
    assert flagged.pop("ignored_as") == "unknown" and "ignored_as" not in plain
    assert flagged == plain and list(flagged) == list(plain) and flagged_rows == plain_rows
    assert plain["ignored"] == 0 and plain["boundary"]["shared"] > 0 and plain["objects"]["matched"] > 0
    want = setup["want_known"]
    assert [plain["boundary"][k] for k in ("predicted", "actual", "shared")] == want["boundary_stitched" if stitch else "boundary"]
