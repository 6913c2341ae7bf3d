"""``./rs evaluate --probs`` and ``./rs masks --threshold`` end to end on the MI355X, on synthetic probability tiles and labels
(four 64 x 64 tiles written with ``robosat_amd.png``; both classes present, the bytes of positives and negatives overlapping),
against the restatement on the raw pixels (tests/prob_ref.py).  Every comparison is exact: integers, or floats equal to
``float(Fraction)``."""

import csv
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prob_ref as P  # noqa: E402

from robosat_amd import png  # noqa: E402
from robosat_amd.colors import continuous_palette_for_color, make_palette  # noqa: E402

pytestmark = pytest.mark.gpu

Z, X0, Y0, SIZE = 18, 69623, 104945, 64
KEYS = [(X0, Y0), (X0, Y0 + 1), (X0 + 1, Y0), (X0 + 1, Y0 + 1)]  # the order tiles_from_slippy_map lists them in is not relied on
POINT_KEYS = ["threshold_byte", "threshold", "tp", "fp", "fn", "tn", "precision", "recall", "f1", "iou"]
GREYS = continuous_palette_for_color("pink", 256)  # 256 entries: a label tile may hold the byte 255


def _rs(args):
    """``./rs`` with these arguments, through the entry point's own parser, in this process (a process per call costs seconds)."""

    from robosat_amd.tools import __main__ as entry

    argv, sys.argv = sys.argv, ["./rs"] + list(args)
    try:
        entry.main()
    finally:
        sys.argv = argv


def _write(root, tiles, mode, palette=None):
    for (x, y), image in tiles.items():
        os.makedirs(os.path.join(root, str(Z), str(x)), exist_ok=True)
        png.write_png(os.path.join(root, str(Z), str(x), str(y) + ".png"), image, mode, palette)
    return root


def _read(root):
    from PIL import Image

    return {key: np.array(Image.open(os.path.join(root, str(Z), str(key[0]), str(key[1]) + ".png"))) for key in KEYS}


def _labels_and_bytes(seed, classes=2):
    """Per tile a label raster of rectangles and, per non-background class, probability bytes: high inside the class, low outside,
    with noise wide enough for the two ranges to overlap, and bytes 0 and 255 present."""

    rng = np.random.RandomState(seed)
    labels, probs = {}, {}
    for i, key in enumerate(KEYS):
        label = np.zeros((SIZE, SIZE), dtype=np.uint8)
        for c in range(1, classes):
            y, x = rng.randint(0, SIZE - 20, size=2)
            label[y:y + 12 + 4 * i, x:x + 20] = c
        planes = []
        for c in range(1, classes):
            centre = np.where(label == c, 165.0, 70.0 + 10 * c)
            planes.append(np.clip(np.rint(centre + rng.normal(0, 55, size=label.shape)), 0, 255).astype(np.uint8))
        labels[key], probs[key] = label, np.stack(planes, axis=-1)
    return labels, probs


def _stack(tiles):
    return np.stack([tiles[key] for key in KEYS])


def _evaluate(tmp, name, masks, labels, dataset, extra):
    out = str(tmp / (name + ".json"))
    _rs(["evaluate", masks, labels, "--dataset", dataset, out] + extra)
    with open(out) as fp:
        return json.load(fp)


def _csv(path):
    with open(path, newline="") as fp:
        return list(csv.reader(fp))


def _same_probability(got, want, kind, ignored=None):
    assert list(got) == ["class", "pixels", "positives"] + (["ignored"] if ignored is not None else []) + [
        "ap", "auc", "brier", "ece", "calibration", "best_f1", "best_iou", "at_half"]
    assert (got["class"], got["pixels"], got["positives"]) == (kind, want["pixels"], want["positives"])
    if ignored is not None:
        assert got["ignored"] == ignored == want["ignored"]
    for key in ("ap", "auc", "brier", "ece", "best_f1", "best_iou", "at_half"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert [{k: row[k] for k in ("pixels", "confidence", "accuracy")} for row in got["calibration"]] == want["calibration"]


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("evaluate_probs")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking"]\ncolors = ["denim", "orange"]\n')
    labels, probs = _labels_and_bytes(1)
    want = P.scores(_stack(probs)[..., 0], _stack(labels), 2, 1)
    # the reference first: every score the round trip relies on is defined, and the best point is not the argmax's
    assert want["ap"] is not None and want["auc"] is not None and want["best_f1"] is not None and want["best_iou"] is not None
    assert 0 < want["positives"] < want["pixels"] and want["best_iou"]["threshold_byte"] != 128
    assert want["best_iou"]["iou"] > want["at_half"]["iou"]
    assert (_stack(probs) == 0).any() and (_stack(probs) == 255).any()
    return {"tmp": tmp, "dataset": str(dataset), "want": want, "label_tiles": labels, "prob_tiles": probs,
            "labels": _write(str(tmp / "labels"), labels, "P", make_palette("denim", "orange")),
            "probs": _write(str(tmp / "probs"), {k: v[..., 0] for k, v in probs.items()}, "P", GREYS)}


def test_probs_curve_and_tiles_are_the_restatement_and_the_threshold_makes_the_round_trip(binary):
    s, tmp, want = binary, binary["tmp"], binary["want"]
    masks = str(tmp / "masks")
    _rs(["masks", masks, s["probs"], "--dataset", s["dataset"]])
    curve, tiles = str(tmp / "curve.csv"), str(tmp / "tiles.csv")
    report = _evaluate(tmp, "report", masks, s["labels"], s["dataset"], ["--probs", s["probs"], "--curve", curve, "--tiles", tiles])
    assert list(report)[-1] == "probability"
    _same_probability(report["probability"], want, "parking")

    # the curve: the 256 points of the restatement
    read = _csv(curve)
    assert read[0] == POINT_KEYS and len(read) == 257
    for line, point in zip(read[1:], want["curve"]):
        got = {k: (None if f == "" else int(f) if k in ("threshold_byte", "tp", "fp", "fn", "tn") else float(f)) for k, f in zip(POINT_KEYS, line)}
        assert got == point

    # at_half is the argmax rs masks took: the report's own confusion matrix M[actual][predicted]
    half = report["probability"]["at_half"]
    assert [[half["tn"], half["fp"]], [half["fn"], half["tp"]]] == report["confusion"]

    # --tiles: the existing columns, then the tile's own Brier score
    rows = _csv(tiles)
    assert rows[0] == ["z", "x", "y", "pixels", "iou_background", "iou_parking", "miou", "predicted_share", "actual_share", "brier"]
    briers = {(int(r[1]), int(r[2])): float(r[-1]) for r in rows[1:]}
    assert briers == {key: P.brier(s["prob_tiles"][key][..., 0].reshape(-1), s["label_tiles"][key].reshape(-1) == 1) for key in KEYS}
    assert [float(r[6]) for r in rows[1:]] == sorted(float(r[6]) for r in rows[1:])  # still worst miou first

    # the round trip: the best threshold, read from the JSON, applied by rs masks, evaluated as a mask
    best = report["probability"]["best_iou"]
    cut = str(tmp / "masks_cut")
    _rs(["masks", cut, s["probs"], "--dataset", s["dataset"], "--threshold", repr(best["threshold"])])
    k = best["threshold_byte"]
    for key, mask in _read(cut).items():
        assert (mask == (s["prob_tiles"][key][..., 0] >= k)).all()
    again = _evaluate(tmp, "cut", cut, s["labels"], s["dataset"], [])
    assert again["confusion"] == [[best["tn"], best["fp"]], [best["fn"], best["tp"]]]
    assert again["iou"]["parking"] == best["iou"] and "probability" not in again


def test_without_probs_the_report_and_the_tile_list_are_what_they_were(binary):
    s, tmp = binary, binary["tmp"]
    masks = str(tmp / "masks_plain")
    _rs(["masks", masks, s["probs"], "--dataset", s["dataset"]])
    tiles = str(tmp / "tiles_plain.csv")
    plain = _evaluate(tmp, "plain", masks, s["labels"], s["dataset"], ["--tiles", tiles])
    assert list(plain) == ["classes", "tiles", "tiles_without_label", "pixels", "confusion", "iou", "miou", "fg_iou", "mcc", "accuracy"]
    assert _csv(tiles)[0] == ["z", "x", "y", "pixels", "iou_background", "iou_parking", "miou", "predicted_share", "actual_share"]
    with_probs = _evaluate(tmp, "with", masks, s["labels"], s["dataset"], ["--probs", s["probs"]])
    assert {k: v for k, v in with_probs.items() if k != "probability"} == plain


def test_with_an_ignore_label_the_ignored_pixels_are_in_no_count(binary):
    s, tmp = binary, binary["tmp"]
    dataset = tmp / "dataset_ignore.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking"]\ncolors = ["denim", "orange"]\nignore = 255\n')
    labels = {key: tile.copy() for key, tile in s["label_tiles"].items()}
    for i, key in enumerate(KEYS):
        labels[key][:, :8 + 4 * i] = 255  # a strip of every tile, over background and parking alike
    want = P.scores(_stack(s["prob_tiles"])[..., 0], _stack(labels), 2, 1, ignore=255)
    assert want["ignored"] == 64 * (8 + 12 + 16 + 20) and want["ap"] is not None and want["auc"] is not None
    labels_dir = _write(str(tmp / "labels_ignore"), labels, "P", GREYS)
    masks = str(tmp / "masks_ignore")
    _rs(["masks", masks, s["probs"], "--dataset", s["dataset"]])
    report = _evaluate(tmp, "ignore", masks, labels_dir, str(dataset), ["--probs", s["probs"]])
    _same_probability(report["probability"], want, "parking", ignored=report["ignored"])
    half = report["probability"]["at_half"]
    assert [[half["tn"], half["fp"]], [half["fn"], half["tp"]]] == report["confusion"]
    assert report["probability"]["pixels"] == report["pixels"] == 4 * SIZE * SIZE - want["ignored"]


def test_with_type_the_plane_of_that_class_is_read_from_rgb_tiles(tmp_path):
    """RGB probability tiles hold three planes, the non-background classes of a dataset of four; ``--type`` picks the plane
    ``class index - 1`` and counts the labels of that class as the positives."""

    classes = ["background", "parking", "building", "road"]
    dataset = tmp_path / "dataset.toml"
    dataset.write_text('[common]\nclasses = {}\ncolors = ["denim", "orange", "green", "purple"]\n'.format(json.dumps(classes)))
    labels, probs = _labels_and_bytes(2, classes=4)
    labels_dir = _write(str(tmp_path / "labels"), labels, "P", make_palette("denim", "orange", "green", "purple"))
    probs_dir = _write(str(tmp_path / "probs"), probs, "RGB")
    masks = str(tmp_path / "masks")
    _rs(["masks", masks, probs_dir, "--dataset", str(dataset)])
    seen = []
    for kind in ("building", "road"):
        index = classes.index(kind)
        want = P.scores(_stack(probs)[..., index - 1], _stack(labels), 4, index)
        assert want["ap"] is not None and want["auc"] is not None and want["best_iou"] is not None
        report = _evaluate(tmp_path, kind, masks, labels_dir, str(dataset), ["--type", kind, "--probs", probs_dir])
        _same_probability(report["probability"], want, kind)
        seen.append(report["probability"]["auc"])
    assert seen[0] != seen[1]  # (the two planes are not taken for each other)
    # a mask tile without a probability tile ends the run and names the tile
    os.remove(os.path.join(probs_dir, str(Z), str(KEYS[2][0]), str(KEYS[2][1]) + ".png"))
    with pytest.raises(SystemExit) as exc:
        _rs(["evaluate", masks, labels_dir, "--dataset", str(dataset), str(tmp_path / "missing.json"), "--type", "road", "--probs", probs_dir])
    assert exc.value.code.startswith("Error: --probs ") and "has no probabilities for the mask tile {}/{}/{}".format(Z, *KEYS[2]) in exc.value.code
