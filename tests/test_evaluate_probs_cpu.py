"""``rs evaluate --probs`` and ``rs masks --threshold`` without a GPU: ``probability_scores`` against the restatement on the raw
pixels (tests/prob_ref.py), exactly -- integers, or floats equal to ``float(Fraction)`` --, the threshold's round trip through JSON
and through ``>=``, the curve CSV, the refusals of the flags before any device is asked for, and the declarations of the two new
symbols."""

import argparse
import csv
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prob_ref as P  # noqa: E402

from robosat_amd import evaluate as H  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_KEYS = ["threshold_byte", "threshold", "tp", "fp", "fn", "tn", "precision", "recall", "f1", "iou"]


def _rasters(kind, n=1500, seed=0):
    """(probability bytes, labels of a binary dataset), at most 2 000 pixels: the pairwise AUC stays cheap."""

    rng = np.random.RandomState(seed)
    actual = (rng.rand(n) < 0.3).astype(np.uint8)
    if kind == "random":
        q = rng.randint(0, 256, size=n)
    elif kind == "informative":  # overlapping ranges: positives high, negatives low
        q = np.clip(np.where(actual == 1, rng.normal(170, 50, n), rng.normal(80, 50, n)), 0, 255)
    elif kind == "two_bytes":
        q = np.where(rng.rand(n) < 0.5 + 0.3 * actual, 254, 1)
    elif kind == "one_byte":
        q = np.full(n, 77)
    elif kind == "byte_zero":  # byte 0 on a third of the pixels, positives among them (the wrap of p == 1.0 is read as 0)
        q = np.where(rng.rand(n) < 0.33, 0, rng.randint(0, 256, size=n))
        assert ((q == 0) & (actual == 1)).any() and ((q == 0) & (actual == 0)).any()
    elif kind == "no_positives":
        q, actual = rng.randint(0, 256, size=n), np.zeros(n, dtype=np.uint8)
    elif kind == "no_negatives":
        q, actual = rng.randint(0, 256, size=n), np.ones(n, dtype=np.uint8)
    else:
        raise KeyError(kind)
    return q.astype(np.uint8), actual


def _pos_neg(q, actual, cls=1):
    hist, bad, _ = P.histogram(q[None, None], actual[None, None], 2, cls)
    assert not bad.any()
    return hist[0, 1].tolist(), hist[0, 0].tolist()


def _same_scores(got, want):
    for key in ("ap", "auc", "brier", "ece"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in ("best_f1", "best_iou", "at_half"):
        assert got[key] == want[key], (key, got[key], want[key])
        if got[key] is not None:
            assert list(got[key]) == POINT_KEYS
    assert len(got["calibration"]) == H.CALIBRATION_BINS == 10
    for b, (row, ref) in enumerate(zip(got["calibration"], want["calibration"])):
        assert list(row) == ["lo", "hi", "pixels", "confidence", "accuracy"]
        assert {k: row[k] for k in ("pixels", "confidence", "accuracy")} == ref, (b, row, ref)
        members = [q for q in range(256) if min(10 * q // 255, 9) == b]
        assert row["lo"] == float(P.LIN[members[0]]) and row["hi"] == float(P.LIN[members[-1]])


@pytest.mark.parametrize("kind", ["random", "informative", "two_bytes", "one_byte", "byte_zero", "no_positives", "no_negatives"])
def test_probability_scores_are_the_restatement_on_the_pixels(kind):
    q, actual = _rasters(kind, seed=len(kind))
    want = P.scores(q, actual, 2, 1)
    pos, neg = _pos_neg(q, actual)
    got = H.probability_scores(pos, neg)
    _same_scores(got, want)
    assert H.curve_rows(pos, neg) == want["curve"]
    assert H.brier_score(pos, neg) == want["brier"]
    json.dumps(got, allow_nan=False)
    if kind == "no_positives":
        assert got["ap"] is None and got["auc"] is None and got["at_half"]["recall"] is None and got["brier"] is not None
    elif kind == "no_negatives":
        assert got["auc"] is None and got["ap"] == 1.0
    else:
        assert got["ap"] is not None and got["auc"] is not None and got["best_f1"] is not None and got["best_iou"] is not None
    if kind == "one_byte":
        assert got["auc"] == 0.5 and got["best_iou"]["threshold_byte"] == 0  # every k up to 77 gives the same point: the smallest


def test_no_pixels_give_nones_and_a_report_without_nan():
    got = H.probability_report("parking", [0] * 256, [0] * 256, ignored=5)
    assert list(got) == ["class", "pixels", "positives", "ignored", "ap", "auc", "brier", "ece", "calibration", "best_f1", "best_iou", "at_half"]
    assert (got["class"], got["pixels"], got["positives"], got["ignored"]) == ("parking", 0, 0, 5)
    assert got["ap"] is None and got["auc"] is None and got["brier"] is None and got["ece"] is None
    assert got["best_f1"] is None and got["best_iou"] is None
    assert all(got["at_half"][k] is None for k in ("precision", "recall", "f1", "iou"))
    assert all(row["pixels"] == 0 and row["confidence"] is None and row["accuracy"] is None for row in got["calibration"])
    text = json.dumps(H.build_report(["background", "parking"], [[0, 0], [0, 0]], 0, 0, probability=got), allow_nan=False)
    assert "NaN" not in text and list(json.loads(text))[-1] == "probability"
    assert "ignored" not in H.probability_report("parking", [0] * 256, [0] * 256)
    want = P.scores(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), 2, 1)
    _same_scores(got, want)


def test_on_a_tie_for_the_best_point_the_smallest_k_wins():
    """Positives at bytes 100 and 200, one negative at 150: k <= 100 gives IoU 2/3 (tp 2, fp 1), 101..150 gives 1/2, 151..200 gives
    1/2, above 0.  F1: 4/5, 2/3, 2/3.  So the best of both is k = 0, the smallest of 0..100.  With the negative at 50: k = 51..100 give
    IoU 1; the smallest is 51."""

    pos, neg = [0] * 256, [0] * 256
    pos[100] = pos[200] = 1
    neg[150] = 1
    got = H.probability_scores(pos, neg)
    assert got["best_iou"]["threshold_byte"] == 0 and got["best_iou"]["iou"] == 2 / 3
    assert got["best_f1"]["threshold_byte"] == 0 and got["best_f1"]["f1"] == 4 / 5
    neg[150], neg[50] = 0, 1
    got = H.probability_scores(pos, neg)
    assert got["best_iou"]["threshold_byte"] == 51 and got["best_iou"]["iou"] == 1.0 and got["best_f1"]["threshold_byte"] == 51
    assert got["auc"] == 1.0 and got["ap"] == 1.0
    # equal as fractions where the floats could differ: 1/3 at two points with other integers (1/3 and 2/6)
    pos, neg = [0] * 256, [0] * 256
    pos[10], pos[20], neg[20], neg[10] = 1, 1, 2, 2  # k <= 10: 2 / 6; k in 11..20: 1 / (1 + 2 + 1) = 1/4
    assert H.probability_scores(pos, neg)["best_iou"]["threshold_byte"] == 0


def test_at_half_of_a_binary_raster_is_the_confusion_matrix_of_the_soft_vote():
    from robosat_amd.tools.masks import softvote

    q, actual = _rasters("informative", seed=3)
    q[:4] = [127, 128, 127, 128]  # both sides of the argmax's cut, under both labels
    actual[:4] = [0, 0, 1, 1]
    foreground = P.LIN[q]
    voted = softvote(np.stack([1.0 - foreground, foreground])[None], axis=0)  # [K = 1][2][n]: averaged over the models, argmax over the classes
    assert voted.shape == q.shape and (voted == (q >= 128)).all()
    at_half = H.probability_scores(*_pos_neg(q, actual))["at_half"]
    matrix = np.bincount(actual.astype(np.int64) * 2 + voted, minlength=4).reshape(2, 2)  # M[actual][predicted]
    assert (at_half["tn"], at_half["fp"], at_half["fn"], at_half["tp"]) == tuple(int(v) for v in matrix.reshape(-1))
    assert at_half["threshold_byte"] == 128


def test_the_threshold_survives_json_bit_for_bit_and_cuts_where_its_byte_does():
    rows = H.curve_rows([1] * 256, [1] * 256)
    thresholds = np.array([row["threshold"] for row in rows])
    assert thresholds.tobytes() == P.LIN.tobytes()  # the anchors themselves
    back = np.array(json.loads(json.dumps([row["threshold"] for row in rows])))
    assert back.tobytes() == P.LIN.tobytes()
    assert ((P.LIN[:, None] >= back[None, :]) == (np.arange(256)[:, None] >= np.arange(256)[None, :])).all()  # all 256 x 256 pairs
    best = H.probability_scores([1] * 256, [1] * 256)["best_iou"]
    assert json.loads(json.dumps(best))["threshold"] == float(P.LIN[best["threshold_byte"]])


def test_the_curve_csv_reads_back(tmp_path):
    q, actual = _rasters("no_positives", seed=2)
    q[q < 40] = 40  # (k <= 40: everything predicted; above the top byte nothing: empty precision fields)
    pos, neg = _pos_neg(q, actual)
    rows = H.curve_rows(pos, neg)
    path = str(tmp_path / "curve.csv")
    H.write_curve_rows(path, rows)
    with open(path, newline="") as fp:
        read = list(csv.reader(fp))
    assert read[0] == POINT_KEYS and len(read) == 257
    for line, row in zip(read[1:], rows):
        for field, key in zip(line, POINT_KEYS):
            if row[key] is None:
                assert field == ""
            elif isinstance(row[key], int):
                assert int(field) == row[key]
            else:
                assert float(field) == row[key]
    assert read[1][POINT_KEYS.index("recall")] == "" and all(line[POINT_KEYS.index("recall")] == "" for line in read[1:])


def test_tile_rows_carry_brier_last_and_keep_their_order(tmp_path):
    from robosat_amd.tiles import Tile

    classes = ["background", "parking"]
    tiles = [Tile(1, 1, 18), Tile(2, 1, 18)]
    matrices = [[[5, 0], [0, 5]], [[5, 3], [2, 0]]]
    plain = H.tile_rows(tiles, matrices, classes)
    rows = H.tile_rows(tiles, matrices, classes, brier=[0.25, None])
    assert [(r["x"], r["y"]) for r in rows] == [(r["x"], r["y"]) for r in plain] == [(2, 1), (1, 1)]
    assert [r["brier"] for r in rows] == [None, 0.25] and "brier" not in plain[0]
    assert H.tile_columns(classes, brier=True) == H.tile_columns(classes) + ["brier"]
    H.write_tile_rows(str(tmp_path / "t.csv"), rows, classes, brier=True)
    with open(str(tmp_path / "t.csv"), newline="") as fp:
        read = list(csv.reader(fp))
    assert read[0][-1] == "brier" and read[1][-1] == "" and float(read[2][-1]) == 0.25
    H.write_tile_rows(str(tmp_path / "p.csv"), plain, classes)
    with open(str(tmp_path / "p.csv"), newline="") as fp:
        assert "brier" not in next(csv.reader(fp))


# ---- the flags ---------------------------------------------------------------------------------------------------------------
def _parser(name):
    import importlib

    tool = importlib.import_module("robosat_amd.tools." + name)
    parser = argparse.ArgumentParser()
    tool.add_parser(parser.add_subparsers())
    return parser, tool


def _write(path, image, mode, palette=None):
    from robosat_amd import png

    os.makedirs(os.path.dirname(path), exist_ok=True)
    png.write_png(path, image, mode, palette)


def _evaluate_dirs(tmp_path, classes):
    from robosat_amd.colors import make_palette

    colors = ["denim", "orange", "green"][:len(classes)]
    os.makedirs(str(tmp_path), exist_ok=True)
    dataset = tmp_path / "dataset.toml"
    dataset.write_text("[common]\nclasses = {}\ncolors = {}\n".format(json.dumps(classes), json.dumps(colors)))
    for name in ("masks", "labels", "probs"):
        _write(str(tmp_path / name / "18" / "5" / "7.png"), np.zeros((8, 6), dtype=np.uint8), "P", make_palette(*colors))
    return ["evaluate", str(tmp_path / "masks"), str(tmp_path / "labels"), "--dataset", str(dataset), str(tmp_path / "report.json")]


def _refused(tool, args, monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flags are checked before the device is"))
    with pytest.raises(SystemExit) as exc:
        tool.main(args)
    assert isinstance(exc.value.code, str) and exc.value.code.startswith("Error:")
    return exc.value.code


def test_evaluate_refuses_curve_without_probs(tmp_path, monkeypatch):
    parser, tool = _parser("evaluate")
    message = _refused(tool, parser.parse_args(_evaluate_dirs(tmp_path, ["background", "parking"]) + ["--curve", "c.csv"]), monkeypatch)
    assert "--curve" in message and "--probs" in message


def test_evaluate_refuses_probs_that_is_no_directory(tmp_path, monkeypatch):
    parser, tool = _parser("evaluate")
    base = _evaluate_dirs(tmp_path, ["background", "parking"])
    message = _refused(tool, parser.parse_args(base + ["--probs", str(tmp_path / "nowhere")]), monkeypatch)
    assert "nowhere is not a directory" in message


def test_evaluate_refuses_probs_on_a_multi_class_dataset_without_type(tmp_path, monkeypatch):
    parser, tool = _parser("evaluate")
    base = _evaluate_dirs(tmp_path, ["background", "parking", "building"])
    message = _refused(tool, parser.parse_args(base + ["--probs", str(tmp_path / "probs")]), monkeypatch)
    assert "--probs" in message and "--type" in message and "parking, building" in message and "3 classes" in message


def test_evaluate_with_good_probs_flags_goes_on_to_ask_for_the_device(tmp_path, monkeypatch):
    import torch

    parser, tool = _parser("evaluate")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for sub, classes, extra in (("a", ["background", "parking"], []), ("b", ["background", "parking", "building"], ["--type", "building"])):
        base = _evaluate_dirs(tmp_path / sub, classes)
        with pytest.raises(SystemExit) as exc:
            tool.main(parser.parse_args(base + ["--probs", str(tmp_path / sub / "probs"), "--curve", str(tmp_path / "c.csv")] + extra))
        assert exc.value.code == "Error: this build computes on the MI355X only"
    args = parser.parse_args(_evaluate_dirs(tmp_path / "c", ["background", "parking"]))
    assert args.probs is None and args.curve is None
    help_text = " ".join(parser._subparsers._group_actions[0].choices["evaluate"].format_help().split())
    assert "multi-class dataset with ignored pixels has no probability view yet" in help_text


def _masks_dirs(tmp_path, mode):
    from robosat_amd.colors import continuous_palette_for_color

    shape = (8, 6) if mode == "P" else (8, 6, 3)
    _write(str(tmp_path / "probs" / "18" / "5" / "7.png"), np.full(shape, 9, dtype=np.uint8), mode,
           continuous_palette_for_color("pink", 256) if mode == "P" else None)
    return ["masks", str(tmp_path / "out"), str(tmp_path / "probs")]


@pytest.mark.parametrize("value", ["0", "-0.5", "1.5", "nan"])
def test_masks_refuses_a_threshold_that_is_no_probability(tmp_path, monkeypatch, value):
    parser, tool = _parser("masks")
    message = _refused(tool, parser.parse_args(_masks_dirs(tmp_path, "P") + ["--threshold", value]), monkeypatch)
    assert "--threshold" in message and "0 < T <= 1" in message


def test_masks_refuses_a_threshold_on_tiles_with_more_than_one_channel(tmp_path, monkeypatch):
    parser, tool = _parser("masks")
    message = _refused(tool, parser.parse_args(_masks_dirs(tmp_path, "RGB") + ["--threshold", "0.5"]), monkeypatch)
    assert "--threshold" in message and "binary" in message and "4 classes" in message and "7.png" in message


def test_masks_with_a_good_threshold_goes_on_to_ask_for_the_device(tmp_path, monkeypatch):
    import torch

    parser, tool = _parser("masks")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for value in ("1", "0.00392156862745098"):
        with pytest.raises(SystemExit) as exc:
            tool.main(parser.parse_args(_masks_dirs(tmp_path / value, "P") + ["--threshold", value]))
        assert exc.value.code == "Error: this build computes on the MI355X only"
    assert parser.parse_args(_masks_dirs(tmp_path / "none", "P")).threshold is None


# ---- entry points ------------------------------------------------------------------------------------------------------------
C_TYPES = {"const uint8_t*": "P", "const double*": "P", "uint8_t*": "P", "int64_t*": "P", "rs_stream_t": "P", "long": "c_long",
           "int": "c_int"}


def test_the_header_declares_the_two_symbols_with_the_signatures_of_the_binding():
    import ctypes

    from robosat_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    kinds = {"P": ctypes.c_void_p, "c_long": ctypes.c_long, "c_int": ctypes.c_int}
    for name in ("rs_eval_prob_hist", "rs_softvote_masks_threshold"):
        found = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert found, name
        params = [" ".join(p.split()) for p in found.group(1).split(",")]
        declared = [kinds[C_TYPES[p.rsplit(" ", 1)[0]]] for p in params]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and list(argtypes) == declared, (name, params)
    found = re.search(r"\bint rs_eval_prob_hist\(([^)]*)\);", header).group(1)
    assert [p.split()[-1] for p in found.split(",")] == ["prob", "actual", "hist", "skipped", "pixels", "group", "C", "cls", "ignore", "stream"]
    found = re.search(r"\bint rs_softvote_masks_threshold\(([^)]*)\);", header).group(1)
    assert [p.split()[-1] for p in found.split(",")] == ["q", "weights", "anchors", "out", "K", "P", "threshold", "stream"]
    assert "Byte 0 is read as probability 0" in header  # (said where the bytes are defined)
    assert _lib.ABI_VERSION == 24  # (new symbols, no old one changed)
    assert callable(ops.prob_histogram)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librobosat_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    for name in ("rs_eval_prob_hist", "rs_softvote_masks_threshold"):
        assert hasattr(_lib.lib(), name)


def test_the_arguments_of_prob_histogram_and_of_the_threshold_are_checked_on_the_host():
    import torch

    from robosat_amd import ops

    a = torch.zeros((1, 2, 2), dtype=torch.uint8)
    for bad in (dict(classes=1, cls=1), dict(classes=9, cls=1), dict(classes=2, cls=0), dict(classes=2, cls=2), dict(classes=3, cls=True),
                dict(classes=2, cls=1, ignore=1), dict(classes=2, cls=1, ignore=256)):
        with pytest.raises(ValueError):
            ops.prob_histogram(a, a, **bad)
    with pytest.raises(ValueError):
        ops.prob_histogram(a, torch.zeros((1, 2, 3), dtype=torch.uint8), 2, 1)
    with pytest.raises(ValueError):
        ops.softvote_masks(torch.zeros((1, 4, 2), dtype=torch.uint8), threshold=0.5)  # two foreground channels
    for t in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.softvote_masks(torch.zeros((1, 4), dtype=torch.uint8), threshold=t)
