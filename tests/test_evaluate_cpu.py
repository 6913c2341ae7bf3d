"""``rs evaluate`` without a GPU: the entry points are declared and exported, the boundary band against the brute-force distance
transform, ``match_objects`` against brute-force matching over label rasters, the scores against ``Metrics`` and the reference's
expressions, the report and the per-tile list, and the validation of the flags in ``main``, which rejects them before it asks for a
device."""

import argparse
import csv
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edt_ref as E  # noqa: E402
import eval_ref as V  # noqa: E402
import features_ref as R  # noqa: E402

from robosat_amd import evaluate as H  # noqa: E402
from robosat_amd.tiles import Tile  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- entry points ------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_in_the_header_and_exported_by_the_library():
    from robosat_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    assert re.search(r"\bint rs_eval_confusion\(const uint8_t\* predicted, const uint8_t\* actual, int64_t\* counts, int64_t\* bad, "
                     r"long pixels, long group, int C,\s+rs_stream_t stream\);", header)
    assert re.search(r"\bint rs_eval_boundary\(const int32_t\* d2_a, const int32_t\* d2_b, int64_t\* counts, long pixels, long group, "
                     r"int D, rs_stream_t stream\);", header)
    assert re.search(r"\bint rs_eval_config\(int\* block_pixels\);", header)
    assert "raster edge is NOT a boundary" in header  # (the departure from the paper's code is stated where the band is defined)
    for name, count in (("rs_eval_confusion", 8), ("rs_eval_boundary", 7), ("rs_eval_config", 1)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == count
    assert _lib.ABI_VERSION == 24  # (new symbols, no old one changed)
    assert callable(ops.mask_confusion) and callable(ops.boundary_counts) and callable(ops.eval_config)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librobosat_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    for name in ("rs_eval_confusion", "rs_eval_boundary", "rs_eval_config"):
        assert hasattr(_lib.lib(), name)
    assert ops.eval_config() == 4096


def test_the_tool_is_registered():
    from robosat_amd.tools import __main__ as entry

    assert "evaluate.add_parser(subparser)" in open(entry.__file__).read() and "``rs evaluate``" in entry.__doc__


# ---- the band ----------------------------------------------------------------------------------------------------------------
def _band_by_definition(mask, d):
    """The set pixels with an unset pixel of the raster within d, centre to centre: every pair of pixels."""

    mask = np.asarray(mask, dtype=bool)
    ys, xs = np.nonzero(~mask)
    out = np.zeros(mask.shape, dtype=bool)
    for y, x in zip(*np.nonzero(mask)):
        out[y, x] = bool(len(ys)) and int(((ys - y) ** 2 + (xs - x) ** 2).min()) <= d * d
    return out


@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("name", ["blobs", "comb", "nested", "all_set"])
def test_the_band_is_what_the_brute_force_transform_gives(name, d):
    mask = {"blobs": R.blobs(20, 23, 3), "comb": R.comb(15), "nested": R.nested(), "all_set": np.ones((9, 11), dtype=bool)}[name]
    got = V.band(mask, d)
    brute = E.edt_brute(mask, d + 1)
    assert (got == ((brute >= 1) & (brute <= d * d))).all()
    assert (got == _band_by_definition(mask, d)).all()
    assert not (got & ~mask).any()
    if name == "all_set":
        assert not got.any()  # no unset pixel, no boundary: the raster's edge is not one
    else:
        assert got.any()


def test_the_raster_edge_is_not_in_the_band():
    mask = np.zeros((12, 12), dtype=bool)
    mask[:6, :] = True  # touches the top, left and right edges; its boundary is the row y = 5
    got = V.band(mask, 1)
    assert got[5].all() and not got[:5].any() and int(got.sum()) == 12


# ---- match_objects -----------------------------------------------------------------------------------------------------------
def _tables(labels, min_area=0):
    return np.concatenate([R.table(plane, min_area, tile=i) for i, plane in enumerate(labels)]).reshape(-1, 7)


def _pair_of_blob_rasters():
    """Two tiles; the actual side is the predicted one moved by a few pixels, except the left 30 columns of tile 0, which are the
    same on both sides (so some pairs reach IoU 1)."""

    p = np.stack([R.blobs(48, 70, 1), R.blobs(48, 70, 2)])
    g = np.stack([np.roll(p[0], (2, 3), axis=(0, 1)), np.roll(p[1], (-1, 4), axis=(0, 1))])
    g[0, :, :30] = p[0, :, :30]
    g[0, :, 30] = False  # (cut: what is equal stays equal as an object)
    p = p.copy()
    p[0, :, 30] = False
    return np.stack([R.label(m) for m in p]), np.stack([R.label(m) for m in g])


@pytest.mark.parametrize("threshold", [0.3, 0.5, 0.75, 1.0])
def test_match_objects_is_the_brute_force_matching(threshold):
    labels_p, labels_g = _pair_of_blob_rasters()
    want = V.match(labels_p, labels_g, threshold)
    got = H.match_objects(_tables(labels_p), _tables(labels_g), V.overlap_rows(labels_p, labels_g), threshold, stitched=False)
    assert got[:3] == want[:3] and got[3] == [float(v) for v in want[3]]
    assert want[1] > 10 and want[2] > 10 and 0 < want[0] < min(want[1], want[2])  # (the case shows something at every threshold)
    if threshold == 1.0:
        assert all(v == 1 for v in want[3])


def test_stitched_tables_match_like_one_raster():
    labels_p, labels_g = _pair_of_blob_rasters()
    want = V.match(labels_p[:1], labels_g[:1], 0.5)
    got = H.match_objects(_tables(labels_p[:1])[:, 1:], _tables(labels_g[:1])[:, 1:], V.overlap_rows(labels_p[:1], labels_g[:1]), 0.5,
                          stitched=True)
    assert got[:3] == want[:3] and got[3] == [float(v) for v in want[3]]


def test_a_tie_at_exactly_one_half_goes_to_the_smaller_keys():
    """A 4-pixel object over two 2-pixel objects: IoU 2 / (4 + 2 - 2) = 1/2 twice.  The two small objects are labels of their own
    although they touch (as the instances of ``--split`` do): the labels are taken as they are.  One match, with the smaller actual key;
    with the sides swapped the smaller predicted key."""

    big = np.array([[[0, 2, 2, 2, 2, 0]]], dtype=np.int32)
    small = np.array([[[0, 2, 2, 4, 4, 0]]], dtype=np.int32)
    pairs = V.overlap_rows(big, small)
    assert pairs.tolist() == [[0, 2, 2, 2], [0, 2, 4, 2]]
    got = H.match_objects(_tables(big), _tables(small), pairs, 0.5, stitched=False)
    assert got == (1, 1, 2, [0.5]) and got == tuple(V.match(big, small, 0.5)[:3]) + ([0.5],)
    swapped = H.match_objects(_tables(small), _tables(big), V.overlap_rows(small, big), 0.5, stitched=False)
    assert swapped == (1, 2, 1, [0.5])
    # which pair it was: with the first small object out of the way (its row dropped) the second takes the match
    assert H.match_objects(_tables(big), _tables(small)[1:], pairs, 0.5, stitched=False) == (1, 1, 1, [0.5])
    # just above one half neither pair matches
    assert H.match_objects(_tables(big), _tables(small), pairs, 0.5000001, stitched=False) == (0, 1, 2, [])
    # the order of the rows does not decide
    assert H.match_objects(_tables(big), _tables(small)[::-1], pairs[::-1], 0.5, stitched=False) == (1, 1, 2, [0.5])


def test_thresholds_are_compared_in_integers():
    """3 shared pixels of a union of 10 is IoU 3/10; the float 0.3 is a little BELOW 3/10, so the pair matches at 0.3, and does not at
    the next float above 3/10."""

    p = np.zeros((1, 2, 8), dtype=np.int32)
    g = np.zeros((1, 2, 8), dtype=np.int32)
    p[0, 0, 0:6] = 1  # 6 pixels
    g[0, 0, 3:8] = 4
    g[0, 1, 3:5] = 4  # 7 pixels, 3 shared: union 10
    pairs = V.overlap_rows(p, g)
    assert pairs.tolist() == [[0, 1, 4, 3]]
    assert H.match_objects(_tables(p), _tables(g), pairs, 0.3, False)[0] == 1
    assert H.match_objects(_tables(p), _tables(g), pairs, float(np.nextafter(0.3, 1)), False)[0] == 0


def test_min_area_removes_one_side_of_a_pair():
    labels_p, labels_g = _pair_of_blob_rasters()
    areas = np.sort(_tables(labels_g)[:, 2])
    min_area = int(areas[len(areas) // 2]) + 1  # about half the actual objects go
    want = V.match(labels_p, labels_g, 0.3, min_area=min_area)
    table_p, table_g = _tables(labels_p, min_area), _tables(labels_g, min_area)
    pairs = V.overlap_rows(labels_p, labels_g)  # (the overlap table knows nothing of --min_area: its pairs name dropped components)
    assert len(table_g) < len(_tables(labels_g)) and len(pairs) > len(table_p)
    got = H.match_objects(table_p, table_g, pairs, 0.3, stitched=False)
    assert got[:3] == want[:3] and got[3] == [float(v) for v in want[3]] and want[0] > 0


def test_empty_tables():
    none7, none4 = np.zeros((0, 7), dtype=np.int32), np.zeros((0, 4), dtype=np.int32)
    assert H.match_objects(none7, none7, none4, 0.5, stitched=False) == (0, 0, 0, [])
    assert H.match_objects(np.zeros((0, 6)), np.zeros((0, 6)), none4, 0.5, stitched=True) == (0, 0, 0, [])
    labels_p, _ = _pair_of_blob_rasters()
    matched, predicted, actual, ious = H.match_objects(_tables(labels_p), none7, none4, 0.5, stitched=False)
    assert (matched, actual, ious) == (0, 0, []) and predicted == len(_tables(labels_p))
    scores = H.ObjectScores(0.5, 0, False)
    scores.add(none7, none7, none4)
    report = scores.report()
    assert report["precision"] is None and report["recall"] is None and report["f1"] is None and report["mean_matched_iou"] is None


# ---- scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_two_class_scores_are_what_metrics_and_the_reference_give(seed):
    from robosat_amd.metrics import Metrics

    rng = np.random.RandomState(seed)
    matrix = rng.randint(0, 10 ** rng.randint(1, 7), size=(2, 2))
    if seed == 5:
        matrix[1] = 0  # no foreground among the labels
    got = H.confusion_scores(matrix, ["background", "parking"])
    metrics = Metrics.from_confusion(["background", "parking"], matrix)
    assert (metrics.confusion_matrix() == matrix).all()
    assert got["miou"] == metrics.get_miou() and got["fg_iou"] == metrics.get_fg_iou()
    tn, fn, fp, tp = (int(v) for v in matrix.reshape(-1))  # (the reference's names: robosat/metrics.py)
    assert got["fg_iou"] == tp / (tp + fn + fp)
    assert got["miou"] == float(np.nanmean([tn / (tn + fn + fp), tp / (tp + fn + fp)]))
    if seed == 5:
        assert got["mcc"] is None and math.isnan(metrics.get_mcc())
    else:
        assert got["mcc"] == metrics.get_mcc() == (tp * tn - fp * fn) / math.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn))
    assert got["accuracy"] == (tn + tp) / (tn + fn + fp + tp)
    assert got["iou"] == {"background": tn / (tn + fn + fp), "parking": tp / (tp + fn + fp)}


def test_an_absent_class_is_null_and_left_out_of_the_mean():
    matrix = [[50, 0, 10], [0, 0, 0], [5, 0, 35]]  # class 1 neither occurs nor is predicted
    got = H.confusion_scores(matrix, ["background", "parking", "building"])
    assert got["iou"] == {"background": 50 / 65, "parking": None, "building": 35 / 50}
    assert got["miou"] == float(np.mean([50 / 65, 35 / 50])) and got["fg_iou"] is None
    assert got["accuracy"] == 85 / 100 and -1 <= got["mcc"] <= 1


def test_the_empty_matrix_has_no_scores():
    got = H.confusion_scores(np.zeros((3, 3), dtype=np.int64), ["a", "b", "c"])
    assert got == {"iou": {"a": None, "b": None, "c": None}, "miou": None, "fg_iou": None, "mcc": None, "accuracy": None}


# ---- report and per-tile list ------------------------------------------------------------------------------------------------
CLASSES = ["background", "parking", "building"]


def test_the_report_has_its_keys_and_is_json_without_nan():
    import json

    matrix = [[50, 0, 10], [0, 0, 0], [5, 0, 35]]
    plain = H.build_report(CLASSES, matrix, 3, 1)
    assert list(plain) == ["classes", "tiles", "tiles_without_label", "pixels", "confusion", "iou", "miou", "fg_iou", "mcc", "accuracy"]
    assert plain["pixels"] == 100 and plain["confusion"] == matrix and plain["tiles"] == 3 and plain["tiles_without_label"] == 1
    scores = H.ObjectScores(0.5, 4, True)
    scores.matched, scores.predicted, scores.actual, scores.ious = 2, 3, 4, [0.75, 0.5]
    full = H.build_report(CLASSES, matrix, 3, 1, kind="building", objects=scores.report(), boundary=H.boundary_report(3, [10, 12, 6]))
    assert list(full)[len(plain):] == ["type", "objects", "boundary"] and full["type"] == "building"
    assert full["objects"] == {"threshold": 0.5, "min_area": 4, "stitched": True, "predicted": 3, "actual": 4, "matched": 2,
                               "precision": 2 / 3, "recall": 2 / 4, "f1": 4 / 7, "mean_matched_iou": 0.625}
    assert full["boundary"] == {"d": 3, "predicted": 10, "actual": 12, "shared": 6, "iou": 6 / 16}
    assert H.boundary_report(1, [0, 0, 0])["iou"] is None
    text = json.dumps(full, allow_nan=False)
    assert "NaN" not in text and json.loads(text)["iou"]["parking"] is None


def test_the_tile_list_is_sorted_worst_first_with_undefined_values_last(tmp_path):
    tiles = [Tile(5, 7, 18), Tile(5, 6, 18), Tile(4, 9, 18), Tile(6, 1, 18), Tile(3, 3, 17)]
    matrices = [
        [[90, 0, 0], [0, 0, 0], [5, 0, 5]],    # building IoU 5 / 10
        [[100, 0, 0], [0, 0, 0], [0, 0, 0]],   # no building on either side: undefined
        [[60, 0, 30], [0, 0, 0], [10, 0, 0]],  # building IoU 0
        [[90, 0, 0], [0, 0, 0], [5, 0, 5]],    # 5 / 10 again: (z, x, y) decides
        [[0, 0, 0], [0, 0, 0], [0, 0, 100]],   # IoU 1
    ]
    rows = H.tile_rows(tiles, matrices, CLASSES, kind="building")
    assert [(r["z"], r["x"], r["y"]) for r in rows] == [(18, 4, 9), (18, 5, 7), (18, 6, 1), (17, 3, 3), (18, 5, 6)]
    assert [r["iou_building"] for r in rows] == [0.0, 0.5, 0.5, 1.0, None]
    assert rows[0]["predicted_share"] == 30 / 100 and rows[0]["actual_share"] == 10 / 100 and rows[0]["pixels"] == 100
    by_miou = H.tile_rows(tiles, matrices, CLASSES)
    assert [r["miou"] for r in by_miou] == sorted(r["miou"] for r in by_miou)  # (every tile has a miou here)
    assert (by_miou[0]["z"], by_miou[0]["x"], by_miou[0]["y"]) == (18, 4, 9)
    path = str(tmp_path / "tiles.csv")
    H.write_tile_rows(path, rows, CLASSES)
    with open(path, newline="") as fp:
        read = list(csv.reader(fp))
    assert read[0] == ["z", "x", "y", "pixels", "iou_background", "iou_parking", "iou_building", "miou", "predicted_share", "actual_share"]
    assert [line[:3] for line in read[1:]] == [["18", "4", "9"], ["18", "5", "7"], ["18", "6", "1"], ["17", "3", "3"], ["18", "5", "6"]]
    assert read[5][6] == "" and read[1][5] == "" and float(read[2][6]) == 0.5 and float(read[2][7]) == rows[1]["miou"]


# ---- the flags ---------------------------------------------------------------------------------------------------------------
def _parser():
    from robosat_amd.tools import evaluate as tool

    parser = argparse.ArgumentParser()
    tool.add_parser(parser.add_subparsers())
    return parser, tool


def _dirs(tmp_path):
    from robosat_amd import png
    from robosat_amd.colors import make_palette

    os.makedirs(str(tmp_path), exist_ok=True)
    dataset = tmp_path / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking", "building"]\ncolors = ["denim", "orange", "green"]\n')
    for name in ("masks", "labels"):
        os.makedirs(str(tmp_path / name / "18" / "5"))
        png.write_png(str(tmp_path / name / "18" / "5" / "7.png"), np.zeros((8, 6), dtype=np.uint8), "P", make_palette("denim", "orange", "green"))
    return ["evaluate", str(tmp_path / "masks"), str(tmp_path / "labels"), "--dataset", str(dataset), str(tmp_path / "report.json")]


def test_the_flags_parse_and_default_off(tmp_path):
    parser, _ = _parser()
    args = parser.parse_args(_dirs(tmp_path))
    assert args.type is None and args.boundary == 0 and args.match is None and args.min_area is None and not args.stitch
    assert args.tiles is None and args.batch_size == 16
    args = parser.parse_args(_dirs(tmp_path / "b") + ["--type", "building", "--boundary", "3", "--match", "0.75", "--min_area", "9", "--stitch",
                                                      "--tiles", "t.csv"])
    assert (args.type, args.boundary, args.match, args.min_area, args.stitch, args.tiles) == ("building", 3, 0.75, 9, True, "t.csv")
    help_text = parser._subparsers._group_actions[0].choices["evaluate"].format_help()
    assert "edge of the raster is not a" in " ".join(help_text.split()) and "counts once per tile" in " ".join(help_text.split())


@pytest.mark.parametrize("extra, words", [
    (["--boundary", "3"], ["--boundary", "--type"]),
    (["--match", "0.5"], ["--match", "--type"]),
    (["--min_area", "0"], ["--min_area", "--type"]),
    (["--stitch"], ["--stitch", "--type"]),
    (["--type", "background"], ["--type", "background", "parking, building"]),
    (["--type", "road"], ["--type", "road"]),
    (["--type", "building", "--boundary", "128"], ["--boundary", "128", "1..127"]),
    (["--type", "building", "--boundary", "-1"], ["--boundary", "-1"]),
    (["--type", "building", "--match", "0"], ["--match", "0 < T <= 1"]),
    (["--type", "building", "--match", "1.01"], ["--match", "1.01"]),
    (["--type", "building", "--match", "nan"], ["--match", "nan"]),
    (["--type", "building", "--min_area", "-3"], ["--min_area", "-3"]),
    (["--batch_size", "0"], ["--batch_size"]),
    (["--type", "building", "--stitch", "--boundary", "6"], ["--boundary 6", "7 pixels", "8x6", "at most 5"]),
])
def test_main_rejects_bad_flags_before_it_needs_a_device(tmp_path, monkeypatch, extra, words):
    import torch

    parser, tool = _parser()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flags are checked before the device is"))
    args = parser.parse_args(_dirs(tmp_path) + extra)
    with pytest.raises(SystemExit) as exc:
        tool.main(args)
    assert isinstance(exc.value.code, str) and exc.value.code.startswith("Error:")
    for word in words:
        assert word in exc.value.code, (word, exc.value.code)


@pytest.mark.parametrize("which", ["masks", "labels"])
def test_a_missing_directory_is_an_error_message(tmp_path, monkeypatch, which):
    import torch

    parser, tool = _parser()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flags are checked before the device is"))
    base = _dirs(tmp_path)
    base[1 if which == "masks" else 2] += "_nowhere"
    with pytest.raises(SystemExit) as exc:
        tool.main(parser.parse_args(base))
    assert exc.value.code.startswith("Error:") and "_nowhere is not a directory" in exc.value.code


@pytest.mark.parametrize("extra", [[], ["--type", "building", "--boundary", "5", "--match", "1", "--min_area", "2", "--stitch"],
                                   ["--type", "parking", "--boundary", "127"]], ids=["plain", "everything", "widest_band"])
def test_with_good_flags_main_goes_on_to_ask_for_the_device(tmp_path, monkeypatch, extra):
    import torch

    parser, tool = _parser()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as exc:
        tool.main(parser.parse_args(_dirs(tmp_path) + extra))
    assert exc.value.code == "Error: this build computes on the MI355X only"
