"""``rs evaluate --centerline`` without a GPU: the numpy reference's reach against the brute-force definition, the link rule at its
edges, ``centerline_report``, the per-tile columns, the validation of the flag in ``main`` before any device is asked for, and the
declaration and binding of ``rs_eval_centerline``."""

import argparse
import csv
import json
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import centerline_eval_ref as C  # noqa: E402
import stitch_ref as S  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import evaluate as H  # noqa: E402
from robosat_amd.tiles import Tile  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["background", "road"]


# ---- the entry point -----------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_in_the_header_and_bound():
    from robosat_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    assert re.search(r"\bint rs_eval_centerline\(const uint8_t\* skel_p, const uint8_t\* skel_g, const int32_t\* d2_to_g, "
                     r"const int32_t\* d2_to_p,\s+const int32_t\* nbr, int64_t\* counts, int B, int H, int W, int rho, "
                     r"rs_stream_t stream\);", header)
    assert "Wiedemann and Heipke" in header and "matching is judged at link ends" in " ".join(header.replace(" * ", " ").split())
    assert "rs_eval_centerline" in _lib.SIGNATURES and len(_lib.SIGNATURES["rs_eval_centerline"][1]) == 11
    assert _lib.ABI_VERSION == 24  # (a new symbol, no old one changed)
    assert callable(ops.centerline_counts) and ops.EVAL_MAX_RHO == ops.EDT_MAX_RADIUS - 1 == 127
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.lib(), "rs_eval_centerline")


# ---- the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, shape, rho", [(0, (24, 24), 1), (1, (24, 17), 3), (2, (9, 24), 5), (3, (24, 24), 23), (4, (1, 13), 2),
                                              (5, (11, 1), 4)])
def test_the_reach_is_the_brute_force_definition(seed, shape, rho):
    rng = np.random.RandomState(seed)
    skeleton = rng.rand(*shape) < 0.03
    assert (C.near(skeleton, rho) == C.near_brute(skeleton, rho)).all()
    roads = T.thin(T.roads(shape[0], shape[1], seed, count=2, width=3))
    assert (C.near(roads, rho) == C.near_brute(roads, rho)).all()
    assert not C.near(np.zeros(shape, dtype=bool), rho).any()  # (an empty skeleton is near nothing: every pixel is capped)


def test_the_stitched_reach_is_the_single_rasters_where_every_tile_is_there():
    skeleton = T.thin(T.roads(24, 24, 7, count=3, width=3))
    grid = S.Grid(S.split(skeleton, 8, 12), pad=4)
    got = grid.cut(C.near(grid.canvas, 5, grid.index >= 0))
    want = np.stack([C.near_brute(skeleton, 5)[r:r + 8, c:c + 12] for c in (0, 12) for r in (0, 8, 16)])  # slots: x, then y
    assert (got == want).all()


def test_the_link_rule_at_its_edges():
    def totals(rows):
        four = C.side_counts(np.array(rows), np.zeros(np.array(rows).shape, dtype=bool)).sum(axis=(1, 2))
        return int(four[0]), int(four[1])

    assert totals([[1, 1, 0], [0, 1, 1], [0, 0, 1]]) == (4, 0)          # a staircase: no diagonal where a detour exists
    assert totals([[1, 0, 0], [0, 1, 0], [0, 0, 1]]) == (0, 2)          # a pure diagonal
    assert totals([[1, 0, 1], [0, 1, 0], [1, 0, 1]]) == (0, 4)          # an X crossing
    assert totals([[0, 0, 0], [0, 1, 0], [0, 0, 0]]) == (0, 0)          # a lone pixel has no length
    assert totals([[0, 0, 1], [0, 0, 1], [1, 1, 1]]) == (4, 0)          # links in the last row and the last column
    assert totals([[0, 0, 1], [1, 0, 0]]) == (0, 0)                     # the row's last and the next row's first pixel: no link


def test_matching_needs_both_ends():
    p = np.zeros((9, 16), dtype=np.uint8)
    g = np.zeros((9, 16), dtype=np.uint8)
    p[4, 2:12] = 1          # nine E links
    g[0, 5] = 1             # one pixel four rows above column 5: within 5 of columns 2..8
    assert C.counts(p, g, 5) == [9, 0, 6, 0, 0, 0, 0, 0]  # ends 2..8 are near: the links 2-3 .. 7-8


# ---- the report ----------------------------------------------------------------------------------------------------------------
def test_identical_sides_score_one():
    report = H.centerline_report(3, [7, 2, 7, 2, 7, 2, 7, 2])
    assert (report["completeness"], report["correctness"], report["quality"], report["f1"]) == (1.0, 1.0, 1.0, 1.0)
    assert report["rho"] == 3 and report["predicted"] == report["actual"]


def test_an_empty_prediction_and_two_empty_sides():
    report = H.centerline_report(2, [0, 0, 0, 0, 5, 1, 0, 0])
    assert report["correctness"] is None and report["completeness"] == 0.0 and report["quality"] == 0.0 and report["f1"] is None
    report = H.centerline_report(2, [0] * 8)
    assert [report[k] for k in ("completeness", "correctness", "quality", "f1")] == [None] * 4
    assert "NaN" not in json.dumps(report, allow_nan=False)


def test_the_integers_pass_through_and_a_case_by_hand():
    big = 3 * 10 ** 12 + 1  # (Python integers: no bound)
    report = H.centerline_report(5, [big, 2, 2, 1, 4, 0, 2, 0])
    assert report["predicted"]["straight"] == big and isinstance(report["predicted"]["straight"], int)
    report = H.centerline_report(5, [3, 2, 2, 1, 4, 0, 2, 0])
    r2 = math.sqrt(2.0)
    assert list(report) == ["rho", "predicted", "actual", "completeness", "correctness", "quality", "f1"]
    assert report["predicted"] == {"straight": 3, "diagonal": 2, "length": 3 + 2 * r2, "matched_straight": 2, "matched_diagonal": 1,
                                   "matched_length": 2 + r2}
    assert report["actual"] == {"straight": 4, "diagonal": 0, "length": 4.0, "matched_straight": 2, "matched_diagonal": 0,
                                "matched_length": 2.0}
    assert report["correctness"] == (2 + r2) / (3 + 2 * r2) and report["completeness"] == 0.5
    assert report["quality"] == (2 + r2) / ((3 + 2 * r2) + 4.0 - 2.0)
    c, k = report["completeness"], report["correctness"]
    assert report["f1"] == 2 * c * k / (c + k)
    with pytest.raises(ValueError):
        H.centerline_report(5, [1, 2, 3])


def test_the_key_comes_after_boundary_and_before_probability_and_is_absent_without_it():
    matrix = [[90, 2], [3, 5]]
    centerline = H.centerline_report(3, [3, 2, 2, 1, 4, 0, 2, 0])
    report = H.build_report(CLASSES, matrix, 1, 0, kind="road", objects={}, boundary=H.boundary_report(2, [1, 1, 1]),
                            probability={"class": "road"}, centerline=centerline)
    keys = list(report)
    assert keys.index("boundary") + 1 == keys.index("centerline") == keys.index("probability") - 1
    assert report["centerline"] == centerline
    assert "centerline" not in H.build_report(CLASSES, matrix, 1, 0, kind="road", objects={})


def test_the_tile_columns_are_there_only_when_given(tmp_path):
    tiles = [Tile(5, 7, 18), Tile(5, 6, 18), Tile(4, 9, 18)]
    matrices = [[[90, 5], [0, 5]], [[60, 30], [10, 0]], [[100, 0], [0, 0]]]
    links = [[3, 2, 2, 1, 4, 0, 2, 0], [0, 0, 0, 0, 5, 1, 0, 0], [0] * 8]
    rows = H.tile_rows(tiles, matrices, CLASSES, kind="road", centerline=links)
    plain = H.tile_rows(tiles, matrices, CLASSES, kind="road")
    assert [(r["z"], r["x"], r["y"]) for r in rows] == [(r["z"], r["x"], r["y"]) for r in plain] == [(18, 5, 6), (18, 5, 7), (18, 4, 9)]
    assert all("centerline_quality" not in r for r in plain)
    whole = H.centerline_report(1, links[0])
    assert (rows[1]["centerline_completeness"], rows[1]["centerline_correctness"], rows[1]["centerline_quality"]) == (
        whole["completeness"], whole["correctness"], whole["quality"])
    assert (rows[0]["centerline_completeness"], rows[0]["centerline_correctness"], rows[0]["centerline_quality"]) == (0.0, None, 0.0)
    path, path_plain = str(tmp_path / "tiles.csv"), str(tmp_path / "plain.csv")
    H.write_tile_rows(path, rows, CLASSES, centerline=True)
    H.write_tile_rows(path_plain, plain, CLASSES)
    with open(path, newline="") as fp:
        read = list(csv.reader(fp))
    with open(path_plain, newline="") as fp:
        read_plain = list(csv.reader(fp))
    assert read[0] == read_plain[0] + ["centerline_completeness", "centerline_correctness", "centerline_quality"]
    assert [line[:len(read_plain[0])] for line in read] == read_plain
    assert read[1][-3:] == ["0.0", "", "0.0"] and read[3][-3:] == ["", "", ""]
    assert [float(v) for v in read[2][-3:]] == [whole["completeness"], whole["correctness"], whole["quality"]]


# ---- the flag ------------------------------------------------------------------------------------------------------------------
def _parser():
    from robosat_amd.tools import evaluate as tool

    parser = argparse.ArgumentParser()
    tool.add_parser(parser.add_subparsers())
    return parser, tool


def _dirs(tmp_path):
    from robosat_amd import png
    from robosat_amd.colors import make_palette

    dataset = tmp_path / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "road"]\ncolors = ["denim", "orange"]\n')
    for name in ("masks", "labels"):
        os.makedirs(str(tmp_path / name / "18" / "5"))
        png.write_png(str(tmp_path / name / "18" / "5" / "7.png"), np.zeros((8, 6), dtype=np.uint8), "P", make_palette("denim", "orange"))
    return ["evaluate", str(tmp_path / "masks"), str(tmp_path / "labels"), "--dataset", str(dataset), str(tmp_path / "report.json")]


def test_the_flag_parses_defaults_off_and_its_help_asks_for_stitch(tmp_path):
    parser, _ = _parser()
    base = _dirs(tmp_path)
    assert parser.parse_args(base).centerline == 0
    assert parser.parse_args(base + ["--type", "road", "--centerline", "3"]).centerline == 3
    help_text = " ".join(parser._subparsers._group_actions[0].choices["evaluate"].format_help().split())
    assert "Roads want --stitch" in help_text and "half a road's width short of every tile border" in help_text
    assert "beyond the tile edge is unknown" in help_text


@pytest.mark.parametrize("extra, words", [
    (["--centerline", "3"], ["--centerline", "--type"]),
    (["--type", "road", "--centerline", "-1"], ["--centerline", "-1", "1..127"]),
    (["--type", "road", "--centerline", "128"], ["--centerline", "128", "1..127"]),
    (["--type", "road", "--stitch", "--centerline", "6"], ["--centerline 6", "7 pixels", "8x6", "at most 5"]),
])
def test_main_rejects_a_bad_flag_before_it_needs_a_device(tmp_path, monkeypatch, extra, words):
    import torch

    parser, tool = _parser()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flags are checked before the device is"))
    with pytest.raises(SystemExit) as exc:
        tool.main(parser.parse_args(_dirs(tmp_path) + extra))
    assert isinstance(exc.value.code, str) and exc.value.code.startswith("Error:")
    for word in words:
        assert word in exc.value.code, (word, exc.value.code)


@pytest.mark.parametrize("extra", [["--type", "road", "--centerline", "127"], ["--type", "road", "--stitch", "--centerline", "5"]])
def test_with_a_good_flag_main_goes_on_to_ask_for_the_device(tmp_path, monkeypatch, extra):
    import torch

    parser, tool = _parser()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as exc:
        tool.main(parser.parse_args(_dirs(tmp_path) + extra))
    assert exc.value.code == "Error: this build computes on the MI355X only"
