"""``rs features --score`` without a GPU: the new entry point is declared and exported, ``scores_from_sums`` against the probability
``rs masks`` votes with, the ``score`` argument of ``featurize`` / ``featurize_stitched``, and the validation of the flags in
``main``, which rejects them before it asks for a device."""

import argparse
import io
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import score_ref as C  # noqa: E402

from robosat_amd import features as F  # noqa: E402
from robosat_amd.tiles import Tile  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_in_the_header_and_exported_by_the_library():
    from robosat_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    assert re.search(r"\bint rs_features_scores\(const int32_t\* labels, const uint8_t\* q,", header)
    assert "rs_features_scores" in _lib.SIGNATURES and len(_lib.SIGNATURES["rs_features_scores"][1]) == 11
    assert _lib.ABI_VERSION == 24  # (a new symbol, no old one changed)
    assert callable(ops.component_scores)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librobosat_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    assert hasattr(_lib.lib(), "rs_features_scores")


def test_the_restatement_sums_what_it_says():
    labels = np.array([[[1, 1, 0], [0, 5, 5]], [[1, 0, 0], [0, 0, 6]]])
    q = np.arange(24, dtype=np.uint8).reshape(2, 2, 2, 3)
    got = C.sums(labels, q)
    assert sorted(got) == [(0, 1), (0, 5), (1, 1), (1, 6)]
    assert got[(0, 1)].tolist() == [0 + 1, 12 + 13] and got[(0, 5)].tolist() == [4 + 5, 16 + 17]
    assert got[(1, 1)].tolist() == [6, 18] and got[(1, 6)].tolist() == [11, 23]
    assert C.rows(np.array([[1, 6, 1, 0, 0, 0, 0], [0, 5, 2, 0, 0, 0, 0]]), got, 2).tolist() == [[11, 23], [9, 33]]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_scores_from_sums_is_the_mean_of_the_soft_vote_over_the_component(k, weighted):
    """Bound 1e-9: the integer form is exact up to its one division; numpy's float64 mean over at most 2^12 pixels of a weighted
    average of K terms errs by under (2^12 + K) * 2^-53, about 5e-13."""

    rng = np.random.RandomState(k)
    labels = np.stack([R.label(R.blobs(48, 70, seed)) for seed in (1, 2)])
    q = rng.randint(0, 256, size=(k, 2, 48, 70)).astype(np.uint8)
    weights = (rng.rand(k) * 3 + 0.1).tolist() if weighted else None
    by_key = C.sums(labels, q)
    keys = sorted(by_key)
    sums = np.array([by_key[key] for key in keys])
    areas = np.array([(labels[r] == name).sum() for r, name in keys])
    got = F.scores_from_sums(sums, areas, weights)
    assert got.dtype == np.float64 and got.shape == (len(keys),) and len(keys) > 10
    want = [C.mean_vote(q[:, r], labels[r] == name, weights) for r, name in keys]
    worst = max(abs(g - w) for g, w in zip(got.tolist(), want))
    print("worst difference", worst)
    assert worst <= 1e-9


def test_scores_from_sums_on_hand_made_numbers_and_bad_arguments():
    got = F.scores_from_sums(np.array([[255 * 4, 0], [0, 0], [510, 255]]), np.array([4, 9, 2]), [1, 3])
    assert got.tolist() == [1020 / (255 * 4 * 4.0), 0.0, (510 + 3 * 255) / (255 * 2 * 4.0)]
    assert F.scores_from_sums(np.array([[255 * 7]]), [7]).tolist() == [1.0]
    assert F.scores_from_sums(np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.int64)).shape == (0,)
    assert F.scores_from_sums(np.array([[100, 50]]), [1], [0, 2]).tolist() == [100 / (255 * 2.0)]  # (a weight of 0 mutes a model)
    for sums, areas, weights in ((np.zeros((2, 2)), [1], None), (np.zeros((1, 2)), [1], [1]), (np.zeros((1, 2)), [1], [1, -1]),
                                 (np.zeros((1, 2)), [1], [0, 0]), (np.zeros((1, 2)), [1], [1, float("nan")]),
                                 (np.zeros((1, 2)), [1], [1, float("inf")]), (np.zeros((1, 2)), [0], None), (np.zeros(3), [1, 1, 1], None)):
        with pytest.raises(ValueError):
            F.scores_from_sums(sums, areas, weights)


def test_the_score_argument_writes_the_property_and_none_leaves_the_features_as_they_were():
    labels = R.label(R.corner_touch())
    table, edges = R.table(labels), R.edges(labels)
    tile = Tile(69623, 104945, 18)
    plain = F.featurize(edges, table, [tile], labels.shape, 0, warn=io.StringIO())
    assert F.featurize(edges, table, [tile], labels.shape, 0, warn=io.StringIO(), score=None) == plain
    score = {(0, int(r[1])): 0.25 + 0.001 * i for i, r in enumerate(table)}
    scored = F.featurize(edges, table, [tile], labels.shape, 0, warn=io.StringIO(), score=score)
    assert [f["properties"]["score"] for f in scored] == [score[key] for key in sorted(score)] and len(scored) == len(table) > 1
    both = F.featurize(edges, table, [tile], labels.shape, 0, warn=io.StringIO(), score=score, iou={key: 0.0 for key in score})
    assert all(list(f["properties"]) == ["tile", "area_px", "iou", "score"] for f in both)
    for feature in scored:
        del feature["properties"]["score"]
    assert scored == plain

    rows, stitched_table = edges[:, 1:], table[:, 1:]  # (one tile as a stitched call: the same labels, rows of 4 and of 6)
    plain = F.featurize_stitched(rows, stitched_table, [tile], labels.shape, 0, warn=io.StringIO())
    assert F.featurize_stitched(rows, stitched_table, [tile], labels.shape, 0, warn=io.StringIO(), score=None) == plain
    by_label = {label: value for (_, label), value in score.items()}
    scored = F.featurize_stitched(rows, stitched_table, [tile], labels.shape, 0, warn=io.StringIO(), score=by_label)
    assert [f["properties"]["score"] for f in scored] == [by_label[key] for key in sorted(by_label)]
    for feature in scored:
        del feature["properties"]["score"]
    assert scored == plain


def _parser():
    from robosat_amd.tools import features as tool

    parser = argparse.ArgumentParser()
    tool.add_parser(parser.add_subparsers())
    return parser, tool


BASE = ["features", "masks", "--type", "parking", "out.geojson"]


def test_the_score_flags_parse_and_default_off():
    parser, _ = _parser()
    args = parser.parse_args(BASE + ["--dataset", "d.toml"])
    assert args.score is None and args.score_weights is None and args.min_score is None
    args = parser.parse_args(BASE + ["--dataset", "d.toml", "--score", "a", "--score", "b", "--score_weights", "2", "1", "--min_score", "0.5"])
    assert args.score == ["a", "b"] and args.score_weights == [2.0, 1.0] and args.min_score == 0.5
    with pytest.raises(SystemExit):
        parser.parse_args(BASE + ["--dataset", "d.toml", "--score", "a", "--min_score", "half"])


@pytest.mark.parametrize("extra, words", [
    (["--score", "{probs}/missing"], ["--score", "missing", "not a directory"]),
    (["--score", "{probs}", "--score", "{probs}/nowhere"], ["--score", "nowhere", "not a directory"]),
    (["--score_weights", "1", "2"], ["--score_weights", "1.0 2.0", "--score"]),
    (["--min_score", "0.5"], ["--min_score", "0.5", "--score"]),
    (["--score", "{probs}", "--score_weights", "1", "2"], ["--score_weights", "2 weights", "1 directories"]),
    (["--score", "{probs}", "--score", "{probs}", "--score_weights", "1"], ["--score_weights", "1 weights", "2 directories"]),
    (["--score", "{probs}", "--score_weights", "-1"], ["--score_weights", "-1.0"]),
    (["--score", "{probs}", "--score_weights", "nan"], ["--score_weights", "nan"]),
    (["--score", "{probs}", "--score_weights", "inf"], ["--score_weights", "inf"]),
    (["--score", "{probs}", "--score", "{probs}", "--score_weights", "0", "0"], ["--score_weights", "0.0 0.0", "all 0"]),
    (["--score", "{probs}", "--min_score", "1.5"], ["--min_score", "1.5", "0 <= S <= 1"]),
    (["--score", "{probs}", "--min_score", "-0.1"], ["--min_score", "-0.1", "0 <= S <= 1"]),
    (["--score", "{probs}", "--min_score", "nan"], ["--min_score", "nan", "0 <= S <= 1"]),
    (["--score", "{probs}", "--geometry", "centerline"], ["--score", "centerline"]),
])
def test_main_rejects_bad_score_flags_before_it_needs_a_device(tmp_path, monkeypatch, extra, words):
    import torch

    parser, tool = _parser()
    dataset = tmp_path / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking"]\ncolors = ["denim", "orange"]\n')
    probs = tmp_path / "probs"
    probs.mkdir()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flags are checked before the device is"))
    args = parser.parse_args(BASE + ["--dataset", str(dataset)] + [e.format(probs=probs) for e in extra])
    with pytest.raises(SystemExit) as exc:
        tool.main(args)
    assert isinstance(exc.value.code, str) and exc.value.code.startswith("Error:")
    for word in words:
        assert word in exc.value.code, (word, exc.value.code)


def test_with_good_flags_main_goes_on_to_ask_for_the_device(tmp_path, monkeypatch):
    """The other side of the test above, as on a machine without one: nothing about the flags stops it, the missing device does."""

    import torch

    parser, tool = _parser()
    dataset = tmp_path / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking"]\ncolors = ["denim", "orange"]\n')
    probs = tmp_path / "probs"
    probs.mkdir()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    args = parser.parse_args(BASE + ["--dataset", str(dataset), "--score", str(probs), "--score", str(probs), "--score_weights", "0", "2.5",
                                     "--min_score", "1"])
    with pytest.raises(SystemExit) as exc:
        tool.main(args)
    assert exc.value.code == "Error: this build computes on the MI355X only"
