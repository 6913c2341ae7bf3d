"""``rs features --dedupe`` without a GPU: the new entry point is declared additively, ``dedupe_keep`` on hand-made tables in both
layouts (the reference's ``iou(...) < threshold`` on pixel counts), and the validation of the two flags at the parser and in
``main``, which rejects them before it asks for a device."""

import argparse
import os
import re

import numpy as np
import pytest

from robosat_amd import features as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_overlap_entry_point_is_declared_additively():
    from robosat_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    assert "rs_features_overlaps(" in header and re.search(r"\bint rs_features_overlaps\(", header)
    assert re.search(r"\blong rs_features_overlaps_workspace_bytes\(", header)
    assert "rs_features_overlaps" in _lib.SIGNATURES and "rs_features_overlaps_workspace_bytes" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 24
    assert callable(ops.overlap_table)


# P (label 5, area 12) shares 4 pixels with Q1 (area 9) and 2 with Q2 (area 6): inter 6, union 12 + 9 + 6 - 6 = 21.
# R (label 40, area 7) touches nothing; S (label 50, area 3) shares one pixel with Q3 (area 100): 1 / 102.
def _tables(per_tile):
    table = np.array([[5, 12, 0, 0, 3, 2], [40, 7, 5, 5, 7, 7], [50, 3, 9, 9, 9, 11]], dtype=np.int32)
    ref = np.array([[2, 9, 0, 0, 2, 2], [17, 6, 3, 0, 4, 2], [60, 100, 9, 9, 18, 18], [90, 1, 20, 20, 20, 20]], dtype=np.int32)
    pairs = np.array([[0, 5, 17, 2], [0, 50, 60, 1], [0, 5, 2, 4]], dtype=np.int32)
    if per_tile:  # the same three in tile 1; tile 0 holds a component with P's label that nothing touches, and an unrelated pair
        table = np.concatenate([[[0, 5, 12, 0, 0, 3, 2]], np.insert(table, 0, 1, axis=1)]).astype(np.int32)
        ref = np.concatenate([[[0, 2, 50, 8, 8, 20, 20]], np.insert(ref, 0, 1, axis=1)]).astype(np.int32)
        pairs[:, 0] = 1
    return table, ref, pairs


@pytest.mark.parametrize("per_tile", [False, True], ids=["stitched", "per_tile"])
def test_dedupe_keep_on_a_hand_made_case(per_tile):
    table, ref, pairs = _tables(per_tile)
    first = 1 if per_tile else 0  # row of P

    def run(threshold):
        keep, iou = F.dedupe_keep(table, ref, pairs, threshold)
        assert keep.dtype == bool and keep.shape == (len(table),) and iou.dtype == np.float64 and iou.shape == (len(table),)
        return keep.tolist()[first:], iou.tolist()[first:], keep.tolist()[:first], iou.tolist()[:first]

    keep, iou, keep_other, iou_other = run(0.3)
    assert iou == [6 / 21, 0.0, 1 / 102]
    assert keep == [True, True, True]
    assert keep_other == [True] * first and iou_other == [0.0] * first  # (tile 0's label 5 is another component)
    assert run(0.28)[0] == [False, True, True]
    assert run(6 / 21)[0] == [False, True, True]  # strict: an IoU of exactly the threshold is a duplicate
    assert run(np.nextafter(6 / 21, 1))[0] == [True, True, True]
    assert run(0.0)[0] == [False, True, False]  # everything that touches the reference goes
    assert run(1.0)[0] == [True, True, True]
    assert run(0.0)[1] == iou  # the IoU does not depend on the threshold


def test_dedupe_keep_takes_pairs_in_any_order_and_empty_tables():
    table, ref, pairs = _tables(True)
    want = F.dedupe_keep(table, ref, pairs, 0.2)
    got = F.dedupe_keep(table, ref, pairs[::-1], 0.2)
    assert (want[0] == got[0]).all() and (want[1] == got[1]).all()
    keep, iou = F.dedupe_keep(table, ref[:0], pairs[:0], 0.0)
    assert keep.all() and (iou == 0.0).all()
    keep, iou = F.dedupe_keep(table[:0], ref, pairs[:0], 0.5)
    assert keep.shape == (0,) and iou.shape == (0,)
    with pytest.raises(ValueError):
        F.dedupe_keep(table, ref[:, 1:], pairs, 0.5)  # one table per tile, the other stitched
    with pytest.raises(ValueError):
        F.dedupe_keep(table, ref[:2], pairs, 0.5)  # a pair with a reference component the table does not list


def test_a_whole_object_is_a_duplicate_where_its_halves_are_not():
    """The reason for --stitch with --dedupe: the halves of a predicted object either side of a seam against the halves of the
    reference object under it give other ratios than the two whole objects do."""

    whole = F.dedupe_keep(np.array([[1, 100, 0, 0, 0, 0]]), np.array([[1, 80, 0, 0, 0, 0]]), np.array([[0, 1, 1, 60]]), 0.5)
    assert whole[0].tolist() == [False] and whole[1].tolist() == [60 / 120]
    halves = F.dedupe_keep(np.array([[0, 1, 50, 0, 0, 0, 0], [1, 1, 50, 0, 0, 0, 0]]), np.array([[0, 1, 70, 0, 0, 0, 0], [1, 9, 10, 0, 0, 0, 0]]),
                           np.array([[0, 1, 1, 50], [1, 1, 9, 10]]), 0.5)
    assert halves[0].tolist() == [False, True] and halves[1].tolist() == [50 / 70, 10 / 50]


def _parser():
    from robosat_amd.tools import features as tool

    parser = argparse.ArgumentParser()
    tool.add_parser(parser.add_subparsers())
    return parser, tool


BASE = ["features", "masks", "--type", "parking", "out.geojson"]


def test_the_dedupe_flags_parse_and_default_off():
    parser, _ = _parser()
    args = parser.parse_args(BASE + ["--dataset", "d.toml"])
    assert args.dedupe is None and args.dedupe_threshold is None
    args = parser.parse_args(BASE + ["--dataset", "d.toml", "--dedupe", "labels", "--dedupe_threshold", "0.25"])
    assert args.dedupe == "labels" and args.dedupe_threshold == 0.25
    with pytest.raises(SystemExit):
        parser.parse_args(BASE + ["--dataset", "d.toml", "--dedupe", "labels", "--dedupe_threshold", "half"])


@pytest.mark.parametrize("extra, word", [
    (["--dedupe", "{labels}"], "--dedupe_threshold"),
    (["--dedupe_threshold", "0.5"], "--dedupe"),
    (["--dedupe", "{labels}", "--dedupe_threshold", "1.5"], "0 <= T <= 1"),
    (["--dedupe", "{labels}", "--dedupe_threshold", "-0.1"], "0 <= T <= 1"),
    (["--dedupe", "{labels}", "--dedupe_threshold", "nan"], "0 <= T <= 1"),
    (["--dedupe", "{labels}", "--dedupe_threshold", "0.5", "--geometry", "centerline"], "centerline"),
    (["--dedupe", "{labels}/missing", "--dedupe_threshold", "0.5"], "not a directory"),
])
def test_main_rejects_bad_dedupe_flags_before_it_needs_a_device(tmp_path, monkeypatch, extra, word):
    import torch

    parser, tool = _parser()
    dataset = tmp_path / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "parking"]\ncolors = ["denim", "orange"]\n')
    labels = tmp_path / "labels"
    labels.mkdir()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flags are checked before the device is"))
    args = parser.parse_args(BASE + ["--dataset", str(dataset)] + [e.format(labels=labels) for e in extra])
    with pytest.raises(SystemExit) as exc:
        tool.main(args)
    assert isinstance(exc.value.code, str) and exc.value.code.startswith("Error:") and word in exc.value.code
