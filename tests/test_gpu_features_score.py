"""``rs features --score`` on the MI355X: ``ops.component_scores`` (csrc/features.hip, rs_features_scores) against its definition
restated with ``np.add.at`` (tests/score_ref.py), on label rasters the device's own stages made.  The shapes are the smallest at
which the kernel can go wrong: raster borders inside a wave, runs of one pixel and runs longer than a block, a tail block, a table
that lists some components only, stitched and split labels, and a sum above 2^32.  Sums are integers: everything is exact."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import score_ref as C  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bytes(k, shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(k,) + tuple(shape)).astype(np.uint8)


def _labels(masks):
    return ops.label_components(_dev(np.stack(masks).astype(np.uint8)))


def _check(labels, table, q, stitched=False):
    """The device's sums for ``table`` against the restatement on the same labels; returns them as numpy [N, K]."""

    got = ops.component_scores(labels, table, _dev(q), stitched=stitched)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(table), q.shape[0]) and got.is_contiguous() and got.is_cuda
    lab = labels.cpu().numpy()
    by_key = C.sums(lab.reshape((1,) + lab.shape) if stitched else lab, q.reshape((q.shape[0], 1) + lab.shape) if stitched else q)
    want = C.rows(table.cpu().numpy(), by_key, q.shape[0], stitched)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (got.cpu().numpy() - want)
    return want


@pytest.mark.parametrize("k", [1, 3, 8])
def test_label_1_either_side_of_a_tile_border_inside_a_wave_is_two_components(k):
    """3 x 5 x 67, all ones: H * W = 335 is a multiple of neither 64 nor 256, so both tile borders lie inside a wave and a block, with
    label 1 on both sides."""

    labels = _labels([np.ones((5, 67), dtype=bool)] * 3)
    table = ops.component_table(labels)
    assert table.cpu().numpy()[:, :3].tolist() == [[0, 1, 335], [1, 1, 335], [2, 1, 335]]
    want = _check(labels, table, _bytes(k, (3, 5, 67), 10 + k))
    assert len({tuple(row) for row in want.tolist()}) == 3, "three different sums, or the test shows nothing"


def _pairs():
    full = np.ones((64, 64), dtype=bool)
    board = R.checkerboard(64, 64)
    return {"checkerboard": [board, ~board], "salt_and_pepper": [R.noise(64, 64, 21, 0.5), R.noise(64, 64, 22, 0.5)], "full": [full, full]}


@pytest.mark.parametrize("name", ["checkerboard", "salt_and_pepper", "full"])
def test_runs_of_one_pixel_and_runs_of_a_whole_tile(name):
    labels = _labels(_pairs()[name])
    table = ops.component_table(labels)
    want = _check(labels, table, _bytes(3, (2, 64, 64), 30))
    assert len(want) == {"checkerboard": 4096, "full": 2}.get(name, len(want)) and len(want) >= 2


def test_blobs_on_tiles_of_a_width_that_is_no_multiple_of_64_and_the_same_bits_twice():
    labels = _labels([R.blobs(48, 70, seed) for seed in (1, 2, 3)])
    table = ops.component_table(labels)
    q = _bytes(3, (3, 48, 70), 31)
    want = _check(labels, table, q)
    assert want.max() > 64 * 255, "no component larger than a wave's share"
    first, second = (ops.component_scores(labels, table, _dev(q)) for _ in range(2))
    assert torch.equal(first, second)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 85)])
def test_a_single_component_in_a_tail_block(h, w):
    labels = _labels([np.ones((h, w), dtype=bool)])
    table = ops.component_table(labels)
    q = _bytes(2, (1, h, w), 40)
    q[0] |= 1  # (no sum of 0: a lane past the end that added something would show)
    want = _check(labels, table, q)
    assert want.tolist() == [[int(q[0].sum()), int(q[1].sum())]]


def test_a_filtered_table_gets_its_rows_alone_and_an_empty_one_an_empty_tensor():
    labels = _labels([R.blobs(48, 70, 5), R.noise(48, 70, 6, 0.3)])
    table = ops.component_table(labels)
    q = _bytes(3, (2, 48, 70), 41)
    everything = _check(labels, table, q)
    assert len(table) > 8
    kept = _check(labels, table[::2].contiguous(), q)
    assert (kept == everything[::2]).all()
    reordered = _check(labels, table.flip(0).contiguous(), q)  # (a row is named by its position in the table, whatever the order)
    assert (reordered == everything[::-1]).all()
    none = ops.component_scores(labels, table[:0], _dev(q))
    assert none.dtype == torch.int64 and tuple(none.shape) == (0, 3)


def test_a_row_that_names_no_pixel_of_the_raster_is_skipped():
    labels = _labels([np.ones((4, 9), dtype=bool)] * 2)
    rows = [[0, 1, 36, 0, 0, 8, 3], [0, 0, 1, 0, 0, 0, 0], [0, 37, 1, 0, 0, 0, 0], [2, 1, 1, 0, 0, 0, 0], [-1, 1, 1, 0, 0, 0, 0],
            [0, -5, 1, 0, 0, 0, 0], [1, 1, 36, 0, 0, 8, 3], [1, 5, 1, 0, 0, 0, 0]]  # (the last: a pixel that is no component's root)
    q = _bytes(2, (2, 4, 9), 42)
    got = ops.component_scores(labels, _dev(np.array(rows, dtype=np.int32)), _dev(q)).cpu().numpy()
    want = np.zeros((len(rows), 2), dtype=np.int64)
    want[0], want[6] = q[:, 0].reshape(2, -1).sum(axis=1), q[:, 1].reshape(2, -1).sum(axis=1)
    assert (got == want).all()


def _l_of_three_tiles():
    """Three tiles of 16 x 24 in an L (no tile at the bottom right): one component across both seams, one inside the right tile."""

    canvas = np.zeros((32, 48), dtype=bool)
    canvas[4:10, 10:40] = True  # across the seam at x = 24
    canvas[4:28, 10:16] = True  # across the seam at y = 16
    canvas[12:15, 30:40] = True  # inside the tile on the right
    return S.Grid(S.split(canvas, 16, 24, absent={(1, 1)}), 0)


def test_stitched_labels_sum_over_the_whole_object_across_both_seams():
    grid = _l_of_three_tiles()
    nbr, origin = (_dev(t) for t in grid.tables())
    labels = ops.stitch_labels(ops.label_components(_dev(grid.stack.astype(np.uint8))), nbr, inplace=True)
    table = ops.component_table_stitched(labels, origin)
    assert table.cpu().numpy()[:, 1].tolist() == [6 * 30 + 18 * 6, 30]
    q = _bytes(3, grid.stack.shape, 50)
    got = ops.component_scores(labels, table, _dev(q), stitched=True)
    # the restatement on the assembled mosaic: its labels by the stitched rule, the planes pasted where their tiles lie
    mosaic = grid.global_labels(grid.canvas)
    assert (grid.cut(mosaic) == labels.cpu().numpy()).all()
    by_key = C.sums(mosaic[None], np.stack([grid.paste(plane) for plane in q])[:, None])
    want = C.rows(table.cpu().numpy(), by_key, 3, stitched=True)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    _check(labels, table, q, stitched=True)


def test_after_the_split_every_instance_has_the_sums_of_its_own_pixels():
    """Two discs of radius 10 joined by a bridge 3 pixels wide, split with R = 4: one row per instance, the sums those of the final
    label raster, and together those of the unsplit component."""

    mask = np.zeros((48, 96), dtype=np.uint8)
    yy, xx = np.mgrid[:48, :96]
    for cx in (24, 70):
        mask[np.hypot(yy - 24, xx - cx) <= 10] = 1
    mask[23:26, 24:70] = 1
    cleaned = _dev(mask[None])
    whole = ops.label_components(cleaned)
    q = _bytes(3, (1, 48, 96), 60)
    before = _check(whole, ops.component_table(whole), q)
    assert len(before) == 1
    instances = ops.split_labels(cleaned, whole, 4)
    table = ops.component_table(instances)
    after = _check(instances, table, q)
    assert len(after) == 2 and (after > 0).all()
    assert (after.sum(axis=0) == before[0]).all()


def test_sums_that_no_32_bit_word_holds():
    """1 x 4096 x 4096, all ones (label 1 throughout, as the labeller names it), model 0 all 255, model 1 all 0: 4 278 190 080 is past
    an int32 and 16 777 216 short of 2^32.  The same two tiles as one stitched raster make twice that, which is past 2^32 too."""

    side = 4096
    labels = torch.ones((2, side, side), dtype=torch.int32, device="cuda:0")
    q = torch.zeros((2, 2, side, side), dtype=torch.uint8, device="cuda:0")
    q[0] = 255
    table = _dev(np.array([[0, 1, side * side, 0, 0, side - 1, side - 1]], dtype=np.int32))
    got = ops.component_scores(labels[:1], table, q[:, :1].contiguous())
    assert got.cpu().tolist() == [[4278190080, 0]] and (1 << 31) < 4278190080 == 255 * side * side
    table = _dev(np.array([[1, 2 * side * side, 0, 0, 2 * side - 1, side - 1]], dtype=np.int32))
    got = ops.component_scores(labels, table, q, stitched=True)
    assert got.cpu().tolist() == [[8556380160, 0]] and (1 << 32) < 8556380160 == 2 * 255 * side * side


def test_bad_arguments_raise_before_anything_is_launched():
    labels = _labels([np.ones((4, 4), dtype=bool)])
    table = ops.component_table(labels)
    q = _dev(_bytes(1, (1, 4, 4), 70))
    with pytest.raises(ValueError):
        ops.component_scores(labels, table, _dev(_bytes(9, (1, 4, 4), 71)))  # more than 8 models
    with pytest.raises(ValueError):
        ops.component_scores(labels, table, _dev(_bytes(1, (1, 4, 5), 72)))  # another shape
    with pytest.raises(ValueError):
        ops.component_scores(labels, table, q, stitched=True)  # rows of 7 where rows of 6 are meant
    with pytest.raises(ValueError):
        ops.component_scores(labels, table, q.cpu())  # (there is no CPU path)
    with pytest.raises(RuntimeError):
        ops.component_scores(labels.cpu(), table.cpu(), q.cpu())
    with pytest.raises(TypeError):
        ops.component_scores(labels, table, q.to(torch.int32))
