"""``rs features --dedupe`` on the MI355X: ``ops.overlap_table`` (csrc/features.hip, rs_features_overlaps) against its definition
restated with ``np.unique``, on label rasters the device's own labelling made from the masks of tests/features_ref.py; then the
stages of the tool against the restatement of the whole rule.  Counts are integers: everything is exact."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _labels(masks):
    return ops.label_components(_dev(np.stack(masks).astype(np.uint8)))


def _restated(a, b, stitched):
    """Rows (raster, label_a, label_b, count) of two numpy label stacks [B, H, W], sorted."""

    raster = np.zeros(a.shape, dtype=np.int64) if stitched else np.broadcast_to(np.arange(len(a))[:, None, None], a.shape)
    both = (a != 0) & (b != 0)
    triples = np.stack([raster[both], a[both], b[both]], axis=1).astype(np.int64)
    if len(triples) == 0:
        return np.zeros((0, 4), dtype=np.int64)
    rows, counts = np.unique(triples, axis=0, return_counts=True)
    return np.concatenate([rows, counts[:, None]], axis=1)


def _check(a, b, stitched=False, capacity=None):
    got = ops.overlap_table(a, b, stitched=stitched, capacity=capacity)
    assert got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 4 and got.is_contiguous()
    want = _restated(a.cpu().numpy(), b.cpu().numpy(), stitched)
    assert got.shape[0] == len(want), (got.shape[0], len(want))
    assert (got.cpu().numpy() == want).all()
    return want


def test_two_independent_blob_rasters_of_a_width_that_is_no_multiple_of_64():
    a = _labels([R.blobs(48, 70, seed) for seed in (1, 2, 3)])
    b = _labels([R.blobs(48, 70, seed) for seed in (4, 5, 6)])
    want = _check(a, b)
    assert sorted(set(want[:, 0].tolist())) == [0, 1, 2] and want[:, 3].max() > 64  # every tile, and runs longer than a wave's share


def test_all_ones_is_one_pair_per_tile_holding_every_pixel():
    ones = _labels([np.ones((96, 80), dtype=bool)] * 2)
    want = _check(ones, ones)
    assert want.tolist() == [[0, 1, 1, 96 * 80], [1, 1, 1, 96 * 80]]


def test_a_checkerboard_against_itself_is_one_pair_per_pixel_and_against_its_shift_none():
    board = R.checkerboard(64, 64)
    a = _labels([board])
    want = _check(a, a)
    assert len(want) == 2048 and (want[:, 3] == 1).all() and (want[:, 1] == want[:, 2]).all()
    assert len(_check(a, _labels([~board]))) == 0  # the board shifted by one pixel


def test_empty_rasters_have_no_rows():
    empty = _labels([np.zeros((64, 64), dtype=bool)])
    assert ops.overlap_table(empty, empty).shape == (0, 4)
    assert len(_check(empty, _labels([R.blobs(64, 64, 7)]))) == 0


def test_a_capacity_of_8_grows_to_the_same_rows():
    a = _labels([R.noise(64, 64, 8, 0.5)])
    b = _labels([R.blobs(64, 64, 9)])
    want = _check(a, b)
    assert len(want) > 16, "fewer pairs than the smallest hash table holds: the test shows nothing"
    assert (_check(a, b, capacity=8) == want).all()
    assert (_check(a, b, capacity=len(want)) == want).all()  # exactly enough
    assert (_check(a, b, capacity=len(want) - 1) == want).all()  # the table holds them, the rows do not: one more call
    with pytest.raises(ValueError):
        ops.overlap_table(a, b, capacity=0)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 130)])
def test_degenerate_shapes(h, w):
    a = _labels([np.ones((h, w), dtype=bool)])
    assert _check(a, a).tolist() == [[0, 1, 1, h * w]]
    mask = R.noise(h, w, 10, 0.6)
    _check(_labels([mask]), a)
    tiles = _labels([np.ones((h, w), dtype=bool)] * 5)  # tiles smaller than a thread's share of pixels
    assert _check(tiles, tiles).tolist() == [[t, 1, 1, h * w] for t in range(5)]


def test_rasters_that_start_off_a_16_byte_boundary():
    """The kernel reads 16 bytes per thread where both rasters allow it and single labels where not; 3 * 5 * 7 pixels is no multiple of 4."""

    a = _labels([R.noise(5, 7, seed, 0.8) for seed in (11, 12, 13)])
    b = _labels([R.noise(5, 7, seed, 0.8) for seed in (14, 15, 16)])
    want = _check(a, b)
    assert len(want) > 0
    shifted = torch.zeros(a.numel() + 1, device=a.device, dtype=torch.int32)
    shifted[1:] = a.reshape(-1)
    a_off = shifted[1:].view(a.shape)
    assert a_off.data_ptr() % 16 == 4 and a_off.is_contiguous()
    assert (_check(a_off, b) == want).all()
    assert len(_check(b, a_off)) == len(want)


def _mosaic(seed):
    """64 x 80 (2 x 2 tiles of 32 x 40) with a blob over the centre."""

    yy, xx = np.mgrid[:64, :80]
    return R.blobs(64, 80, seed, 5) | (((yy - 31) / 11) ** 2 + ((xx - 41) / 14) ** 2 <= 1)


def test_a_stitched_mosaic_is_one_raster_and_counts_run_across_the_seams():
    grids = [S.Grid(S.split(_mosaic(seed).astype(np.uint8), 32, 40), 0) for seed in (17, 18)]
    nbr = _dev(grids[0].tables()[0])
    local = [ops.label_components(_dev(g.stack)) for g in grids]
    a, b = (ops.stitch_labels(labels, nbr) for labels in local)
    for g, got in zip(grids, (a, b)):
        assert (got.cpu().numpy() == g.cut(g.global_labels(g.canvas))).all()
    want = _check(a, b, stitched=True)
    assert (want[:, 0] == 0).all()
    centre = want[np.argmax(want[:, 3])]  # the two centre blobs: their pair has pixels in all four tiles
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    per_tile = [int(((an[t] == centre[1]) & (bn[t] == centre[2])).sum()) for t in range(4)]
    assert min(per_tile) > 0 and sum(per_tile) == centre[3]
    assert len(_check(*local)) > len(want)  # tile by tile that pair is four rows


def test_what_the_library_refuses():
    a = _labels([np.ones((4, 6), dtype=bool)] * 2)
    ws = torch.zeros(1 << 10, device=a.device, dtype=torch.int64)
    rows = torch.zeros((8, 4), device=a.device, dtype=torch.int32)
    counters = torch.zeros(2, device=a.device, dtype=torch.int32)
    lib = ops._lib.lib()

    def call(pixels, group, capacity=8, rows_ptr=rows.data_ptr(), ws_ptr=ws.data_ptr()):
        return lib.rs_features_overlaps(a.data_ptr(), a.data_ptr(), ws_ptr, rows_ptr, capacity, counters.data_ptr(), pixels, group,
                                        torch.cuda.current_stream().cuda_stream)

    assert call(48, 24) == 0 and call(48, 48) == 0
    torch.cuda.synchronize()
    for pixels, group in ((48, 36), (48, 0), (0, 24), (1 << 29, 1 << 29)):
        assert call(pixels, group) == ops._lib.RS_EINVAL, (pixels, group)
    assert call(48, 24, capacity=-1) == ops._lib.RS_EINVAL
    assert call(48, 24, rows_ptr=None) == ops._lib.RS_EINVAL and call(48, 24, ws_ptr=None) == ops._lib.RS_EINVAL
    assert call(48, 24, ws_ptr=ws.data_ptr() + 4) == ops._lib.RS_EINVAL
    assert lib.rs_features_overlaps_workspace_bytes(8) == 16 * 12 and lib.rs_features_overlaps_workspace_bytes(9) == 32 * 12
    assert lib.rs_features_overlaps_workspace_bytes(-1) == ops._lib.RS_EINVAL
    assert call(48, 24, capacity=0, rows_ptr=None) == 0  # count only
    assert counters.tolist() == [2, 0]


# ---- the stages of the tool against the rule written out ---------------------------------------------------------------------
INDEX, DENOISE, GROW, MIN_AREA, THRESHOLD = 2, 3, 4, 12, 0.3


def _rule(pred, ref, threshold):
    """{label: (area, iou)} of the kept components of ONE raster: ``pred`` and ``ref`` numpy label images."""

    kept = {}
    for label in np.unique(pred[pred != 0]).tolist():
        mask = pred == label
        touched = np.unique(ref[mask & (ref != 0)]).tolist()
        inter = int((mask & (ref != 0)).sum())
        union = int(mask.sum()) + sum(int((ref == q).sum()) for q in touched) - inter
        if not touched:
            kept[label] = (int(mask.sum()), 0.0)
        elif inter < threshold * union:
            kept[label] = (int(mask.sum()), inter / union)
    return kept


def _images(seed, h, w):
    rng = np.random.RandomState(seed)
    image = rng.choice(np.array([0, 1], dtype=np.uint8), size=(h, w))
    image[R.blobs(h, w, seed, 10)] = INDEX
    return image


def test_the_stages_per_tile_equal_the_rule(tmp_path):
    from robosat_amd.tools.features import Dedupe

    masks = np.stack([_images(seed, 48, 70) for seed in (21, 22, 23)])
    shifted = np.roll(masks, (3, -5), axis=(1, 2))  # the same objects a little off: a spread of IoUs
    shifted[2] = _images(24, 48, 70)
    shifted[1, :, 35:] = 0
    dedupe = Dedupe(str(tmp_path), THRESHOLD, INDEX)
    labels = ops.label_components(ops.clean_masks(_dev(masks), INDEX, DENOISE, GROW))
    table = ops.component_table(labels, MIN_AREA)
    kept, iou = dedupe.filter(labels, table, _dev(shifted))
    want = {}
    for t in range(3):
        pred = R.filter_labels(R.label(R.clean(masks[t], INDEX, DENOISE, GROW)), MIN_AREA)
        for label, value in _rule(pred, R.label(shifted[t] == INDEX), THRESHOLD).items():
            want[(t, label)] = value
    assert dedupe.examined == len(table) and dedupe.dropped == len(table) - len(want) and 0 < len(want) < len(table)
    assert {(int(r[0]), int(r[1])): int(r[2]) for r in kept.cpu().numpy()} == {k: v[0] for k, v in want.items()}
    assert iou == {k: v[1] for k, v in want.items()}  # floats, to the last bit
    assert any(0 < v < THRESHOLD for v in iou.values()) and any(v == 0 for v in iou.values())


def test_the_stages_stitched_equal_the_rule(tmp_path):
    from robosat_amd.tools.features import Dedupe

    image = np.where(_mosaic(25), INDEX, 0).astype(np.uint8)
    other = np.roll(np.where(_mosaic(25) | _mosaic(26), INDEX, 1).astype(np.uint8), (2, 4), axis=(0, 1))
    grid, ref_grid = S.Grid(S.split(image, 32, 40), S.margin(DENOISE, GROW)), S.Grid(S.split(other, 32, 40), S.margin(DENOISE, GROW))
    nbr, origin = (_dev(t) for t in grid.tables())
    dedupe = Dedupe(str(tmp_path), 0.9, INDEX)
    labels = ops.stitch_labels(ops.label_components(ops.clean_masks_stitched(_dev(grid.stack), nbr, INDEX, DENOISE, GROW)), nbr, inplace=True)
    table = ops.component_table_stitched(labels, origin, MIN_AREA)
    kept, iou = dedupe.filter(labels, table, _dev(ref_grid.stack), nbr, origin)
    pred = R.filter_labels(grid.global_labels(R.clean(grid.canvas, INDEX, DENOISE, GROW) * (grid.index >= 0)), MIN_AREA)
    want = _rule(pred, ref_grid.global_labels(ref_grid.canvas == INDEX), 0.9)
    assert {int(r[0]): int(r[1]) for r in kept.cpu().numpy()} == {k: v[0] for k, v in want.items()}
    assert iou == {k: v[1] for k, v in want.items()}
    assert dedupe.examined == len(table) and len(want) > 0 and any(v > 0 for v in iou.values())
