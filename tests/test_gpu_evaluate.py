"""``rs evaluate`` on the MI355X: ``ops.mask_confusion`` and ``ops.boundary_counts`` (csrc/evaluate.hip) against their definitions
restated in numpy (tests/eval_ref.py).  Every value is an integer, so every comparison is equality.  The shapes are the smallest at
which the kernels can go wrong: one pixel, groups that begin at odd byte offsets (7 x 9 = 63), groups one pixel short of a block
(63 x 65 = 4095, so the block border lies one pixel inside the second tile), exactly a block (64 x 64) and many blocks with a tail
(256 x 257)."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_ref as V  # noqa: E402
import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 7, 9), (2, 63, 65), (1, 64, 64), (2, 256, 257)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _confusion(predicted, actual, classes, stitched=False):
    """The device's counts, checked for form and against the restatement; returned as numpy."""

    counts, bad = ops.mask_confusion(_dev(predicted), _dev(actual), classes, stitched=stitched)
    groups = 1 if stitched else predicted.shape[0]
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (groups, classes, classes) and counts.is_cuda and counts.is_contiguous()
    assert bad.dtype == torch.int64 and tuple(bad.shape) == (groups,)
    want_counts, want_bad = V.confusion(predicted, actual, classes, stitched=stitched)
    assert torch.equal(counts.cpu(), torch.from_numpy(want_counts)), (counts.cpu().numpy() - want_counts)
    assert torch.equal(bad.cpu(), torch.from_numpy(want_bad)), (bad.cpu().numpy(), want_bad)
    return want_counts, want_bad


def _rasters(kind, shape, classes, seed):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, classes, size=shape).astype(np.uint8), rng.randint(0, classes, size=shape).astype(np.uint8)
    if kind == "one_cell":  # every lane of every wave on one counter: actual C - 1, predicted C - 2
        return np.full(shape, classes - 2, dtype=np.uint8), np.full(shape, classes - 1, dtype=np.uint8)
    both = rng.randint(0, classes, size=shape).astype(np.uint8)
    return both, both.copy()


@pytest.mark.parametrize("kind", ["random", "one_cell", "equal"])
@pytest.mark.parametrize("classes", [2, 3, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_mask_confusion_is_the_bincount_per_tile(shape, classes, kind):
    predicted, actual = _rasters(kind, shape, classes, 7 * classes + shape[2])
    counts, bad = _confusion(predicted, actual, classes)
    assert not bad.any() and (counts.sum(axis=(1, 2)) == shape[1] * shape[2]).all()
    if kind == "one_cell":
        assert (counts[:, classes - 1, classes - 2] == shape[1] * shape[2]).all()
    if kind == "equal":
        assert (counts == counts * np.eye(classes, dtype=np.int64)).all()  # the diagonal only


def test_the_counts_are_set_not_added_to_and_the_same_twice():
    predicted, actual = _rasters("random", (2, 63, 65), 3, 5)
    first = ops.mask_confusion(_dev(predicted), _dev(actual), 3)
    second = ops.mask_confusion(_dev(predicted), _dev(actual), 3)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert int(first[0].sum()) == predicted.size


def test_rasters_at_odd_addresses_count_the_same():
    """Views one and three bytes into their buffers: no thread's 16 bytes are aligned, every load is the checked one."""

    predicted, actual = _rasters("random", (2, 63, 65), 8, 6)
    n = predicted.size
    store_p, store_a = torch.zeros(n + 16, dtype=torch.uint8, device="cuda:0"), torch.zeros(n + 16, dtype=torch.uint8, device="cuda:0")
    view_p, view_a = store_p[1:1 + n].view(2, 63, 65), store_a[3:3 + n].view(2, 63, 65)
    view_p.copy_(_dev(predicted))
    view_a.copy_(_dev(actual))
    assert view_p.data_ptr() % 16 == 1 and view_a.data_ptr() % 16 == 3 and view_p.is_contiguous()
    counts, bad = ops.mask_confusion(view_p, view_a, 8)
    want_counts, want_bad = V.confusion(predicted, actual, 8)
    assert torch.equal(counts.cpu(), torch.from_numpy(want_counts)) and torch.equal(bad.cpu(), torch.from_numpy(want_bad))


def _probe_positions(shape):
    """The first and last pixel of every group and the pixels either side of every block border inside the batch."""

    b, h, w = shape
    block = ops.eval_config()
    at = {g * h * w for g in range(b)} | {(g + 1) * h * w - 1 for g in range(b)}
    for border in range(block, b * h * w, block):
        at |= {border - 1, border}
    return sorted(at), block


@pytest.mark.parametrize("shape", [(3, 7, 9), (2, 63, 65)], ids=["3x7x9", "2x63x65"])
def test_one_pixel_moves_one_count_in_its_own_group(shape):
    b, h, w = shape
    positions, block = _probe_positions(shape)
    if shape == (2, 63, 65):
        assert block == 4096 and positions == [0, 4094, 4095, 4096, 8189]  # (the border lies one pixel inside the second tile)
    actual = _dev(np.zeros(shape, dtype=np.uint8))
    for at in positions:
        predicted = np.zeros(shape, dtype=np.uint8)
        predicted.reshape(-1)[at] = 2
        counts, bad = ops.mask_confusion(_dev(predicted), actual, 3)
        want = np.zeros((b, 3, 3), dtype=np.int64)
        want[:, 0, 0] = h * w
        want[at // (h * w), 0, 0] -= 1
        want[at // (h * w), 0, 2] += 1
        assert torch.equal(counts.cpu(), torch.from_numpy(want)), (at, counts.cpu().numpy())
        assert not bad.cpu().numpy().any()


@pytest.mark.parametrize("value", [3, 255])
@pytest.mark.parametrize("side", ["predicted", "actual", "both"])
def test_values_that_are_no_class_are_counted_once_and_in_no_cell(side, value):
    """At the last pixel of the first group (4094) and either side of the block border (4095, 4096); C = 3."""

    shape, classes = (2, 63, 65), 3
    predicted, actual = _rasters("random", shape, classes, 11)
    clean_counts, _ = V.confusion(predicted, actual, classes)
    places = [4094, 4095, 4096]
    removed = np.zeros((2, classes, classes), dtype=np.int64)
    for at in places:
        removed[at // 4095, actual.reshape(-1)[at], predicted.reshape(-1)[at]] += 1
        if side in ("predicted", "both"):
            predicted.reshape(-1)[at] = value
        if side in ("actual", "both"):
            actual.reshape(-1)[at] = value
    counts, bad = _confusion(predicted, actual, classes)
    assert bad.tolist() == [1, 2]  # one per pixel, also where both values are bad
    assert (counts == clean_counts - removed).all()  # every other count as if those pixels were absent


@pytest.mark.parametrize("shape", [(3, 7, 9), (2, 63, 65)], ids=["3x7x9", "2x63x65"])
def test_stitched_is_one_group_the_sum_of_the_tiles(shape):
    predicted, actual = _rasters("random", shape, 3, 12)
    predicted[-1, -1, -1] = 9
    per_tile, per_tile_bad = _confusion(predicted, actual, 3)
    whole, whole_bad = _confusion(predicted, actual, 3, stitched=True)
    assert (whole[0] == per_tile.sum(axis=0)).all() and whole_bad.tolist() == [per_tile_bad.sum()] == [1]


# ---- boundary_counts ---------------------------------------------------------------------------------------------------------
def _pattern(name, h, w, seed):
    if name == "blobs":
        return R.blobs(h, w, seed)
    if name == "checkerboard":
        return R.checkerboard(h, w) if seed % 2 else ~R.checkerboard(h, w)
    m = np.zeros((h, w), dtype=bool)  # comb: a spine along the top (seed odd) or bottom row, every other column a tooth
    m[0 if seed % 2 else -1, :] = True
    m[:, seed % 2::2] = True
    return m


def _boundary(masks_a, masks_b, d, nbr=None):
    d2_a = ops.distance_transform(_dev(masks_a.astype(np.uint8)), d + 1, nbr)
    d2_b = ops.distance_transform(_dev(masks_b.astype(np.uint8)), d + 1, nbr)
    got = ops.boundary_counts(d2_a, d2_b, d, stitched=nbr is not None)
    assert got.dtype == torch.int64 and tuple(got.shape) == (1 if nbr is not None else len(masks_a), 3) and got.is_cuda
    return got.cpu().numpy()


@pytest.mark.parametrize("d", [1, 3, 8])
@pytest.mark.parametrize("name", ["blobs", "comb", "checkerboard"])
@pytest.mark.parametrize("shape", [(2, 63, 65), (3, 7, 9)], ids=["2x63x65", "3x7x9"])
def test_boundary_counts_are_the_bands_of_the_restatement(shape, name, d):
    b, h, w = shape
    masks_a = np.stack([_pattern(name, h, w, 2 * i + 1) for i in range(b)])
    masks_b = np.stack([np.roll(_pattern(name, h, w, 2 * i + (1 if name == "blobs" else 2)), (1, 2) if name == "blobs" else (0, 0), axis=(0, 1))
                        for i in range(b)])
    band_a = np.stack([V.band(m, d) for m in masks_a])
    band_b = np.stack([V.band(m, d) for m in masks_b])
    want = V.boundary(band_a, band_b)
    got = _boundary(masks_a, masks_b, d)
    assert (got == want).all(), (got, want)
    assert want[:, :2].min() > 0 and (want[:, 2] <= want[:, :2].min(axis=1)).all()
    if name == "blobs":
        assert (want[:, 2] > 0).all() and (want[:, 2] < want[:, 0]).all()  # bands that overlap in part


@pytest.mark.parametrize("d", [1, 3, 8])
def test_stitched_bands_reach_across_the_seams(d):
    """A 2 x 2 block of 32 x 32 tiles: a slab that ends exactly at the vertical seam (its nearest unset pixels lie in the next tile)
    and blobs everywhere else.  Per tile the slab has no band along the seam; stitched it has."""

    image_a = R.blobs(64, 64, 3, count=4)
    image_a[4:28, 12:32] = True
    image_a[4:28, 32:40] = False
    image_b = np.roll(image_a, (2, 1), axis=(0, 1))
    grid_a, grid_b = S.Grid(S.split(image_a, 32, 32), 0), S.Grid(S.split(image_b, 32, 32), 0)
    nbr, _ = grid_a.tables()
    band_a, band_b = V.band_stitched(grid_a, d), V.band_stitched(grid_b, d)
    slot = grid_a.coords.index((0, 0))
    assert band_a[slot, 14:18, 31].all() and not V.band(grid_a.stack[slot], d)[14:18, 31].any()  # (the case shows something)
    want = V.boundary(band_a, band_b, stitched=True)
    got = _boundary(grid_a.stack, grid_b.stack, d, _dev(nbr))
    assert (got == want).all(), (got, want)
    per_tile = _boundary(grid_a.stack, grid_b.stack, d)
    assert per_tile.shape == (4, 3) and (per_tile.sum(axis=0) != want[0]).any()


def test_the_raster_edge_is_no_boundary():
    mask = np.zeros((1, 12, 12), dtype=bool)
    mask[0, :6, :] = True  # touches three edges of the raster; the band at D = 1 is the row y = 5 alone
    assert _boundary(mask, mask, 1).tolist() == [[12, 12, 12]]
    full = np.ones((1, 12, 12), dtype=bool)
    assert _boundary(full, mask, 1).tolist() == [[0, 12, 0]]


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_anything_is_launched():
    u8 = torch.zeros((2, 7, 9), dtype=torch.uint8)
    i32 = torch.zeros((2, 7, 9), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="robosat_amd: .*MI355X"):
        ops.mask_confusion(u8, u8, 3)
    with pytest.raises(RuntimeError, match="robosat_amd: .*MI355X"):
        ops.boundary_counts(i32, i32, 3)
    with pytest.raises(ValueError, match="robosat_amd: .*are on"):
        ops.mask_confusion(u8.to("cuda:0"), u8, 3)
    gu8, gi32 = u8.to("cuda:0"), i32.to("cuda:0")
    with pytest.raises(ValueError, match="robosat_amd: .*both"):
        ops.mask_confusion(gu8, gu8[:1], 3)
    with pytest.raises(ValueError, match="robosat_amd: .*both"):
        ops.mask_confusion(gu8.view(2, 63), gu8.view(2, 63), 3)
    with pytest.raises(ValueError, match="robosat_amd: .*both"):
        ops.boundary_counts(gi32, gi32[:, :3], 3)
    for classes in (1, 9):
        with pytest.raises(ValueError, match="robosat_amd: 2 to 8 classes"):
            ops.mask_confusion(gu8, gu8, classes)
    for d in (0, 128):
        with pytest.raises(ValueError, match="robosat_amd: .*1..127"):
            ops.boundary_counts(gi32, gi32, d)
    with pytest.raises(TypeError, match="robosat_amd"):
        ops.mask_confusion(gi32, gi32, 3)
