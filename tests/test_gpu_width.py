"""``ops.distance_transform`` (rs_features_edt) on the MI355X against the restatement of tests/edt_ref.py, exactly (the results are
integers): per tile, and with the neighbour table on the ONE raster the tiles form (tests/stitch_ref.py, absent tiles unknown)."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edt_ref as E  # noqa: E402
import stitch_ref as S  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _check(masks, radius):
    """Every tile of uint8 [B, H, W] against the restatement."""

    got = ops.distance_transform(_dev(masks), radius)
    assert got.dtype == torch.int32 and got.shape == masks.shape
    want = torch.from_numpy(np.stack([E.edt(m, radius) for m in masks]).astype(np.int32))
    assert torch.equal(got.cpu(), want), "first difference at (tile, y, x) = {}".format(np.argwhere(got.cpu().numpy() != want.numpy())[:1])
    return got


def _three(h, w, seed):
    """B = 3: 90 % noise, roads (set bytes of 255: non-zero is set), and a full tile with a single hole off-centre."""

    rng = np.random.RandomState(seed)
    full = np.ones((h, w), np.uint8)
    full[h // 3, (2 * w) // 3] = 0
    return np.stack([(rng.rand(h, w) < 0.9).astype(np.uint8), T.roads(h, w, seed, width=9).astype(np.uint8) * 255, full])


@pytest.mark.parametrize("radius", [1, 7, 128])
def test_a_tile_narrower_than_a_wave_and_than_the_radius(radius):
    """70 x 45: W < 64 and no multiple of 32; R = 128 exceeds both sides."""

    _check(_three(70, 45, 0), radius)


def test_single_pixels():
    masks = np.array([1, 0, 7], np.uint8).reshape(3, 1, 1)
    for radius in (1, 5, 128):
        got = _check(masks, radius)
        assert got.flatten().tolist() == [radius * radius, 0, radius * radius], "nothing unset anywhere: capped"


def test_all_ones_is_the_cap_everywhere_and_all_zeros_is_zero():
    got = _check(np.ones((3, 64, 64), np.uint8), 34)
    assert (got == 34 * 34).all()
    got = _check(np.zeros((3, 64, 64), np.uint8), 34)
    assert (got == 0).all()


@pytest.mark.parametrize("radius", [34, 128])
def test_roads_across_the_strip_and_row_block_edges(radius):
    """130 x 257: five 64-column strips, the last one pixel wide, and three blocks of rows."""

    _check(_three(130, 257, 1), radius)


def test_two_tiles_of_512_at_the_command_lines_default_radius():
    _check(np.stack([T.roads(512, 512, seed, count=6, width=21) for seed in (2, 3)]).astype(np.uint8), 34)


def test_a_tile_does_not_depend_on_the_batch_it_travels_in():
    masks = _three(70, 45, 4)
    assert torch.equal(ops.distance_transform(_dev(masks[:1]), 7)[0], ops.distance_transform(_dev(masks), 7)[0])


# ---- stitched ----------------------------------------------------------------------------------------------------------------------
TH, TW = 48, 40


@pytest.fixture(scope="module")
def hole_grid():
    """3 x 3 tiles of 48 x 40, the centre and the bottom right corner absent."""

    h, w = 3 * TH, 3 * TW
    yy, xx = np.mgrid[:h, :w]
    m = np.hypot(yy - TH + 0.5, xx - TW + 0.5) <= 15  # a blob over the four-tile corner of (0, 0), (1, 0), (0, 1) and the absent centre
    m |= np.abs(yy - 14) <= 5  # a road through the three tiles of the first row
    m |= np.abs((xx - 100) * np.sin(1.1) - (yy - 60) * np.cos(1.1)) <= 4  # and one down the right column
    m[TH:2 * TH, :TW] = True  # tile (0, 1), beside the absent centre, is all ones
    m[2 * TH:, TW:2 * TW] = np.random.RandomState(5).rand(TH, TW) < 0.97  # (1, 2): below the centre, unset pixels near its corners too
    return S.Grid(S.split(m.astype(np.uint8), TH, TW, absent=[(1, 1), (2, 2)]), 0)


def _check_stitched(grid, radius):
    nbr, _ = grid.tables()
    got = ops.distance_transform(_dev(grid.stack), radius, _dev(nbr)).cpu()
    want = torch.from_numpy(E.edt_stitched(grid, radius).astype(np.int32))
    assert torch.equal(got, want), "first difference at (slot, y, x) = {}".format(np.argwhere(got.numpy() != want.numpy())[:1])
    return got.numpy()


@pytest.mark.parametrize("radius", [5, 40])
def test_the_stitched_transform_is_the_transform_of_the_one_raster(hole_grid, radius):
    got = _check_stitched(hole_grid, radius)
    full = hole_grid.coords.index((0, 1))
    assert (hole_grid.stack[full] == 1).all()
    alone = E.edt(hole_grid.stack[full], radius)
    assert (alone == radius * radius).all() and (got[full] < radius * radius).any(), "its distances come from its present neighbours"
    assert (got[full][:, TW - 1] == radius * radius)[radius:TH - radius].all(), "and none from the absent centre beside it"


def test_a_radius_beyond_the_tiles_smaller_side_is_refused_with_the_table(hole_grid):
    nbr, _ = hole_grid.tables()
    with pytest.raises(ValueError):
        ops.distance_transform(_dev(hole_grid.stack), 41, _dev(nbr))
    ops.distance_transform(_dev(hole_grid.stack), 41)  # (per tile any radius up to 128 goes)


def test_small_random_grids_with_absent_tiles():
    """Tiles of 9 x 7 and 5 x 70, every radius up to the smaller side: rows of absent tiles above and below are filled from the
    corner tiles, W is no multiple of anything."""

    rng = np.random.RandomState(6)
    for th, tw in ((9, 7), (5, 70)):
        for _ in range(4):
            image = (rng.rand(3 * th, 3 * tw) < 0.92).astype(np.uint8)
            absent = [(c, r) for c in range(3) for r in range(3) if rng.rand() < 0.35][:8]
            grid = S.Grid(S.split(image, th, tw, absent=absent), 0)
            for radius in (1, min(th, tw) // 2, min(th, tw)):
                _check_stitched(grid, radius)


# ---- the rest of the boundary ----------------------------------------------------------------------------------------------------
def test_sample_pixels_is_numpy_indexing():
    rng = np.random.RandomState(7)
    raster = rng.randint(0, 1 << 14, (3, 20, 33)).astype(np.int32)
    coords = np.stack([rng.randint(0, 3, 500), rng.randint(0, 20, 500), rng.randint(0, 33, 500)], axis=1).astype(np.int32)
    got = ops.sample_pixels(_dev(raster), _dev(coords))
    assert got.dtype == torch.int32 and got.is_cuda
    assert (got.cpu().numpy() == raster[coords[:, 0], coords[:, 1], coords[:, 2]]).all()
    assert ops.sample_pixels(_dev(raster), _dev(coords[:0])).shape == (0,)


def test_bad_arguments_raise_before_anything_is_launched():
    masks = torch.ones((1, 8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.distance_transform(masks, 4)
    with pytest.raises(RuntimeError):
        ops.sample_pixels(torch.zeros((1, 8, 8), dtype=torch.int32), torch.zeros((1, 3), dtype=torch.int32))
    for radius in (0, 129, -1):
        with pytest.raises(ValueError):
            ops.distance_transform(masks.to("cuda:0"), radius)
