"""``rs features --split`` on the MI355X: ``ops.split_seeds`` / ``ops.grow_labels`` / ``ops.split_labels`` (csrc/features.hip:
rs_features_split_cores, rs_features_split_seeds, rs_features_grow) against the restatement of tests/split_ref.py, exactly (the
rasters are integers): per tile, after a given number of steps around the kernel's block and apron borders, for every chunking and
every number of fused steps, and with the neighbour table on the ONE raster the tiles form (tests/stitch_ref.py)."""

import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import split_ref as P  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _same(got, want, what):
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert (got == want).all(), "{}: first difference at (tile, y, x) = {}".format(what, np.argwhere(got != want)[:1])


def _grow_once(raster, steps, nbr=None):
    """One call of the ABI on a copy of int32 [B, H, W]: (the raster after ``steps`` steps, counters)."""

    lab = _dev(raster.astype(np.int32))
    b, h, w = lab.shape
    ws = torch.empty(_lib.lib().rs_features_grow_workspace_bytes(b, h, w) // 4 + 1, device=lab.device, dtype=torch.int32)
    counters = torch.full((2,), -7, device=lab.device, dtype=torch.int32)
    rc = _lib.lib().rs_features_grow(ctypes.c_void_p(lab.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                     ctypes.c_void_p(nbr.data_ptr()) if nbr is not None else None, ctypes.c_void_p(counters.data_ptr()),
                                     b, h, w, steps, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return lab.cpu().numpy(), counters.tolist()


# ---- per tile ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 37, 53), (3, 64, 64), (2, 130, 70), (1, 200, 333), (2, 5, 70)]  # (the last: fewer rows than any number of fused steps)


@functools.lru_cache(maxsize=None)
def _masks(shape):
    b, h, w = shape
    return np.stack([P.touching_blobs(h, w, 10 * h + t, radius=(9, 6, 11)[t % 3]) for t in range(b)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _reference(shape, radius):
    """(L0, the final labels) of every tile, by the restatement."""

    starts = [P.start_of(m, radius) for m in _masks(shape)]
    return np.stack(starts).astype(np.int32), np.stack([P.grow(s) for s in starts]).astype(np.int32)


@pytest.mark.parametrize("radius", [1, 3, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_seeds_and_growth_are_the_restatement_exactly(shape, radius):
    masks = _masks(shape)
    start, final = _reference(shape, radius)
    if radius == 8 and shape[1] >= 37:
        assert (start == -1).any() and sum(len(np.unique(f)) for f in final) > sum(len(np.unique(R.label(m))) for m in masks), "something is split"
    cleaned = _dev(masks)
    labels = ops.label_components(cleaned)
    cores = ops.label_components(_dev(np.stack([P.seeds(m, radius) for m in masks]).astype(np.uint8)))
    got = ops.split_seeds(labels, cores)
    _same(got, start, "split_seeds")
    grown = ops.grow_labels(got)
    assert grown.data_ptr() == got.data_ptr(), "in place"
    _same(grown, final, "grow_labels")
    _same(ops.split_labels(cleaned, labels, radius), final, "split_labels")
    _same(labels, np.stack([R.label(m) for m in masks]), "the labels that went in are left alone")


def test_a_spiral_corridor_takes_hundreds_of_steps_and_many_chunks():
    mask = P.spiral_corridor()
    start = P.start_of(mask, 3)
    assert (start > 0).sum() == 1, "one seed pixel"
    want, steps = P.grow(start, want_steps=True)
    assert steps > 300
    got, enqueued = ops.grow_labels(_dev(start[None].astype(np.int32)), want_steps=True)
    assert steps <= enqueued < steps + ops.GROW_STEPS and enqueued // ops.GROW_STEPS >= 10
    _same(got, want[None], "spiral")
    cleaned = _dev(mask[None].astype(np.uint8))
    _same(ops.split_labels(cleaned, ops.label_components(cleaned), 3), want[None], "spiral, end to end")


def _probe_raster(bh, bw):
    """Two blocks either way and a little more, all unassigned but for a few holes."""

    h, w = 2 * bh + 5, 2 * bw + 7
    raster = np.full((h, w), -1, dtype=np.int64)
    raster[::7, 3::11] = 0
    return raster


def _probes():
    """(name, y, x) of single seeds whose front reaches, after exactly d = K - 1, K, K + 1 steps, the first row / column of the next
    block (`core`) or the outermost ring of that block's apron (`ring`), from either side."""

    bh, bw, k = ops.grow_config()
    out = []
    for d in (k - 1, k, k + 1):
        if d < 1:
            continue
        for name, y, x in (("core_from_w", bh + 2, bw - d), ("core_from_e", bh + 2, bw - 1 + d), ("core_from_n", bh - d, bw + 3),
                           ("core_from_s", bh - 1 + d, bw + 3), ("ring_from_w", bh + 2, bw - k - d), ("ring_from_n", bh - k - d, bw + 3),
                           ("ring_from_e", bh + 2, bw - 1 + k + d), ("ring_from_s", bh - 1 + k + d, bw + 3),
                           ("corner", bh - (d + 1) // 2, bw - d // 2)):
            if 0 <= y < 2 * bh + 5 and 0 <= x < 2 * bw + 7:
                out.append(("{}_{}".format(name, d - k), y, x, d))
    return out


def test_single_seeds_around_the_block_and_apron_borders_step_by_step():
    """The raster after exactly d - 1, d, d + 1 and 2 K + 1 steps (one call each, so one, two or three launches) is the
    restatement's: a front that arrives from the apron, or from beyond it, comes in neither early nor late."""

    bh, bw, k = ops.grow_config()
    base = _probe_raster(bh, bw)
    probes = _probes()
    assert len(probes) >= 9
    for name, y, x, d in probes:
        raster = base.copy()
        raster[y, x] = 5
        raster[raster.shape[0] - 1 - y, raster.shape[1] - 1 - x] = 9  # a second label from the opposite side: ties where they meet
        for steps in sorted({max(d - 1, 1), d, d + 1, 2 * k + 1}):
            want = P.grow(raster, steps=steps)
            got, counters = _grow_once(raster[None], steps)
            assert (got[0] == want).all(), "{} after {} steps: first difference at {}".format(name, steps, np.argwhere(got[0] != want)[:1])
            assert counters == [int((want > 0).sum()) - 2, int((want == -1).sum())], name


def test_the_chunking_and_the_number_of_fused_steps_do_not_change_a_pixel():
    bh, bw, k = ops.grow_config()
    start, final = _reference((2, 130, 70), 8)
    for steps in (1, 3, k, 1000):
        _same(ops.grow_labels(_dev(start), steps=steps), final, "steps = {}".format(steps))
    for fused in (1, 2, 5, 16):
        with ops.knob("grow_fused", fused):
            assert ops.grow_config() == (bh, bw, fused)
            _same(ops.grow_labels(_dev(start)), final, "fused = {}".format(fused))
            got, _ = _grow_once(start, 7)
        assert (got == np.stack([P.grow(s, steps=7) for s in start])).all(), "fused = {}, 7 steps".format(fused)
    assert ops.grow_config() == (bh, bw, k)


def test_a_converged_raster_is_left_as_it_is_and_both_counters_read_zero():
    _, final = _reference((3, 64, 64), 3)
    for steps in (1, 2, 40):
        got, counters = _grow_once(final, steps)
        assert (got == final).all() and counters == [0, 0]


def test_an_unreachable_pixel_is_an_error_return_not_a_spin():
    raster = np.zeros((1, 40, 70), dtype=np.int32)
    raster[0, 3:9, 3:9] = -1
    raster[0, 5, 5] = 12
    raster[0, 30, 60] = -1  # background all round it
    got, counters = _grow_once(raster, 64)
    want = raster.copy()
    want[0, 3:9, 3:9] = 12
    assert (got == want).all() and counters == [35, 1]
    got, counters = _grow_once(got, 64)
    assert (got == want).all() and counters == [0, 1]
    with pytest.raises(RuntimeError, match="no label reaches"):
        ops.grow_labels(_dev(raster))


def test_bad_arguments_raise_before_anything_is_launched():
    labels = torch.zeros((1, 8, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.grow_labels(labels)
    with pytest.raises(RuntimeError):
        ops.split_seeds(labels, labels)
    cleaned = torch.ones((1, 8, 8), dtype=torch.uint8, device="cuda:0")
    for radius in (0, 65, -1):
        with pytest.raises(ValueError):
            ops.split_labels(cleaned, labels.to("cuda:0"), radius)
    with pytest.raises(ValueError):
        ops.grow_labels(labels.to("cuda:0"), steps=0)
    with pytest.raises(ValueError):
        ops.split_seeds(labels.to("cuda:0"), torch.zeros((1, 8, 9), dtype=torch.int32, device="cuda:0"))


# ---- stitched ------------------------------------------------------------------------------------------------------------------------
def _disc(image, cy, cx, r):
    yy, xx = np.mgrid[:image.shape[0], :image.shape[1]]
    image[np.hypot(yy - cy, xx - cx) <= r] = 1


def _layouts():
    """name -> (image, tile height, tile width, absent positions)."""

    square = P.touching_blobs(64, 64, 3, radius=7).astype(np.uint8)
    _disc(square, 32, 32, 8)  # on the four-tile corner
    _disc(square, 31, 12, 7)  # on the seams
    _disc(square, 14, 32, 7)
    _disc(square, 50, 30, 7)
    row = P.touching_blobs(32, 96, 4, radius=7).astype(np.uint8)
    _disc(row, 16, 30, 8)  # cut by the seam to the absent tile: not eroded from there
    small = P.touching_blobs(48, 48, 5, radius=7).astype(np.uint8)
    tiny = P.touching_blobs(24, 28, 6, radius=6).astype(np.uint8)
    return {"2x2_of_32": (square, 32, 32, ()), "3x1_middle_absent": (row, 32, 32, ((1, 0),)), "3x3_of_16": (small, 16, 16, ()),
            "4x4_of_6x7": (tiny, 6, 7, ())}


LAYOUTS = _layouts()


@functools.lru_cache(maxsize=None)
def _grid(name):
    image, th, tw, absent = LAYOUTS[name]
    return S.Grid(S.split(image, th, tw, absent=absent), 0)


def _stitched(grid, radius):
    nbr, origin = (_dev(t) for t in grid.tables())
    cleaned = _dev(grid.stack)
    labels = ops.stitch_labels(ops.label_components(cleaned), nbr, inplace=True)
    return ops.split_labels(cleaned, labels, radius, nbr), nbr, origin


@pytest.mark.parametrize("radius", [2, 5])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_the_stitched_split_is_the_restatement_on_the_one_raster(name, radius):
    grid = _grid(name)
    want = P.split_stitched(grid, radius)
    got, nbr, _ = _stitched(grid, radius)
    _same(got, want, name)
    nbr_np, _ = grid.tables()
    start = P.start_stitched(grid, radius).astype(np.int32)
    assert (start == -1).any(), "something to grow"
    for fused in (1, 16):
        with ops.knob("grow_fused", fused):
            _same(ops.grow_labels(_dev(start), nbr, steps=3), want, "{}, fused = {}".format(name, fused))


@pytest.mark.parametrize("radius", [2, 5])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_the_stitched_partition_is_that_of_the_same_pixels_as_one_large_raster(name, radius):
    """Through the per-tile path the labels have other names: the map between the two label sets over all set pixels is a bijection,
    and the tables agree in areas and boxes.  (An absent tile is unknown to the seeds and unset on the large raster: the layout with
    one is compared with the objects near it cleared away, so that both mean the same.)"""

    image, th, tw, absent = LAYOUTS[name]
    image = image.copy()
    for c, r in absent:
        image[max(r * th - radius - 1, 0):(r + 1) * th + radius + 1, max(c * tw - radius - 1, 0):(c + 1) * tw + radius + 1] = 0
    grid = S.Grid(S.split(image, th, tw, absent=absent), 0)
    got, nbr, origin = _stitched(grid, radius)
    whole = _dev(grid.canvas[None].astype(np.uint8))
    large = ops.split_labels(whole, ops.label_components(whole), radius)
    a, b = grid.paste(got.cpu().numpy()), large.cpu().numpy()[0]
    assert ((a != 0) == (grid.canvas != 0)).all() and ((b != 0) == (grid.canvas != 0)).all()
    pairs = np.unique(np.stack([a[a != 0], b[a != 0]], axis=1), axis=0)
    assert len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])) and len(pairs) > 1
    stitched_rows = ops.component_table_stitched(got, origin).cpu().numpy()[:, 1:]
    large_rows = ops.component_table(large).cpu().numpy()[:, 2:]
    assert R.sort_rows(stitched_rows).tolist() == R.sort_rows(large_rows).tolist()
