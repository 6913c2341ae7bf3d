"""``rs evaluate --type --ignored unknown`` on the MI355X: ``ops.select_known`` (rs_eval_select), ``ops.boundary_counts`` with a coded
plane (rs_eval_boundary_coded) and the chain of stages behind the flag, against the numpy restatement (tests/eval_ignore_ref.py).
Every value is an integer, so every comparison is equality.  The shapes are the smallest at which these kernels can go wrong: one
pixel; runs that end inside a vector and groups smaller than a thread's run (7 x 9); group borders off every alignment (63 x 65);
exactly one block (64 x 64); a block of 4096 pixels that straddles two groups (48 x 48); many groups in one block (5 x 5).  Every
shape also runs as a view one element into its storage, where no address is 16-byte aligned."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edt_ref as E  # noqa: E402
import eval_ignore_ref as N  # noqa: E402
import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import evaluate as H  # noqa: E402
from robosat_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 7, 9), (2, 63, 65), (1, 64, 64), (3, 48, 48), (40, 5, 5)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
UNKNOWN = ["none", "all", "random", "first", "last"]
IGNORE = 255


def _dev(a, offset=0):
    """The array on the device; with ``offset`` as a contiguous view that many elements into a larger storage."""

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    if not offset:
        return t
    store = torch.zeros(t.numel() + 16, dtype=t.dtype, device="cuda:0")
    view = store[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == offset * t.element_size() and view.is_contiguous()
    return view


def _unknown(kind, shape, seed):
    u = np.zeros(shape, dtype=bool)
    if kind == "all":
        u[:] = True
    elif kind == "random":
        u = np.random.RandomState(seed).rand(*shape) < 0.1
    elif kind == "first":
        u.reshape(-1)[0] = True
    elif kind == "last":
        u.reshape(-1)[-1] = True
    return u


# ---- select_known --------------------------------------------------------------------------------------------------------------
def _select_cases(shape):
    """(C, cls, ignore, kind, p, a): random class bytes, in the mask also the ignore value, in the label also a byte that is
    neither a class nor the ignore value; then U."""

    for classes in (2, 8):
        for cls in sorted({1, classes - 1}):
            for ignore in (classes, 255):
                for k, kind in enumerate(UNKNOWN):
                    rng = np.random.RandomState(1000 * classes + 10 * cls + k + shape[2])
                    p = rng.randint(0, classes, size=shape).astype(np.uint8)
                    a = rng.randint(0, classes, size=shape).astype(np.uint8)
                    p[rng.rand(*shape) < 0.05] = ignore
                    a[rng.rand(*shape) < 0.05] = 200
                    a[_unknown(kind, shape, k)] = ignore
                    yield classes, cls, ignore, kind, p, a


def _check_select(got, p, a, cls, ignore, shape):
    want_p, want_g = N.coded(p, a, cls, ignore)
    for plane, want in zip(got, (want_p, want_g, want_p == E.SET, want_g == E.SET)):
        assert plane.dtype == torch.uint8 and tuple(plane.shape) == shape and plane.is_cuda and plane.is_contiguous()
        assert torch.equal(plane.cpu(), torch.from_numpy(want.astype(np.uint8)))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_select_known_is_the_coding_of_the_definition(shape, offset):
    for classes, cls, ignore, kind, p, a in _select_cases(shape):
        got = ops.select_known(_dev(p, offset), _dev(a, offset and 3), cls, ignore, classes)
        _check_select(got, p, a, cls, ignore, shape)
        if kind == "all":
            assert int(got[2].sum()) == 0 and int(got[3].sum()) == 0 and int((got[0] == 2).sum()) == p.size


@pytest.mark.parametrize("shape", [(3, 7, 9), (2, 63, 65), (1, 64, 64)], ids=["3x7x9", "2x63x65", "1x64x64"])
def test_select_writes_planes_at_odd_addresses_and_nothing_beside_them(shape):
    """The entry point itself, its four outputs one, two, three and five bytes into their storages: every store is the checked one,
    and the bytes before and behind a plane stay as they were."""

    classes, cls, ignore, _, p, a = list(_select_cases(shape))[-3]
    n = p.size
    stores = [torch.full((n + 32,), 77, dtype=torch.uint8, device="cuda:0") for _ in range(4)]
    views = [s[o:o + n] for s, o in zip(stores, (1, 2, 3, 5))]
    dp, da = _dev(p), _dev(a)
    ops._call("rs_eval_select", ops._dev(dp, "predicted", torch.uint8), ops._dev(da, "actual", torch.uint8),
              *[ops._dev(v, "out", torch.uint8) for v in views], n, classes, cls, ignore, ops._stream())
    _check_select([v.view(shape) for v in views], p, a, cls, ignore, shape)
    for s, o in zip(stores, (1, 2, 3, 5)):
        assert bool((s[:o] == 77).all()) and bool((s[o + n:] == 77).all())


def test_select_known_refuses_bad_arguments():
    u8 = torch.zeros((2, 7, 9), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="robosat_amd: .*MI355X"):
        ops.select_known(u8.cpu(), u8.cpu(), 1, 255, 2)
    with pytest.raises(ValueError, match="robosat_amd: .*both"):
        ops.select_known(u8, u8[:1], 1, 255, 2)
    with pytest.raises(TypeError, match="robosat_amd"):
        ops.select_known(u8.to(torch.int32), u8.to(torch.int32), 1, 255, 2)
    for ignore in (1, 256, None, True):
        with pytest.raises(ValueError, match="robosat_amd"):
            ops.select_known(u8, u8, 1, ignore, 2)
    for index in (0, 2, -1):
        with pytest.raises(ValueError, match="robosat_amd: the class to select"):
            ops.select_known(u8, u8, index, 255, 2)
    for classes in (1, 9):
        with pytest.raises(ValueError, match="robosat_amd: 2 to 8 classes"):
            ops.select_known(u8, u8, 1, 255, classes)
    i32 = torch.zeros((2, 7, 9), dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="robosat_amd: coded"):
        ops.boundary_counts(i32, i32, 1, coded=u8[:1])
    with pytest.raises(TypeError, match="robosat_amd"):
        ops.boundary_counts(i32, i32, 1, coded=i32)


# ---- boundary_counts with a coded plane ----------------------------------------------------------------------------------------
def _pattern(name, h, w, seed):
    if name == "blobs":
        return R.blobs(h, w, seed)
    if name == "checkerboard":
        return R.checkerboard(h, w) if seed % 2 else ~R.checkerboard(h, w)
    m = np.zeros((h, w), dtype=bool)  # comb: a spine along the top (seed odd) or bottom row, every other column a tooth
    m[0 if seed % 2 else -1, :] = True
    m[:, seed % 2::2] = True
    return m


_BANDS = {}


def _band_cases(shape):
    """[(name, kind, d, p, a, the restatement's int64 [B, 3])] of a shape, computed once and left unchanged."""

    if shape not in _BANDS:
        b, h, w = shape
        cases = []
        for name in ("blobs", "comb", "checkerboard"):
            p = np.stack([_pattern(name, h, w, 2 * i + 1) for i in range(b)]).astype(np.uint8)
            a = np.stack([np.roll(_pattern(name, h, w, 2 * i + (1 if name == "blobs" else 2)), (1, 2) if name == "blobs" else (0, 0), axis=(0, 1))
                          for i in range(b)]).astype(np.uint8)
            for k, kind in enumerate(UNKNOWN):
                label = np.where(_unknown(kind, shape, 20 + k), IGNORE, a).astype(np.uint8)
                cp, cg = N.coded(p, label, 1, IGNORE)
                for d in (1, 3):
                    cases.append((name, kind, d, p, label, N.band_counts(cp, cg, d)))
        _BANDS[shape] = cases
    return _BANDS[shape]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_coded_band_counts_are_the_restatement(shape, offset):
    seen = 0
    for name, kind, d, p, label, want in _band_cases(shape):
        coded_p, coded_g, _, _ = ops.select_known(_dev(p), _dev(label), 1, IGNORE, 2)
        d2_p = _dev(ops.distance_transform(coded_p, d + 1).cpu().numpy(), offset)
        d2_g = _dev(ops.distance_transform(coded_g, d + 1).cpu().numpy(), offset)
        coded = _dev(coded_g.cpu().numpy(), offset)
        got = ops.boundary_counts(d2_p, d2_g, d, coded=coded)
        assert got.dtype == torch.int64 and tuple(got.shape) == (shape[0], 3) and got.is_cuda
        assert (got.cpu().numpy() == want).all(), (name, kind, d, got.cpu().numpy(), want)
        whole = ops.boundary_counts(d2_p, d2_g, d, stitched=True, coded=coded)
        assert tuple(whole.shape) == (1, 3) and (whole.cpu().numpy()[0] == want.sum(axis=0)).all(), (name, kind, d)
        assert torch.equal(ops.boundary_counts(d2_p, d2_g, d, coded=coded_p), got)  # U is the same in both planes: either serves
        if kind == "all":
            assert not want.any()
        if kind == "none":  # a plane without a 2: the counts of the entry point without one
            assert torch.equal(got, ops.boundary_counts(d2_p, d2_g, d))
        if kind == "random" and shape[1] * shape[2] >= 63 * 65:
            # the transform writes a distance at unknown pixels, so the count without the plane is another: the plane has a say
            seen += int(not torch.equal(got, ops.boundary_counts(d2_p, d2_g, d)))
    assert seen or shape[1] * shape[2] < 63 * 65


# ---- the whole chain -----------------------------------------------------------------------------------------------------------
def _boxes(h, w, seed):
    """(p, a) uint8 [h, w]: class 1 = five boxes and a road, the prediction the label moved by (1, 1) with a box more."""

    rng = np.random.RandomState(seed)
    g = np.zeros((h, w), dtype=bool)
    for _ in range(5):
        y, x = rng.randint(0, h - 4), rng.randint(0, w - 4)
        g[y:y + rng.randint(3, 8), x:x + rng.randint(3, 8)] = True
    g |= T.roads(h, w, seed, count=1, width=3)
    p = np.roll(g, (1, 1), axis=(0, 1))
    y, x = rng.randint(0, h - 4), rng.randint(0, w - 4)
    p[y:y + 4, x:x + 4] = True
    return p.astype(np.uint8), g.astype(np.uint8)


def _chain(p, a, d, rhos, threshold, min_area=0, nbr=None, origin=None, classes=2, index=1):
    """The stages of ``Evaluation.add`` behind the flag -> (band counts summed, (matched, predicted, actual, IoUs), {rho: the eight
    counts summed})."""

    stitched = nbr is not None
    coded_p, coded_g, mask_p, mask_g = ops.select_known(_dev(p), _dev(a), index, IGNORE, classes)
    d2_p, d2_g = ops.distance_transform(coded_p, d + 1, nbr), ops.distance_transform(coded_g, d + 1, nbr)
    band = ops.boundary_counts(d2_p, d2_g, d, stitched=stitched, coded=coded_g).cpu().numpy().sum(axis=0).tolist()
    labels_p, labels_g = ops.label_components(mask_p), ops.label_components(mask_g)
    if stitched:
        labels_p, labels_g = ops.stitch_labels(labels_p, nbr, inplace=True), ops.stitch_labels(labels_g, nbr, inplace=True)
        table_p, table_g = ops.component_table_stitched(labels_p, origin, min_area), ops.component_table_stitched(labels_g, origin, min_area)
    else:
        table_p, table_g = ops.component_table(labels_p, min_area), ops.component_table(labels_g, min_area)
    pairs = ops.overlap_table(labels_p, labels_g, stitched=stitched)
    matched, predicted, actual, ious = H.match_objects(table_p.cpu().numpy(), table_g.cpu().numpy(), pairs.cpu().numpy(), threshold, stitched)
    skel_p, skel_g = ops.thin_masks(mask_p, nbr), ops.thin_masks(mask_g, nbr)
    links = {rho: ops.centerline_counts(skel_p, skel_g, rho, nbr).cpu().numpy().sum(axis=0).tolist() for rho in rhos}
    return band, (matched, predicted, actual, sorted(ious)), links


def _want_tiles(p, a, d, rhos, threshold, min_area=0, index=1):
    cp, cg = N.coded(p, a, index, IGNORE)
    return (N.band_counts(cp, cg, d).sum(axis=0).tolist(), N.objects(cp, cg, threshold, min_area),
            {rho: np.array(N.centerline_counts(cp, cg, rho)).sum(axis=0).tolist() for rho in rhos})


def _want_grid(tiles_p, tiles_a, d, rhos, threshold, index=1):
    """The restatement on the canvas the tiles form, and the tables of the stitched call."""

    coded = {key: N.coded(tiles_p[key], tiles_a[key], index, IGNORE) for key in tiles_p}
    gp, gg = N.grid({k: c[0] for k, c in coded.items()}), N.grid({k: c[1] for k, c in coded.items()})
    want = (N.band_counts_grid(gp, gg, d).tolist(), N.objects_grid(gp, gg, threshold), {rho: N.centerline_counts_grid(gp, gg, rho) for rho in rhos})
    return want, gp


def _stitched_chain(tiles_p, tiles_a, d, rhos, threshold, index=1, classes=2):
    want, grid = _want_grid(tiles_p, tiles_a, d, rhos, threshold, index)
    nbr, origin = grid.tables()
    keys = grid.coords
    got = _chain(np.stack([tiles_p[k] for k in keys]), np.stack([tiles_a[k] for k in keys]), d, rhos, threshold, nbr=_dev(nbr), origin=_dev(origin),
                 classes=classes, index=index)
    return got, want


def _same(got, want):
    assert got[0] == want[0], (got[0], want[0])
    # (an IoU comes back as the float nearest its fraction: compared as that float, or as the other call's floats)
    assert got[1][:3] == want[1][:3] and got[1][3] == sorted(float(f) for f in want[1][3]), (got[1], want[1])
    assert got[2] == want[2], (got[2], want[2])


def test_the_chain_per_tile_equals_the_restatement():
    """Three tiles of 31 x 33, three classes, the class scored is 2: ignored rectangles that cut an object, swallow a predicted one
    whole, and a tile without any."""

    pairs = [_boxes(31, 33, seed) for seed in (2, 3, 5)]
    p = np.stack([2 * pair[0] for pair in pairs]).astype(np.uint8)
    a = np.stack([2 * pair[1] for pair in pairs]).astype(np.uint8)
    p[0, 20:24, 2:6] = 1  # the other class: in no mask
    p[1, 25:29, 25:30] = 2
    a[0, 8:20, 10:22] = IGNORE
    a[1, 24:30, 24:31] = IGNORE  # swallows the predicted box above
    a[1, :, 15] = IGNORE  # a line of ignored pixels from edge to edge: every object across it is two
    want = _want_tiles(p, a, 3, (1, 3), 0.5, index=2)
    _same(_chain(p, a, 3, (1, 3), 0.5, classes=3, index=2), want)
    plain = _want_tiles(p, np.where(a == IGNORE, 0, a), 3, (1, 3), 0.5, index=2)
    assert want[0] != plain[0] and want[1][:3] != plain[1][:3] and want[2] != plain[2]  # (the ignored pixels have a say in every view)
    assert want[0][2] > 0 and want[1][0] > 0 and want[2][3][2] > 0
    _same(_chain(p, a, 1, (1,), 0.25, min_area=6, classes=3, index=2), _want_tiles(p, a, 1, (1,), 0.25, min_area=6, index=2))


def _grid_scene():
    p, a = _boxes(32, 32, 5)
    a[10:22, 13:19] = IGNORE  # across the vertical seam x = 16, through whatever lies there
    a[14:18, 0:32] = IGNORE   # and across the horizontal one
    p[11:14, 14:18] = 1       # a predicted object wholly inside U
    return p, a


def test_the_chain_stitched_equals_the_restatement_with_a_tile_absent_and_u_across_a_seam():
    p, a = _grid_scene()
    absent = {(1, 0)}
    tiles_p, tiles_a = S.split(p, 16, 16, absent=absent, x0=7, y0=3), S.split(a, 16, 16, absent=absent, x0=7, y0=3)
    got, want = _stitched_chain(tiles_p, tiles_a, 3, (1, 3), 0.5)
    _same(got, want)
    assert want[0][2] > 0 and want[1][1] > 0 and want[2][3][0] > 0
    known = {k: np.where(v == IGNORE, 0, v) for k, v in tiles_a.items()}
    assert _want_grid(tiles_p, known, 3, (1, 3), 0.5)[0] != want
    per_tile = _chain(np.stack([tiles_p[k] for k in sorted(tiles_p)]), np.stack([tiles_a[k] for k in sorted(tiles_a)]), 3, (1, 3), 0.5)
    _same(per_tile, _want_tiles(np.stack([tiles_p[k] for k in sorted(tiles_p)]), np.stack([tiles_a[k] for k in sorted(tiles_a)]), 3, (1, 3), 0.5))


# ---- what "unknown" means, on the device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 11])
def test_an_ignored_strip_counts_what_the_raster_without_it_does(k):
    p, a = _boxes(24, 32, 3)
    a_cut = a.copy()
    a_cut[:, -k:] = IGNORE
    p_noise = p.copy()
    p_noise[::2, -k:] = 1
    full = _chain(p_noise[None], a_cut[None], 3, (2,), 0.5)
    narrow = _chain(np.ascontiguousarray(p[None, :, :-k]), np.ascontiguousarray(a[None, :, :-k]), 3, (2,), 0.5)
    _same(full, narrow)
    _same(full, _want_tiles(p_noise[None], a_cut[None], 3, (2,), 0.5))
    assert full[0][2] > 0 and full[1][0] > 0 and full[2][2][0] > 0


@pytest.mark.parametrize("tile", [(0, 0), (1, 1)])
@pytest.mark.parametrize("d", [3, 15])
def test_a_wholly_ignored_tile_counts_what_the_grid_without_it_does(tile, d):
    p, a = _boxes(32, 32, 5)
    tiles_p, tiles_a = S.split(p, 16, 16), S.split(a, 16, 16)
    ignored = dict(tiles_a)
    ignored[tile] = np.full_like(tiles_a[tile], IGNORE)
    with_ignored, want = _stitched_chain(tiles_p, ignored, d, (d,), 0.5)
    without, _ = _stitched_chain({k: v for k, v in tiles_p.items() if k != tile}, {k: v for k, v in tiles_a.items() if k != tile}, d, (d,), 0.5)
    _same(with_ignored, without)
    _same(with_ignored, want)
    assert with_ignored[0][2] > 0 and with_ignored[1][1] > 0 and with_ignored[2][d][0] > 0


# ---- without an ignored pixel the flagged path is the unflagged one ------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_without_ignored_pixels_every_output_is_the_unflagged_paths(shape, offset):
    b, h, w = shape
    rng = np.random.RandomState(h + w)
    p = np.where(np.stack([R.blobs(h, w, i) for i in range(b)]), 2, rng.randint(0, 2, size=shape)).astype(np.uint8)
    a = np.where(np.stack([R.blobs(h, w, 40 + i) for i in range(b)]), 2, rng.randint(0, 2, size=shape)).astype(np.uint8)
    dp, da = _dev(p, offset), _dev(a, offset)
    coded_p, coded_g, mask_p, mask_g = ops.select_known(dp, da, 2, IGNORE, 3)
    clean_p, clean_g = ops.clean_masks(_dev(p), 2, 0, 0), ops.clean_masks(_dev(a), 2, 0, 0)
    assert torch.equal(mask_p, clean_p) and torch.equal(mask_g, clean_g) and torch.equal(coded_p, clean_p) and torch.equal(coded_g, clean_g)
    for d in (1, 3):
        d2_p, d2_g = ops.distance_transform(coded_p, d + 1), ops.distance_transform(coded_g, d + 1)
        assert torch.equal(d2_p, ops.distance_transform(clean_p, d + 1)) and torch.equal(d2_g, ops.distance_transform(clean_g, d + 1))
        for stitched in (False, True):
            assert torch.equal(ops.boundary_counts(d2_p, d2_g, d, stitched=stitched, coded=coded_g),
                               ops.boundary_counts(d2_p, d2_g, d, stitched=stitched))
