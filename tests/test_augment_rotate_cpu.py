"""``[augment] rotate`` of ``rs train`` without a GPU: parsing and refusals (robosat_amd/augment.py, tools/train.py), the eighth draw
that is made only with the key, the float64 restatement (tests/augment_rotate_ref.py) against the integer maps' definitions in exact
fractions, the quarter turns, the mirror, and the entry point's declaration."""

import os
import random
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
import augment_rotate_ref as R  # noqa: E402
import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = {"zoom": 1.5, "brightness": [0.8, 1.2], "contrast": [0.8, 1.2], "saturation": [0.8, 1.2], "gamma": [0.8, 1.25]}
ALMOST = 1.0 - 2.0 ** -53  # the largest value random.random() returns


def _bands():
    from robosat_amd.bands import bands_from_config

    return bands_from_config({"common": {}})


# ---- config parsing ------------------------------------------------------------------------------------------------------------

def test_the_key_parses_and_an_absent_key_is_off():
    from robosat_amd.augment import Jitter, describe, jitter_from_config

    for value in (0, 45, 180):
        j = jitter_from_config({"augment": {"rotate": value}}, _bands())
        assert j.rotate == float(value) and isinstance(j.rotate, float)
    plain = jitter_from_config({"augment": dict(TABLE)}, _bands())
    assert plain.rotate == 0.0 and plain._fields[-1] == "rotate"
    assert Jitter(1.5, (0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (0.8, 1.25), True) == plain  # six values still build one
    assert describe(plain) == "zoom <= 1.5, brightness [0.8, 1.2], contrast [0.8, 1.2], saturation [0.8, 1.2], gamma [0.8, 1.25]"
    assert describe(plain._replace(rotate=0.0)) == describe(plain)
    turned = jitter_from_config({"augment": dict(TABLE, rotate=180)}, _bands())
    assert describe(turned) == describe(plain) + ", rotate <= 180 deg"
    assert describe(plain._replace(rotate=22.5)).endswith(", rotate <= 22.5 deg")


@pytest.mark.parametrize("value", [-1, 180.5, [0, 90], True, "45"])
def test_a_bad_angle_is_refused_with_the_key_in_the_message(value):
    from robosat_amd.augment import jitter_from_config

    with pytest.raises(ValueError, match=r"^\[augment\] rotate "):
        jitter_from_config({"augment": {"rotate": value}}, _bands())


def test_rs_train_refuses_a_bad_angle_and_the_host_pipeline(monkeypatch):
    from robosat_amd.tools.train import augment_options

    monkeypatch.delenv("ROBOSAT_TRAIN_HOST_PIPELINE", raising=False)
    assert augment_options({"augment": {"rotate": 30}}, {"common": {}}).rotate == 30.0
    with pytest.raises(SystemExit) as err:
        augment_options({"augment": dict(TABLE, rotate=270)}, {"common": {}})
    assert str(err.value).startswith("Error: [augment] rotate ")
    monkeypatch.setenv("ROBOSAT_TRAIN_HOST_PIPELINE", "1")
    with pytest.raises(SystemExit) as err:
        augment_options({"augment": {"rotate": 30}}, {"common": {}})
    assert str(err.value).startswith("Error: [augment] ") and "ROBOSAT_TRAIN_HOST_PIPELINE" in str(err.value)


# ---- draws -----------------------------------------------------------------------------------------------------------------------

def test_the_angle_is_an_eighth_draw_made_only_with_the_key(tmp_path):
    from robosat_amd import datasets as md
    from robosat_amd.augment import jitter_from_config

    size = 48
    root = synth.make_dataset(str(tmp_path / "ds"), n_train=3, n_val=1, size=64, seed=21)
    img, lab = os.path.join(root, "training", "images"), os.path.join(root, "training", "labels")
    tables = (dict(TABLE), dict(TABLE, rotate=0), dict(TABLE, rotate=180), {"rotate": 30})
    plain, zero, full, alone = (md.UnaugmentedTiles([img], lab, size, draw=True, jitter=jitter_from_config({"augment": t}, _bands()))
                                for t in tables)
    for i in range(len(plain)):
        random.seed(900 + i)
        expect = [random.random() for _ in range(13)]
        for ds in (plain, zero):  # without the key, or with 0: 4 + 7 draws and the six-entry item, as before
            random.seed(900 + i)
            item = ds[i]
            assert len(item) == 6 and random.random() == expect[11]
        random.seed(900 + i)
        u8, m8, code, geom, color, rot, tiles = full[i]
        assert random.random() == expect[12]  # 4 + 7 + 1
        assert code == item[2] and torch.equal(u8, item[0]) and torch.equal(m8, item[1]) and tiles == item[5]
        assert torch.equal(geom, item[3]) and torch.equal(color, item[4])  # what the same seed gives without the key
        assert rot.dtype == torch.int32 and tuple(rot.shape) == (2,)
        assert tuple(rot.tolist()) == R.rot_of((2.0 * expect[11] - 1.0) * 180.0)
        random.seed(900 + i)
        _, _, _, geom1, color1, rot1, _ = alone[i]  # the key alone: still the seven draws before it, everything else the identity
        assert random.random() == expect[12]
        assert geom1.tolist() == [size, 0, 0] and color1.tolist() == [1.0] * 4
        assert tuple(rot1.tolist()) == R.rot_of((2.0 * expect[11] - 1.0) * 30.0)


def test_the_angle_at_the_ends_of_the_draw():
    from robosat_amd.augment import rotation

    for limit in (180.0, 45.0, 0.5):
        for r_a in (0.0, 0.5, ALMOST):
            assert rotation(limit, r_a) == R.rot_of((2.0 * r_a - 1.0) * limit)
        assert rotation(limit, 0.5) == (65536, 0)
    assert rotation(180.0, 0.0) == (-65536, 0) and rotation(180.0, ALMOST) == (-65536, 0)
    assert rotation(90.0, 0.0) == (0, -65536) and rotation(180.0, 0.75) == (0, 65536)
    for r_a in np.linspace(0.0, ALMOST, 997):  # every pair the draw can give passes the entry point's test of a rotation
        c, s = rotation(180.0, float(r_a))
        assert abs(c) <= 65536 and abs(s) <= 65536 and abs(c * c + s * s - 2 ** 32) <= 2 ** 17


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def _windows(size):
    return sorted(set(A.corner_windows(size, 4)) | {(1, 0, 0), (1, size - 1, size - 1), (size, 0, 0)})


@pytest.mark.parametrize("size", [1, 5, 8, 33])
def test_the_integer_maps_are_the_definitions(size):
    for angle in (0, 7, -30, 45, 90, 133, -179.999, 180):
        rot = R.rot_of(angle)
        for geom in _windows(size):
            a, b = R.coefficients(size, geom[0], rot)
            assert (a, b) == R.coefficients_by_definition(size, geom[0], rot)
            ux, uy = R.positions(size, geom, rot)
            near_x, near_y = R.nearest_index(ux), R.nearest_index(uy)
            (xi, fx), (yi, fy) = R.bilinear_index(ux), R.bilinear_index(uy)
            for y in range(size):
                for x in range(size):
                    px, py = R.position_by_definition(x, y, size, geom, a, b)
                    assert Fraction(int(ux[y, x]), 2 ** 17) == px and Fraction(int(uy[y, x]), 2 ** 17) == py
                    assert (near_x[y, x], near_y[y, x]) == (R.nearest_by_definition(px), R.nearest_by_definition(py))
                    for i, f, p in ((xi, fx, px), (yi, fy, py)):
                        d0, df = R.bilinear_by_definition(p)
                        assert i[y, x] == d0 and f[y, x] == float(df) and 0.0 <= f[y, x] < 1.0
            for i in (near_x, near_y, xi, xi + 1, yi, yi + 1):
                folded = R.fold(i, size)
                assert folded.min() >= 0 and folded.max() <= size - 1
                assert all(folded.flat[k] == R.mirror_by_definition(int(i.flat[k]), size) for k in range(i.size))


def test_one_fold_is_enough_for_every_window_and_angle():
    """The extreme is the whole tile at 45 degrees, 0.21 S outside; no window at any angle comes near a second fold."""
    for size in (1, 2, 5, 8, 33, 96):
        for w in range(1, size + 1):
            for x0, y0 in ((0, 0), (size - w, size - w), (0, size - w)):
                for angle in np.linspace(-180.0, 180.0, 73):
                    lo, hi = R.sample_range(size, (w, x0, y0), R.rot_of(float(angle)))
                    assert -size <= lo and hi <= 2 * size - 1, (size, w, angle)


@pytest.mark.parametrize("size", [5, 8, 33])
@pytest.mark.parametrize("angle, turns", [(0, 0), (90, 1), (180, 2), (-90, -1), (-180, -2)])
def test_quarter_turns_of_the_whole_tile_are_rot90(size, angle, turns):
    images, masks = A.tiles(200 + size, 1, size, 3)
    rot = R.rot_of(angle)
    assert sorted(abs(v) for v in rot) == [0, 65536]
    ux, uy = R.positions(size, (size, 0, 0), rot)
    assert not R.bilinear_index(ux)[1].any() and not R.bilinear_index(uy)[1].any()
    zero, one = [0.0] * 3, [1.0] * 3
    for op in (0, 3):
        got_i, got_m = R.rotate(images[0], masks[0], op, (size, 0, 0), rot, A.IDENTITY_COLOR, zero, one, True)
        want_i, want_m = A.jitter(np.rot90(images[0], turns), np.rot90(masks[0], turns), op, (size, 0, 0), A.IDENTITY_COLOR, zero, one, True)
        assert np.array_equal(got_m, want_m) and np.array_equal(got_i, want_i)


def test_the_cases_of_the_gpu_tests_exercise_the_mirror_and_stay_in_the_tile():
    cases = dict(R.image_cases())
    assert len(cases) == 4 * 3 * 2 + 3
    assert {c["images"].shape[3] for c in cases.values()} == {1, 2, 3, 4} and {c["images"].shape[1] for c in cases.values()} == set(R.SIZES)
    seen = set()
    for case in cases.values():
        size = case["images"].shape[1]
        for n in range(8):
            geom, rot = case["geom"][n], case["rot"][n]
            seen.add((size, geom, rot))
            lo, hi = R.sample_range(size, geom, rot)
            assert -size <= lo and hi <= 2 * size - 1  # one fold lands in [0, S - 1]
            ux, uy = R.positions(size, geom, rot)
            for u in (ux, uy):
                for i in (R.nearest_index(u), R.bilinear_index(u)[0], R.bilinear_index(u)[0] + 1):
                    assert R.fold(i, size).min() >= 0 and R.fold(i, size).max() <= size - 1
    for size in R.SIZES:  # every angle with every window, at every size
        assert len({k for k in seen if k[0] == size}) >= 24
        # the whole tile at 45 degrees leaves the tile on all four sides, for the mask and for the image
        assert (size, (size, 0, 0), R.rot_of(45)) in seen
        ux, uy = R.positions(size, (size, 0, 0), R.rot_of(45))
        for u in (ux, uy):
            assert R.nearest_index(u).min() < 0 and R.nearest_index(u).max() > size - 1
            assert R.bilinear_index(u)[0].min() < 0 and R.bilinear_index(u)[0].max() + 1 > size - 1
    ux, uy = R.positions(96, (96, 0, 0), R.rot_of(45))
    outside = (R.nearest_index(ux) < 0) | (R.nearest_index(ux) > 95) | (R.nearest_index(uy) < 0) | (R.nearest_index(uy) > 95)
    assert 0.16 < outside.mean() < 0.18  # (the two squares share an octagon of 2 (sqrt 2 - 1) S^2: 17 % of the pixels are mirrored)


def test_the_restatement_turns_and_mirrors():
    """Values a hand can follow: at 0 degrees the rotation is the zoom's mask; a constant tile stays constant at any angle (the
    weights sum to one, the mirror adds nothing foreign); contrast 0 gives the SOURCE tile's band mean, not the turned window's."""
    size = 8
    images, masks = A.tiles(210, 1, size, 3)
    zero, one = [0.0] * 3, [1.0] * 3
    for geom in A.corner_windows(size, 4):
        for op in (0, 5):
            _, want_m = A.jitter(images[0], masks[0], op, geom, A.IDENTITY_COLOR, zero, one, True)
            _, got_m = R.rotate(images[0], masks[0], op, geom, (65536, 0), A.IDENTITY_COLOR, zero, one, True)
            assert np.array_equal(got_m, want_m)
    flat = np.full((size, size, 3), 100, dtype=np.uint8)
    img, _ = R.rotate(flat, masks[0], 2, (5, 1, 2), R.rot_of(37), A.IDENTITY_COLOR, zero, one, True)
    assert np.abs(img - 100.0 / 255).max() < 1e-15
    img, _ = R.rotate(images[0], masks[0], 0, (3, 0, 0), R.rot_of(45), (1.0, 0.0, 1.0, 1.0), zero, one, True)
    mean = images[0].reshape(-1, 3).astype(np.int64).sum(axis=0) / (size * size * 255.0)
    assert np.allclose(img, mean[:, None, None], rtol=0, atol=1e-15)
    # a positive angle turns the content counter-clockwise as displayed: a mark right of the centre moves up
    mark = np.zeros((9, 9), dtype=np.uint8)
    mark[4, 7] = 1
    _, msk = R.rotate(np.zeros((9, 9, 3), np.uint8), mark, 0, (9, 0, 0), R.rot_of(90), A.IDENTITY_COLOR, zero, one, True)
    assert msk[1, 4] == 1 and msk.sum() == 1


def test_the_chain_in_float32_stays_under_a_quarter_of_the_cap():
    """Whether the GPU tests' cap can be met at all: the same formulas in float32 numpy (rounded after every operation) against
    float64 on the cases the GPU tests run.  The GPU bound is four times what the kernel measures there and may not exceed 1e-5, so
    an fp32 chain has to stay under 2.5e-6."""
    worst = 0.0
    for _, case in R.image_cases():
        for n in range(len(case["index"])):
            wide, wide_mask = R.oracle(case, n)
            narrow, narrow_mask = R.oracle(case, n, dtype=np.float32)
            assert wide.dtype == np.float64 and narrow.dtype == np.float32 and np.array_equal(wide_mask, narrow_mask)
            worst = max(worst, float(np.abs(wide - narrow).max()))
    print("float32 numpy chain: largest |float32 - float64| = {:.3e}".format(worst))
    assert worst <= 2.5e-6


# ---- declarations ---------------------------------------------------------------------------------------------------------------

def test_header_and_ctypes_declare_the_entry_point():
    from robosat_amd import _lib

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    found = re.search(r"\bint rs_augment_tiles_rotate\(([^)]*)\)", header)
    assert found and len(found.group(1).split(",")) == 17
    assert "rs_augment_tiles_rotate" in _lib.SIGNATURES and len(_lib.SIGNATURES["rs_augment_tiles_rotate"][1]) == 17
    assert _lib.ABI_VERSION == 24  # (a new symbol, no old one changed)
