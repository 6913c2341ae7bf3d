"""The ``[augment]`` table of ``rs train`` without a GPU: parsing and refusals (robosat_amd/augment.py, tools/train.py), the seven
draws per item behind the four of the flips and rotations, the float64 restatement (tests/augment_ref.py) against the integer maps'
definitions and, at identity, against the reference chain's CPU statement, and the two entry points' declarations."""

import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
TABLE = {"zoom": 1.5, "brightness": [0.8, 1.2], "contrast": [0.8, 1.2], "saturation": [0.8, 1.2], "gamma": [0.8, 1.25]}


def _bands(modes=None):
    from robosat_amd.bands import bands_from_config

    common = {} if modes is None else {"image_dirs": ["d{}".format(i) for i in range(len(modes))], "image_modes": modes}
    return bands_from_config({"common": common})


# ---- config parsing ------------------------------------------------------------------------------------------------------------

def test_the_table_parses_and_absent_keys_are_the_identity():
    from robosat_amd.augment import describe, jitter_from_config

    assert jitter_from_config({"common": {}}, _bands()) is None  # no table: nothing changes
    j = jitter_from_config({"augment": dict(TABLE)}, _bands())
    assert (j.zoom, j.brightness, j.contrast, j.saturation, j.gamma, j.rgb) == (1.5, (0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (0.8, 1.25), True)
    assert "zoom" in describe(j) and "gamma [0.8, 1.25]" in describe(j)
    j = jitter_from_config({"augment": {}}, _bands(["L"]))
    assert (j.zoom, j.brightness, j.contrast, j.saturation, j.gamma, j.rgb) == (1.0, (1.0, 1.0), (1.0, 1.0), (1.0, 1.0), (1.0, 1.0), False)
    assert jitter_from_config({"augment": {"saturation": [0.5, 1.5]}}, _bands(["RGBA"])).rgb
    assert jitter_from_config({"augment": {"saturation": [1, 1], "gamma": [2, 2]}}, _bands(["L", "L"])).gamma == (2.0, 2.0)


@pytest.mark.parametrize("table, modes, key", [
    ({"hue": [0.9, 1.1]}, None, "hue"),
    ({"zoom": 0.5}, None, "zoom"),
    ({"zoom": 4.5}, None, "zoom"),
    ({"zoom": [1, 2]}, None, "zoom"),
    ({"zoom": True}, None, "zoom"),
    ({"brightness": 1.2}, None, "brightness"),
    ({"brightness": [0.0, 1.2]}, None, "brightness"),
    ({"contrast": [1.2, 0.8]}, None, "contrast"),
    ({"contrast": [0.8, 1.0, 1.2]}, None, "contrast"),
    ({"gamma": [0.8, 4.5]}, None, "gamma"),
    ({"gamma": ["0.8", "1.2"]}, None, "gamma"),
    ({"saturation": [-1.0, 1.0]}, None, "saturation"),
    ({"saturation": [0.8, 1.2]}, ["L"], "saturation"),
    ({"saturation": [0.8, 1.2]}, ["L", "RGB"], "saturation"),
])
def test_a_bad_table_is_refused_with_the_key_in_the_message(table, modes, key):
    from robosat_amd.augment import jitter_from_config

    with pytest.raises(ValueError, match=r"^\[augment\] {} ".format(key)):
        jitter_from_config({"augment": table}, _bands(modes))


def test_rs_train_refuses_a_bad_table_and_the_host_pipeline(monkeypatch):
    from robosat_amd.tools.train import augment_options

    monkeypatch.delenv("ROBOSAT_TRAIN_HOST_PIPELINE", raising=False)
    assert augment_options({"common": {}}, {"common": {}}) is None
    assert augment_options({"augment": dict(TABLE)}, {"common": {}}).zoom == 1.5
    with pytest.raises(SystemExit) as err:
        augment_options({"augment": {"zoom": 9}}, {"common": {}})
    assert str(err.value).startswith("Error: [augment] zoom ")
    with pytest.raises(SystemExit) as err:
        augment_options({"augment": {"saturation": [0.5, 1.5]}}, {"common": {"image_dirs": ["ir"], "image_modes": ["L"]}})
    assert str(err.value).startswith("Error: [augment] saturation ")
    monkeypatch.setenv("ROBOSAT_TRAIN_HOST_PIPELINE", "1")
    assert augment_options({"common": {}}, {"common": {}}) is None  # (the host pipeline alone stays what it is)
    with pytest.raises(SystemExit) as err:
        augment_options({"augment": dict(TABLE)}, {"common": {}})
    assert str(err.value).startswith("Error: [augment] ") and "ROBOSAT_TRAIN_HOST_PIPELINE" in str(err.value)


# ---- draws -----------------------------------------------------------------------------------------------------------------------

def test_a_jittered_item_consumes_four_plus_seven_draws(tmp_path):
    from robosat_amd import datasets as md
    from robosat_amd.augment import jitter_from_config

    size = 48
    root = synth.make_dataset(str(tmp_path / "ds"), n_train=3, n_val=1, size=64, seed=21)
    img, lab = os.path.join(root, "training", "images"), os.path.join(root, "training", "labels")
    jit = jitter_from_config({"augment": dict(TABLE)}, _bands())
    only_gamma = jitter_from_config({"augment": {"gamma": TABLE["gamma"]}}, _bands())
    plain, full, part = (md.UnaugmentedTiles([img], lab, size, draw=True, jitter=j) for j in (None, jit, only_gamma))
    for i in range(len(plain)):
        random.seed(700 + i)
        expect = [random.random() for _ in range(12)]
        random.seed(700 + i)
        item = plain[i]
        assert len(item) == 4 and random.random() == expect[4]  # unjittered: the 4-tuple and four draws, as before
        random.seed(700 + i)
        u8, m8, code, geom, color, tiles = full[i]
        assert random.random() == expect[11]  # 4 + 7
        assert code == item[2] and torch.equal(u8, item[0]) and torch.equal(m8, item[1]) and tiles == item[3]
        assert geom.dtype == torch.int32 and tuple(geom.shape) == (3,) and color.dtype == torch.float32 and tuple(color.shape) == (4,)
        r = expect[4:11]  # r_w, r_x, r_y, r_b, r_k, r_s, r_g
        wmin = 32  # ceil(48 / 1.5)
        w = size - int(r[0] * (size - wmin + 1))
        assert geom.tolist() == [w, int(r[1] * (size - w + 1)), int(r[2] * (size - w + 1))]
        want = [lo + v * (hi - lo) for v, (lo, hi) in zip(r[3:], (jit.brightness, jit.contrast, jit.saturation, jit.gamma))]
        assert color.tolist() == [float(np.float32(v)) for v in want]
        # one key alone: still seven draws, the same r_g for gamma, everything else the identity
        random.seed(700 + i)
        _, _, _, geom1, color1, _ = part[i]
        assert random.random() == expect[11]
        assert geom1.tolist() == [size, 0, 0] and color1.tolist() == [1.0, 1.0, 1.0, color.tolist()[3]]


def test_the_window_at_the_ends_of_the_draws():
    from robosat_amd.augment import window

    almost = 1.0 - 2.0 ** -53  # the largest value random.random() returns
    for size, zoom, wmin in ((8, 4.0, 2), (33, 4.0, 9), (96, 4.0, 24), (512, 1.5, 342), (256, 1.0, 256), (100, 3.0, 34)):  # ceil(S / zoom)
        assert window(size, zoom, 0.0, 0.0, 0.0) == (size, 0, 0)
        w, x0, y0 = window(size, zoom, almost, 0.0, almost)
        assert w == wmin and x0 == 0 and y0 == size - w
        assert window(size, zoom, almost, almost, 0.0) == (wmin, size - wmin, 0)
        for r_w in np.linspace(0.0, almost, 23):
            w, x0, y0 = window(size, zoom, float(r_w), almost, almost)
            assert wmin <= w <= size and x0 == y0 == size - w  # never past the tile


# ---- the restatement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [1, 8, 33, 96])
def test_the_integer_maps_are_the_definitions(size):
    for w in sorted({1, max(1, size // 4), -(-size // 4), max(1, size // 2), max(1, size - 1), size}):
        near = A.nearest_index(size, w)
        i0, i1, f = A.bilinear_index(size, w)
        for j in range(size):
            assert near[j] == A.nearest_by_definition(j, w, size)
            d0, d1, df = A.bilinear_by_definition(j, w, size)
            assert (i0[j], i1[j]) == (d0, d1) and 0.0 <= f[j] < 1.0
            assert 0 <= i0[j] <= i1[j] <= w - 1 and 0 <= near[j] <= w - 1  # taps never leave the window
            if i1[j] == i0[j]:  # past the last centre: both taps on the last pixel, whatever the weight
                assert i0[j] == w - 1
            else:
                assert f[j] == float(df)
        if w == size:
            assert np.array_equal(i0, np.arange(size)) and not f.any() and np.array_equal(near, np.arange(size))


@pytest.mark.parametrize("bands", [3, 4])
def test_the_restatement_at_identity_is_the_reference_chain(bands):
    from oracle import tools_ref as T

    rng = np.random.default_rng(31 + bands)
    size = 20
    image = rng.integers(0, 256, size=(size, size, bands), dtype=np.uint8)
    mask = rng.integers(0, 3, size=(size, size), dtype=np.uint8)
    mean, std = (MEAN + [0.449])[:bands], (STD + [0.226])[:bands]
    draws = [[1, 1, 1, 1], [0, 1, 1, 1], [1, 0, 1, 1], [0, 0, 1, 1], [1, 0, 0, 1], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    codes = [int(d[0] < 0.5) + 2 * sum(v < 0.5 for v in d[1:]) for d in draws]
    assert sorted(codes) == list(range(8))
    for d, op in zip(draws, codes):
        want_i, want_m = T.augment(image, mask, d, mean, std)
        got_i, got_m = A.jitter(image, mask, op, (size, 0, 0), A.IDENTITY_COLOR, mean, std, rgb=bands >= 3, dtype=np.float32)
        assert got_i.dtype == np.float32 and np.array_equal(got_i, want_i) and np.array_equal(got_m, want_m), op
        wide, _ = A.jitter(image, mask, op, (size, 0, 0), A.IDENTITY_COLOR, mean, std, rgb=bands >= 3)
        assert wide.dtype == np.float64 and np.abs(wide - want_i).max() < 1e-6


def test_the_restatement_zooms_and_jitters():
    """Sanity of the float64 chain on values a hand can follow: a 2x zoom of a ramp stays a ramp, contrast 0 is the band mean,
    brightness clamps, saturation 0 is the luma on the colour bands and leaves band 3 alone."""
    size = 8
    ramp = np.tile((np.arange(size, dtype=np.uint8) * 10)[None, :, None], (size, 1, 4))
    ramp[..., 3] = 77
    mask = np.tile(np.arange(size, dtype=np.uint8)[None, :], (size, 1))
    zero, one = [0.0] * 4, [1.0] * 4
    img, msk = A.jitter(ramp, mask, 0, (4, 2, 2), A.IDENTITY_COLOR, zero, one, rgb=True)
    assert np.allclose(img[0, 0] * 255, np.clip(10 * (2 + (np.arange(size) + 0.5) / 2 - 0.5), 20, 50)) and msk[0].tolist() == [2, 2, 3, 3, 4, 4, 5, 5]
    img, _ = A.jitter(ramp, mask, 3, (size, 0, 0), (1.0, 0.0, 1.0, 1.0), zero, one, rgb=True)
    assert np.allclose(img[0], 35.0 / 255) and np.allclose(img[3], 77.0 / 255)
    img, _ = A.jitter(ramp, mask, 0, (size, 0, 0), (4.0, 1.0, 1.0, 1.0), zero, one, rgb=True)
    assert img.max() == 1.0 and img[0, 0, 0] == 0.0
    grey = ramp.copy()
    grey[..., 1] = 200
    img, _ = A.jitter(grey, mask, 0, (size, 0, 0), (1.0, 1.0, 0.0, 1.0), zero, one, rgb=True)
    assert np.allclose(img[0], img[1]) and np.allclose(img[1], img[2]) and np.allclose(img[3], 77.0 / 255)
    img, _ = A.jitter(grey, mask, 0, (size, 0, 0), (1.0, 1.0, 0.0, 1.0), zero, one, rgb=False)
    assert np.allclose(img[1], 200.0 / 255)  # (no RGB source: no saturation stage)


def test_the_chain_in_float32_stays_under_a_quarter_of_the_cap():
    """Whether the GPU tests' cap can be met at all: the same formulas in float32 numpy (rounded after every operation, numpy's
    power) against float64 on the cases the GPU tests run.  The GPU bound is four times what the kernel measures there and may not
    exceed 1e-5, so an fp32 chain has to stay under 2.5e-6; this one is 1.0e-6 off at the most."""
    worst = 0.0
    for _, case in A.image_cases():
        for n, i in enumerate(case["index"]):
            args = (case["images"][i], case["masks"][i], case["op"][n], case["geom"][n], case["color"][n], case["mean"], case["std"], case["rgb"])
            wide, wide_mask = A.jitter(*args)
            narrow, narrow_mask = A.jitter(*args, dtype=np.float32)
            assert np.array_equal(wide_mask, narrow_mask)
            worst = max(worst, float(np.abs(wide - narrow).max()))
    print("float32 numpy chain: largest |float32 - float64| = {:.3e}".format(worst))
    assert worst <= 2.5e-6


# ---- declarations ---------------------------------------------------------------------------------------------------------------

def test_header_and_ctypes_declare_the_two_entry_points():
    from robosat_amd import _lib

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    for name, count in (("rs_tile_band_sums", 6), ("rs_augment_tiles_jitter", 16)):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == count
    assert _lib.ABI_VERSION == 24  # (new symbols, no old one changed)
