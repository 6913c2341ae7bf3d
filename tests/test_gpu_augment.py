"""The zoom and colour jitter of ``rs train`` on the MI355X (csrc/augment.hip: ``ops.tile_band_sums``, ``ops.augment_tiles_jitter``)
against numpy and the float64 restatement in tests/augment_ref.py, and the two device loaders with an ``[augment]`` table.

The image bound.  Measured on the MI355X over ``augment_ref.image_cases()`` plus the clamp and contrast-0 launches below: the largest
|kernel - float64| is 8.953e-07 (profiles/augment_jitter/README.md; the same chain in float32 numpy, rounded after every operation, is
1.0e-06 off on the same cases).  The bound is four times the measured figure -- the margin is for ``powf`` and fused multiply-adds on
other inputs -- and stays under the cap of 1e-5, itself under 0.1 % of one input byte's step after normalisation (1/255/0.229 =
1.7e-2)."""

import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = 8.953e-07
TOL = 4 * MEASURED
assert TOL <= 1e-5
TABLE = {"zoom": 1.5, "brightness": [0.8, 1.2], "contrast": [0.8, 1.2], "saturation": [0.8, 1.2], "gamma": [0.8, 1.25]}


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _launch(case):
    """One launch of the jitter kernel on a case of ``augment_ref``: (images fp32 [N,C,S,S], masks int64 [N,S,S]) as numpy."""
    from robosat_amd import ops

    images, masks = torch.from_numpy(case["images"]).to(DEV), torch.from_numpy(case["masks"]).to(DEV)
    out, om = ops.augment_tiles_jitter(images, masks, _i32(case["index"]), _i32(case["op"]), case["geom"], case["color"],
                                       ops.tile_band_sums(images), case["mean"], case["std"], case["rgb"])
    return out.cpu().numpy(), om.cpu().numpy()


def _oracle(case, n):
    i = case["index"][n]
    return A.jitter(case["images"][i], case["masks"][i], case["op"][n], case["geom"][n], case["color"][n], case["mean"], case["std"],
                    case["rgb"])


# ---- band sums -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t, s, c", [(1, 1, 1), (3, 5, 3), (2, 33, 4), (5, 64, 3), (4, 96, 2)])
def test_band_sums_equal_numpy(t, s, c):
    from robosat_amd import ops

    images, _ = A.tiles(10 + s, t, s, c)
    got = ops.tile_band_sums(torch.from_numpy(images).to(DEV))
    assert got.dtype == torch.int64 and tuple(got.shape) == (t, c)
    assert np.array_equal(got.cpu().numpy(), images.reshape(t, -1, c).astype(np.int64).sum(axis=1))


def test_band_sums_of_a_slice_whose_base_is_not_aligned():
    """Tiles 1.. of a larger tensor: the base is S*S*C = 75 (and 3267) bytes past an aligned address, and at 33 x 33 x 3 every tile
    after it starts at another residue of 16; the output is overwritten, not added to; two runs give the same bits."""
    from robosat_amd import ops

    for s, c in ((5, 3), (33, 3), (33, 1)):
        whole, _ = A.tiles(20 + s, 7, s, c)
        dev = torch.from_numpy(whole).to(DEV)
        part = dev[1:]
        assert part.is_contiguous() and (part.data_ptr() - dev.data_ptr()) % 16 != 0
        want = whole[1:].reshape(6, -1, c).astype(np.int64).sum(axis=1)
        first = ops.tile_band_sums(part)
        assert np.array_equal(first.cpu().numpy(), want)
        assert torch.equal(ops.tile_band_sums(part), first)
    big, _ = A.tiles(29, 2, 96, 3)  # one byte past an aligned base: a 16-byte head of 15 bytes, blocks that straddle both tiles
    flat = torch.zeros(big.size + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(big).to(DEV).reshape(-1)
    got = ops.tile_band_sums(flat[1:].view(2, 96, 96, 3))
    assert np.array_equal(got.cpu().numpy(), big.reshape(2, -1, 3).astype(np.int64).sum(axis=1))


# ---- identity ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [8, 33, 96])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_identity_parameters_reproduce_augment_tiles_bit_for_bit(s, c):
    from robosat_amd import ops

    images, masks = A.tiles(30 + s + c, 5, s, c)
    images, masks = torch.from_numpy(images).to(DEV), torch.from_numpy(masks).to(DEV)
    index, op = _i32([4, 0, 2, 2, 1, 3, 0, 4]), _i32(A.OPS)
    mean, std = A.BAND_MEAN[:c], A.BAND_STD[:c]
    want_i, want_m = ops.augment_tiles(images, masks, index, op, mean, std)
    geom, color = [(s, 0, 0)] * 8, [A.IDENTITY_COLOR] * 8
    for sums, rgb in ((ops.tile_band_sums(images), c >= 3), (None, False)):
        got_i, got_m = ops.augment_tiles_jitter(images, masks, index, op, geom, color, sums, mean, std, rgb)
        assert torch.equal(got_i, want_i) and torch.equal(got_m, want_m)
    got_i, got_m = ops.augment_tiles_jitter(images, None, index, op, geom, color, None, mean, std, False)
    assert got_m is None and torch.equal(got_i, want_i)


# ---- masks -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [8, 33, 96])
def test_masks_are_exactly_the_oracles_for_every_op_and_window(s, measured):
    images, masks = A.tiles(70 + s, 5, s, 3)
    windows = A.corner_windows(s, 4)
    wmin = -(-s // 4)
    assert windows[0] == (s, 0, 0) and windows[1] == (wmin, 0, 0) and windows[2] == (wmin, s - wmin, s - wmin)
    for k, win in enumerate(windows):
        case = A.make_case(images, masks, [4, 0, 2, 2, 1, 3, 0, 4], A.OPS, [win] * 8, [A.IDENTITY_COLOR] * 8, True)
        got_i, got_m = _launch(case)
        for n in range(8):
            want_i, want_m = _oracle(case, n)
            assert np.array_equal(got_m[n], want_m), (k, n)
            measured["masks-S{}-{}-{}".format(s, k, n)] = float(np.abs(got_i[n] - want_i).max())
            assert measured["masks-S{}-{}-{}".format(s, k, n)] <= TOL, (k, n)


# ---- images ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def measured():
    """The largest |kernel - float64| of every image comparison of this module, printed at the end (the figure of the README)."""
    worst = {}
    yield worst
    if worst:
        print("\naugment jitter: largest |kernel - float64| = {:.3e} ({}); bound {:.3e}".format(max(worst.values()), max(worst, key=worst.get), TOL))


@pytest.mark.parametrize("name", [name for name, _ in A.image_cases()])
def test_images_against_the_float64_oracle(name, measured):
    case = dict(A.image_cases())[name]
    got_i, got_m = _launch(case)
    errs = []
    for n in range(len(case["index"])):
        want_i, want_m = _oracle(case, n)
        errs.append(float(np.abs(got_i[n] - want_i).max()))
        assert np.array_equal(got_m[n], want_m), n
    measured[name] = max(errs)
    print("{}: largest |kernel - float64| per item {}".format(name, ["{:.2e}".format(e) for e in errs]))
    assert max(errs) <= TOL, errs
    if case["images"].shape[3] == 4:  # band 3 is no colour: the saturation stage leaves it alone
        still = dict(case, color=[(b, k, 1.0, g) for b, k, _, g in case["color"]])
        assert np.array_equal(_launch(still)[0][:, 3], got_i[:, 3]) and not np.array_equal(_launch(still)[0][:, :3], got_i[:, :3])


def test_more_items_than_one_launch_carries(measured):
    """70 items: the entry point carries 64 windows and factor sets per launch, so this is two launches; every item differs."""
    s, n_items = 8, 70
    images, masks = A.tiles(81, 5, s, 3)
    rng = np.random.default_rng(82)
    geom = []
    for _ in range(n_items):
        w = int(rng.integers(2, s + 1))
        geom.append((w, int(rng.integers(0, s - w + 1)), int(rng.integers(0, s - w + 1))))
    color = [tuple(lo + rng.random() * (hi - lo) for lo, hi in A.RANGES.values()) for _ in range(n_items)]
    case = A.make_case(images, masks, [int(v) for v in rng.integers(0, 5, n_items)], [int(v) for v in rng.integers(0, 8, n_items)], geom, color, True)
    got_i, got_m = _launch(case)
    errs = []
    for n in range(n_items):
        want_i, want_m = _oracle(case, n)
        errs.append(float(np.abs(got_i[n] - want_i).max()))
        assert np.array_equal(got_m[n], want_m), n
    measured["70-items"] = max(errs)
    assert max(errs) <= TOL, errs


def test_brightness_clamps_and_contrast_zero_is_the_band_mean(measured):
    s = 12
    white = np.full((1, s, s, 3), 255, dtype=np.uint8)
    images, masks = A.tiles(90, 1, s, 3)
    mean, std = A.BAND_MEAN[:3], A.BAND_STD[:3]
    case = A.make_case(np.concatenate([white, images]), np.concatenate([masks, masks]), [0, 1], [0, 5], [(s, 0, 0), (7, 2, 3)],
                   [(1.5, 1.0, 1.0, 1.0), (1.0, 0.0, 1.0, 1.0)], True)
    got_i, _ = _launch(case)
    top = (np.float32(1.0) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)  # 255 * 1.5 clamps to 1
    assert np.array_equal(got_i[0], np.broadcast_to(top[:, None, None], (3, s, s)))
    band_mean = images[0].reshape(-1, 3).astype(np.int64).sum(axis=0) / (s * s * 255.0)
    want = (band_mean - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert np.abs(got_i[1] - want[:, None, None]).max() <= TOL and np.ptp(got_i[1], axis=(1, 2)).max() == 0.0
    for n in range(2):
        measured["clamp-mean-{}".format(n)] = float(np.abs(got_i[n] - _oracle(case, n)[0]).max())
        assert measured["clamp-mean-{}".format(n)] <= TOL


# ---- launch errors ---------------------------------------------------------------------------------------------------------------

def test_launch_errors():
    from robosat_amd import ops

    s = 8
    images, masks = A.tiles(95, 2, s, 3)
    images, masks = torch.from_numpy(images).to(DEV), torch.from_numpy(masks).to(DEV)
    sums = ops.tile_band_sums(images)
    index, op, mean, std = _i32([0, 1]), _i32([0, 3]), A.BAND_MEAN[:3], A.BAND_STD[:3]
    ident = [A.IDENTITY_COLOR] * 2

    def run(geom, color=ident, im=images, su=sums, rgb=True, mean=mean, std=std):
        return ops.augment_tiles_jitter(im, masks, index, op, geom, color, su, mean, std, rgb)

    run([(s, 0, 0), (1, s - 1, s - 1)])  # the two extremes of a valid window
    for bad in ((0, 0, 0), (s + 1, 0, 0), (-1, 0, 0)):  # w outside [1, S]
        with pytest.raises(ValueError, match="RS_EINVAL"):
            run([(s, 0, 0), bad])
    for bad in ((4, 5, 0), (4, 0, 5), (4, -1, 0), (4, 0, -1), (s, 1, 0)):  # a window that leaves the tile
        with pytest.raises(ValueError, match="RS_EINVAL"):
            run([bad, (s, 0, 0)])
    five = torch.zeros((2, s, s, 5), dtype=torch.uint8, device=DEV)  # C > 4
    with pytest.raises(ValueError, match="RS_EINVAL"):
        run([(s, 0, 0)] * 2, im=five, su=None, rgb=False, mean=[0.5] * 5, std=[0.5] * 5)
    two = torch.zeros((2, s, s, 2), dtype=torch.uint8, device=DEV)  # rgb with fewer than three bands
    with pytest.raises(ValueError, match="RS_EINVAL"):
        run([(s, 0, 0)] * 2, im=two, su=None, rgb=True, mean=[0.5] * 2, std=[0.5] * 2)
    run([(s, 0, 0)] * 2, im=two, su=None, rgb=False, mean=[0.5] * 2, std=[0.5] * 2)
    with pytest.raises(ValueError, match="RS_EINVAL"):  # a contrast factor needs the band sums
        run([(s, 0, 0)] * 2, color=[A.IDENTITY_COLOR, (1.0, 0.9, 1.0, 1.0)], su=None)
    with pytest.raises(ValueError, match="RS_EINVAL"):
        ops.tile_band_sums(five)


# ---- loaders -----------------------------------------------------------------------------------------------------------------------

def test_the_two_device_loaders_jitter_alike_and_leave_validation_alone(tmp_path):
    """The shapes of test_device_augment_loader_reproduces_the_host_loader.  With the table and the same seeds the default loaders
    (workers decode and draw) and the cached ones (the loop draws) yield bit-equal training batches, twice over; their validation
    batches are those of a config without the table; a training batch is not the unjittered one."""
    from robosat_amd.tools.train import get_device_loaders, get_split_loaders

    ds_root = synth.make_dataset(str(tmp_path / "ds"), n_train=8, n_val=4, size=160, seed=4)
    plain = {"common": {"image_size": 128, "batch_size": 2}}
    model = dict(plain, augment=dict(TABLE))
    dataset = {"common": {"dataset": ds_root}}
    dev = torch.device(DEV)

    def batches(loader, seed):
        random.seed(seed)
        return [(im.clone(), mk.clone(), tl) for im, mk, tl in loader]

    split_train, split_val = get_split_loaders(model, dataset, 0, dev)
    cache_train, cache_val = get_device_loaders(model, dataset, dev)
    plain_train, plain_val = get_device_loaders(plain, dataset, dev)
    assert cache_train.cache.band_sums is not None and cache_val.cache.band_sums is None and plain_train.cache.band_sums is None
    want = batches(split_train, 123)
    assert len(want) == len(split_train) == 4
    for loader in (cache_train, split_train, cache_train):  # the other loader, and each a second time
        got = batches(loader, 123)
        assert len(got) == len(want)
        for (gi, gm, gt), (wi, wm, wt) in zip(got, want):
            assert gi.is_cuda and gi.dtype == torch.float32 and gm.dtype == torch.int64 and tuple(gi.shape) == (2, 3, 128, 128)
            assert torch.equal(gi, wi) and torch.equal(gm, wm)
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(batches(cache_train, 124), want))  # (another seed, other draws)
    unjittered = batches(plain_train, 123)  # (four draws per item instead of eleven: only the first item's view is the same)
    assert not torch.equal(unjittered[0][0], want[0][0])
    val = batches(plain_val, 5)  # (the validation loaders draw their four numbers per item too, as the reference's chain does)
    for loader in (split_val, cache_val):
        got = batches(loader, 5)
        assert len(got) == len(val) == 2
        for (gi, gm, _), (wi, wm, _) in zip(got, val):
            assert torch.equal(gi, wi) and torch.equal(gm, wm)
