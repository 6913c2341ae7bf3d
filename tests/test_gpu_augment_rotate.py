"""The free rotation of ``rs train`` on the MI355X (csrc/augment.hip: ``ops.augment_tiles_rotate``) against the float64 restatement
in tests/augment_rotate_ref.py and against the jitter kernel on tiles turned on the host, and the two device loaders with
``[augment] rotate``.

The image bound.  Measured on the MI355X over ``augment_rotate_ref.image_cases()`` plus the 0-degree and the 70-item launches below:
the largest |kernel - float64| is 1.046e-06 (`all-S96-2`, item 4; profiles/augment_rotate/README.md; the same chain in float32
numpy, rounded after every operation, is 1.046e-06 off on the image cases too).  The bound is four times the measured figure -- the margin the jitter
module takes for ``powf`` and fused multiply-adds on other inputs -- and stays under the project's cap of 1e-5.  Masks are exact."""

import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
import augment_rotate_ref as R  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = 1.046e-06
TOL = 4 * MEASURED
assert TOL <= 1e-5
TABLE = {"zoom": 1.5, "brightness": [0.8, 1.2], "contrast": [0.8, 1.2], "saturation": [0.8, 1.2], "gamma": [0.8, 1.25]}


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _launch(case):
    """One call of the rotate entry point on a case of ``augment_rotate_ref``: (images fp32 [N,C,S,S], masks int64 [N,S,S]) as numpy."""
    from robosat_amd import ops

    images, masks = torch.from_numpy(case["images"]).to(DEV), torch.from_numpy(case["masks"]).to(DEV)
    out, om = ops.augment_tiles_rotate(images, masks, _i32(case["index"]), _i32(case["op"]), case["geom"], case["rot"], case["color"],
                                       ops.tile_band_sums(images), case["mean"], case["std"], case["rgb"])
    return out.cpu().numpy(), om.cpu().numpy()


@pytest.fixture(scope="module")
def measured():
    """The largest |kernel - float64| of every image comparison of this module, printed at the end (the figure of the README)."""
    worst = {}
    yield worst
    if worst:
        print("\naugment rotate: largest |kernel - float64| = {:.3e} ({}); bound {:.3e}".format(max(worst.values()), max(worst, key=worst.get), TOL))


def _compare(case, name, measured):
    got_i, got_m = _launch(case)
    errs = []
    for n in range(len(case["index"])):
        want_i, want_m = R.oracle(case, n)
        errs.append(float(np.abs(got_i[n] - want_i).max()))
        assert np.array_equal(got_m[n], want_m), (name, n)
    measured[name] = max(errs)
    print("{}: largest |kernel - float64| per item {}".format(name, ["{:.2e}".format(e) for e in errs]))
    assert max(errs) <= TOL, errs
    return got_i, got_m


# ---- images and masks against the restatement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [name for name, _ in R.image_cases()])
def test_images_and_masks_against_the_float64_oracle(name, measured):
    _compare(dict(R.image_cases())[name], name, measured)


def test_more_items_than_one_launch_carries(measured):
    """70 items: the entry point carries 64 windows, angles and factor sets per launch, so this is two launches; every item differs."""
    s, n_items = 8, 70
    images, masks = A.tiles(181, 5, s, 3)
    rng = np.random.default_rng(182)
    geom = []
    for _ in range(n_items):
        w = int(rng.integers(2, s + 1))
        geom.append((w, int(rng.integers(0, s - w + 1)), int(rng.integers(0, s - w + 1))))
    rot = [R.rot_of(float(a)) for a in rng.uniform(-180.0, 180.0, n_items)]
    color = [tuple(lo + rng.random() * (hi - lo) for lo, hi in A.RANGES.values()) for _ in range(n_items)]
    assert len(set(rot)) == n_items
    case = R.make_case(images, masks, [int(v) for v in rng.integers(0, 5, n_items)], [int(v) for v in rng.integers(0, 8, n_items)], geom,
                       rot, color, True)
    _compare(case, "70-items", measured)


# ---- against the jitter kernel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [5, 8, 33, 96])
@pytest.mark.parametrize("angle, turns", [(90, 1), (180, 2), (-90, -1)])
def test_quarter_turns_are_the_jitter_kernel_on_tiles_turned_on_the_host(s, angle, turns):
    from robosat_amd import ops

    images, masks = A.tiles(190 + s, 5, s, 3)
    turned_i = np.ascontiguousarray(np.rot90(images, turns, axes=(1, 2)))
    turned_m = np.ascontiguousarray(np.rot90(masks, turns, axes=(1, 2)))
    index, op, mean, std = _i32(R.INDEX), _i32(A.OPS), A.BAND_MEAN[:3], A.BAND_STD[:3]
    geom, color = [(s, 0, 0)] * 8, [A.IDENTITY_COLOR] * 8
    want_i, want_m = ops.augment_tiles_jitter(torch.from_numpy(turned_i).to(DEV), torch.from_numpy(turned_m).to(DEV), index, op, geom,
                                              color, None, mean, std, True)
    got_i, got_m = ops.augment_tiles_rotate(torch.from_numpy(images).to(DEV), torch.from_numpy(masks).to(DEV), index, op, geom,
                                            [R.rot_of(angle)] * 8, color, None, mean, std, True)
    assert torch.equal(got_m, want_m) and torch.equal(got_i, want_i)
    got_i, got_m = ops.augment_tiles_rotate(torch.from_numpy(images).to(DEV), None, index, op, geom, [R.rot_of(angle)] * 8, color, None,
                                            mean, std, False)
    assert got_m is None and torch.equal(got_i, want_i)


def test_zero_degrees_is_the_zoom_of_the_jitter_kernel(measured):
    """At S = 8 every window's A = 65536 w / 8 is exact: the masks are the jitter kernel's bit for bit.  The images are within the
    bound of the restatement (the zoom clamps its taps to the window, the rotation reads the window's true neighbours)."""
    from robosat_amd import ops

    s = 8
    images, masks = A.tiles(195, 5, s, 3)
    win = A.corner_windows(s, 4) + [(1, 3, 4), (3, 5, 0), (7, 1, 0), (5, 0, 3)]
    rng = np.random.default_rng(196)
    color = [tuple(lo + rng.random() * (hi - lo) for lo, hi in A.RANGES.values()) for _ in range(8)]
    case = R.make_case(images, masks, R.INDEX, A.OPS, win, [(65536, 0)] * 8, color, True)
    _, got_m = _compare(case, "zero-degrees", measured)
    dev_i, dev_m = torch.from_numpy(images).to(DEV), torch.from_numpy(masks).to(DEV)
    _, want_m = ops.augment_tiles_jitter(dev_i, dev_m, _i32(case["index"]), _i32(case["op"]), case["geom"], case["color"],
                                         ops.tile_band_sums(dev_i), case["mean"], case["std"], True)
    assert np.array_equal(got_m, want_m.cpu().numpy())


# ---- launch errors ---------------------------------------------------------------------------------------------------------------

def test_launch_errors():
    from robosat_amd import ops

    s = 8
    images, masks = A.tiles(197, 2, s, 3)
    images, masks = torch.from_numpy(images).to(DEV), torch.from_numpy(masks).to(DEV)
    sums = ops.tile_band_sums(images)
    index, op, mean, std = _i32([0, 1]), _i32([0, 3]), A.BAND_MEAN[:3], A.BAND_STD[:3]
    ident, whole, still = [A.IDENTITY_COLOR] * 2, [(s, 0, 0)] * 2, [(65536, 0)] * 2

    def run(geom=whole, rot=still, color=ident, im=images, su=sums, rgb=True, mean=mean, std=std):
        return ops.augment_tiles_rotate(im, masks, index, op, geom, rot, color, su, mean, std, rgb)

    run(rot=[(0, -65536), R.rot_of(45)])
    run(geom=[(s, 0, 0), (1, s - 1, s - 1)])  # the two extremes of a valid window
    for bad in ((65537, 0), (0, -65537), (65536, 65536), (0, 0), (46341, 46500), (2 ** 16, 2 ** 9 + 1)):  # no rotation
        with pytest.raises(ValueError, match="RS_EINVAL"):
            run(rot=[(65536, 0), bad])
    for bad in ((0, 0, 0), (s + 1, 0, 0), (4, 5, 0), (4, 0, 5), (4, -1, 0), (s, 1, 0)):  # a window that leaves the tile
        with pytest.raises(ValueError, match="RS_EINVAL"):
            run(geom=[bad, (s, 0, 0)])
    five = torch.zeros((2, s, s, 5), dtype=torch.uint8, device=DEV)  # C > 4
    with pytest.raises(ValueError, match="RS_EINVAL"):
        run(im=five, su=None, rgb=False, mean=[0.5] * 5, std=[0.5] * 5)
    two = torch.zeros((2, s, s, 2), dtype=torch.uint8, device=DEV)  # rgb with fewer than three bands
    with pytest.raises(ValueError, match="RS_EINVAL"):
        run(im=two, su=None, rgb=True, mean=[0.5] * 2, std=[0.5] * 2)
    run(im=two, su=None, rgb=False, mean=[0.5] * 2, std=[0.5] * 2)
    with pytest.raises(ValueError, match="RS_EINVAL"):  # a contrast factor needs the band sums
        run(color=[A.IDENTITY_COLOR, (1.0, 0.9, 1.0, 1.0)], su=None)
    for bad in ([(65536, 0)], [(65536, 0, 0)] * 2, [65536, 0]):  # `rot` of the wrong shape
        with pytest.raises(ValueError, match="rot"):
            run(rot=bad)
    with pytest.raises(RuntimeError, match="host values"):  # `rot` on the device
        run(rot=_i32(still))


# ---- loaders -----------------------------------------------------------------------------------------------------------------------

def test_the_two_device_loaders_rotate_alike_and_leave_validation_alone(tmp_path):
    """The shapes of the jitter module's loader test.  With ``rotate = 180`` in the full table and the same seeds the default loaders
    (workers decode and draw) and the cached ones (the loop draws) yield bit-equal training batches, twice over; they are not the
    batches of the table without the key; the validation batches are those of a config without the table."""
    from robosat_amd.tools.train import get_device_loaders, get_split_loaders

    ds_root = synth.make_dataset(str(tmp_path / "ds"), n_train=8, n_val=4, size=160, seed=4)
    plain = {"common": {"image_size": 128, "batch_size": 2}}
    unturned = dict(plain, augment=dict(TABLE))
    model = dict(plain, augment=dict(TABLE, rotate=180))
    dataset = {"common": {"dataset": ds_root}}
    dev = torch.device(DEV)

    def batches(loader, seed):
        random.seed(seed)
        return [(im.clone(), mk.clone(), tl) for im, mk, tl in loader]

    split_train, split_val = get_split_loaders(model, dataset, 0, dev)
    cache_train, cache_val = get_device_loaders(model, dataset, dev)
    unturned_train, _ = get_device_loaders(unturned, dataset, dev)
    _, plain_val = get_device_loaders(plain, dataset, dev)
    assert split_train.jitter.rotate == cache_train.jitter.rotate == 180.0 and unturned_train.jitter.rotate == 0.0
    want = batches(split_train, 123)
    assert len(want) == len(split_train) == 4
    for loader in (cache_train, split_train, cache_train):  # the other loader, and each a second time
        got = batches(loader, 123)
        assert len(got) == len(want)
        for (gi, gm, gt), (wi, wm, wt) in zip(got, want):
            assert gi.is_cuda and gi.dtype == torch.float32 and gm.dtype == torch.int64 and tuple(gi.shape) == (2, 3, 128, 128)
            assert torch.equal(gi, wi) and torch.equal(gm, wm) and bool(torch.isfinite(gi).all())
    other = batches(unturned_train, 123)
    assert len(other) == len(want) and all(not torch.equal(a[0], b[0]) for a, b in zip(other, want))
    val = batches(plain_val, 5)
    for loader in (split_val, cache_val):
        assert loader.jitter is None
        got = batches(loader, 5)
        assert len(got) == len(val) == 2
        for (gi, gm, _), (wi, wm, _) in zip(got, val):
            assert torch.equal(gi, wi) and torch.equal(gm, wm)
