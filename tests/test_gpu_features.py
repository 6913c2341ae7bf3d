"""``rs features`` raster stages on the MI355X against the numpy restatements of tests/features_ref.py, byte for byte: class select +
open + close (both kernel forms), canonical labels, component table, boundary-edge sets."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402

from robosat_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = [0, 1, 2, 3, 4, 5, 20, 21]
# (819 x 800 is the largest plane pair that fits the 160 KB LDS with 25 words per row; 820 x 800 is the first that does not)
SIZES = [(1, 1), (7, 5), (64, 64), (100, 130), (512, 512), (576, 576), (819, 800), (820, 800), (1024, 1024)]
INDEX = 2


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _images(h, w, seed, few=False):
    """Class-index images (classes 0..3, the selected one is INDEX): random at several densities, blobs, full, empty, border."""

    rng = np.random.RandomState(seed)
    masks = [R.noise(h, w, seed, 0.5), R.blobs(h, w, seed), np.ones((h, w), bool), R.border(h, w)]
    if not few:
        masks += [R.noise(h, w, seed + 1, 0.1), R.noise(h, w, seed + 2, 0.9), np.zeros((h, w), bool), R.blobs(h, w, seed + 1, 12)]
    out = []
    for m in masks:
        other = rng.choice(np.array([0, 1, 3], dtype=np.uint8), size=(h, w))
        out.append(np.where(m, np.uint8(INDEX), other))
    return np.stack(out)


def test_lds_limit_is_where_the_sizes_say():
    assert ops.clean_form(819, 800) == ops.CLEAN_LDS and ops.clean_form(820, 800) == ops.CLEAN_HBM
    assert ops.clean_form(512, 512) == ops.CLEAN_LDS and ops.clean_form(576, 576) == ops.CLEAN_LDS and ops.clean_form(1024, 1024) == ops.CLEAN_HBM


@pytest.mark.parametrize("eps", EPS)
def test_clean_masks_equal_the_restatement(eps):
    for h, w in SIZES:
        images = _images(h, w, eps, few=h * w > 820 * 800)
        want = np.stack([R.clean(im, INDEX, eps, eps) for im in images])
        dev = _dev(images)
        got = ops.clean_masks(dev, INDEX, eps, eps).cpu().numpy()
        assert got.dtype == np.uint8 and (got == want).all(), (eps, h, w, int((got != want).sum()))
        forms = [ops.CLEAN_HBM] + ([ops.CLEAN_LDS] if ops.clean_form(h, w) == ops.CLEAN_LDS else [])
        assert len(forms) == 2 or h * w >= 820 * 800
        for form in forms:
            other = ops.clean_masks(dev, INDEX, eps, eps, form=form).cpu().numpy()
            assert (other == want).all(), ("form", form, eps, h, w)


@pytest.mark.parametrize("eps_open,eps_close", [(20, 0), (0, 20), (3, 20), (20, 5), (4, 21), (64, 2)])
def test_clean_masks_with_different_discs(eps_open, eps_close):
    for h, w in ((100, 130), (512, 512), (820, 800)):
        images = _images(h, w, 7, few=True)
        want = np.stack([R.clean(im, INDEX, eps_open, eps_close) for im in images])
        for form in [ops.CLEAN_AUTO, ops.CLEAN_HBM] + ([ops.CLEAN_LDS] if ops.clean_form(h, w) == ops.CLEAN_LDS else []):
            assert (ops.clean_masks(_dev(images), INDEX, eps_open, eps_close, form=form).cpu().numpy() == want).all(), (h, w, form)


def test_clean_masks_rejects_bad_arguments():
    images = _dev(_images(8, 8, 0, few=True))
    with pytest.raises(ValueError):
        ops.clean_masks(images, INDEX, 65, 0)
    with pytest.raises(ValueError):
        ops.clean_masks(_dev(_images(820, 800, 0, few=True)), INDEX, 3, 3, form=ops.CLEAN_LDS)
    with pytest.raises(RuntimeError):
        ops.clean_masks(images.cpu(), INDEX, 3, 3)


def _check_components(masks, min_area=0):
    masks = np.stack(masks).astype(np.uint8)
    b, h, w = masks.shape
    want = np.stack([R.label(m) for m in masks])
    labels = ops.label_components(_dev(masks))
    got = labels.cpu().numpy()
    assert got.dtype == np.int32 and (got == want).all(), int((got != want).sum())
    table = ops.component_table(labels, min_area)
    want_table = np.concatenate([R.table(want[i], min_area, tile=i) for i in range(b)])
    assert (table.cpu().numpy() == want_table).all() and table.shape == want_table.shape
    edges = R.sort_rows(ops.boundary_edges(labels, table).cpu().numpy())
    want_edges = np.concatenate([R.edges(R.filter_labels(want[i], min_area), tile=i) for i in range(b)])
    assert edges.shape == want_edges.shape and (edges == want_edges).all()
    return got, table.cpu().numpy(), edges


@pytest.mark.parametrize("h,w", SIZES)
def test_labels_table_and_edges_equal_the_restatement(h, w):
    images = _images(h, w, 3, few=h * w > 820 * 800)
    masks = [im == INDEX for im in images] + [R.closing(R.opening(images[1] == INDEX, 5), 5)]
    _check_components(masks)


def test_checkerboard_has_a_component_per_pixel():
    got, table, edges = _check_components([R.checkerboard(512, 512), R.checkerboard(512, 512)])
    assert len(table) == 2 * 512 * 512 // 2 and len(edges) == 4 * len(table)


def test_spiral_filling_a_tile():
    got, table, _ = _check_components([R.spiral(512)])
    assert len(table) == 1 and table[0, 1] == 1 and table[0, 2] == R.spiral(512).sum()


def test_comb_filling_a_tile():
    got, table, _ = _check_components([R.comb(512), R.comb(512)[::-1].copy(), R.comb(512).T.copy()])
    assert len(table) == 3


def test_corner_contacts_and_nesting():
    _check_components([R.corner_touch()])
    _, table, _ = _check_components([R.nested()])
    assert len(table) == 3
    _check_components([R.self_touching()])


@pytest.mark.parametrize("min_area", [1, 2, 50, 10 ** 6])
def test_min_area_filter(min_area):
    masks = [R.noise(100, 130, 1, 0.5), R.blobs(100, 130, 2), R.noise(100, 130, 3, 0.3)]
    _, table, edges = _check_components(masks, min_area)
    assert (table[:, 2] >= min_area).all()
    if min_area == 10 ** 6:
        assert len(table) == 0 and len(edges) == 0


def test_a_tile_alone_equals_the_tile_in_a_batch_and_runs_repeat():
    images = np.concatenate([_images(512, 512, 11), _images(512, 512, 12)])[:16]
    assert len(images) == 16
    dev = _dev(images)
    outs = []
    for _ in range(2):
        clean = ops.clean_masks(dev, INDEX, 20, 20)
        labels = ops.label_components(clean)
        table = ops.component_table(labels, 4)
        edges = R.sort_rows(ops.boundary_edges(labels, table).cpu().numpy())
        outs.append((clean.cpu().numpy(), labels.cpu().numpy(), table.cpu().numpy(), edges))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    clean, labels, table, edges = outs[0]
    for i in (0, 5, 15):
        c1 = ops.clean_masks(dev[i:i + 1].contiguous(), INDEX, 20, 20)
        l1 = ops.label_components(c1)
        t1 = ops.component_table(l1, 4)
        e1 = R.sort_rows(ops.boundary_edges(l1, t1).cpu().numpy())
        assert (c1.cpu().numpy()[0] == clean[i]).all() and (l1.cpu().numpy()[0] == labels[i]).all()
        assert (t1.cpu().numpy()[:, 1:] == table[table[:, 0] == i][:, 1:]).all()
        assert (e1[:, 1:] == edges[edges[:, 0] == i][:, 1:]).all()
