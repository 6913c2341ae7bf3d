"""The centerline raster stages on the MI355X through the ops wrappers: ``ops.thin_masks`` (Guo-Hall thinning) byte for byte and
``ops.skeleton_links`` as a set of rows against the numpy restatements of tests/thin_ref.py, tile by tile."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

# either side of the 32- and 64-pixel word edges; 512 x 512 for the full tile's 257 pairs and the chunked stop
SIZES = [(1, 1), (2, 2), (7, 5), (31, 33), (64, 64), (65, 63), (100, 130), (512, 512)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _batch(h, w):
    """One batch of every pattern: tiles that converge at once (empty, the spiral, noise) beside tiles that take long (full)."""

    spiral = np.zeros((h, w), dtype=bool)
    n = min(h, w)
    spiral[:n, :n] = R.spiral(n)
    tiles = [R.blobs(h, w, 3 * h + w), R.noise(h, w, h, 0.5), R.noise(h, w, w, 0.9), np.ones((h, w), bool), np.zeros((h, w), bool),
             R.border(h, w) if h > 2 and w > 2 else np.ones((h, w), bool), spiral]
    return np.stack(tiles).astype(np.uint8)


_CACHE = {}


def _reference(h, w):
    """(batch, its restated skeletons, the most pairs any tile took), computed once per size and left unchanged."""

    if (h, w) not in _CACHE:
        batch = _batch(h, w)
        done = [T.thin(m, want_pairs=True) for m in batch]
        _CACHE[(h, w)] = batch, np.stack([s for s, _ in done]), max(p for _, p in done)
    return _CACHE[(h, w)]


@pytest.mark.parametrize("h,w", SIZES)
def test_thin_masks_equals_the_restatement_byte_for_byte(h, w):
    batch, want, pairs = _reference(h, w)
    got = ops.thin_masks(_dev(batch))
    assert got.dtype == torch.uint8 and got.shape == batch.shape
    got = got.cpu().numpy()
    wrong = [(i, int((got[i] != want[i]).sum())) for i in range(len(batch)) if (got[i] != want[i]).any()]
    assert not wrong, ("tiles (index, differing pixels)", wrong)
    if (h, w) == (512, 512):
        assert pairs == 257  # the full tile: S/2 + 1 pairs, many chunks of the default size
    # non-zero is foreground, whatever the byte; a single tile gives what it gives in the batch
    assert (ops.thin_masks(_dev(batch[:1] * 7)).cpu().numpy() == want[:1]).all()


@pytest.mark.parametrize("h,w", [(65, 63), (100, 130)])
def test_the_skeleton_does_not_depend_on_the_chunk_size(h, w):
    batch, want, pairs = _reference(h, w)
    assert pairs > 8, "every chunk size below converges in its first chunk: the test shows nothing"
    for chunk in (1, 3, 8, 1000):
        assert (ops.thin_masks(_dev(batch), pairs=chunk).cpu().numpy() == want).all(), chunk
    assert (ops.thin_masks(_dev(want)).cpu().numpy() == want).all(), "a skeleton is a fixed point"


@pytest.mark.parametrize("min_area", [0, 12])
@pytest.mark.parametrize("h,w", [(7, 5), (65, 63), (100, 130)])
def test_link_rows_equal_the_restatement_as_sets(h, w, min_area):
    batch, skeletons, _ = _reference(h, w)
    masks = _dev(batch)
    labels = ops.label_components(masks)
    table = ops.component_table(labels, min_area)
    got = ops.skeleton_links(ops.thin_masks(masks), labels, table)
    assert got.dtype == torch.int32 and got.shape[1] == 5
    want, dropped = [], 0
    for i, m in enumerate(batch):
        ref_labels = R.label(m)
        kept = R.table(ref_labels, min_area)[:, 1]
        dropped += len(np.unique(ref_labels)) - 1 - len(kept)
        want.append(T.links(skeletons[i], ref_labels, kept=kept, tile=i))
    want = R.sort_rows(np.concatenate(want))
    got = R.sort_rows(got.cpu().numpy().astype(np.int64))
    assert got.shape == want.shape and (got == want).all()
    assert len({tuple(r) for r in got.tolist()}) == len(got), "a link twice"
    if min_area and (h, w) != (7, 5):
        assert dropped > 0, "min_area dropped nothing: the test shows nothing"
    if not min_area and (h, w) != (7, 5):
        assert (want[:, 4] == -1).any() and {0, 1, 2, 3} <= set(want[:, 4].tolist())
    assert len(ops.skeleton_links(ops.thin_masks(masks), labels, table[:0])) == 0


def test_bad_arguments_raise_as_the_neighbouring_stages_do():
    masks = _dev(_batch(8, 8))
    labels = ops.label_components(masks)
    table = ops.component_table(labels)
    with pytest.raises(RuntimeError):
        ops.thin_masks(masks.cpu())
    with pytest.raises(ValueError):
        ops.thin_masks(masks, pairs=0)
    with pytest.raises(ValueError):
        ops.thin_masks(torch.zeros((1, 1, 4097), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(TypeError):
        ops.thin_masks(masks.to(torch.int32))
    with pytest.raises(RuntimeError):
        ops.skeleton_links(masks.cpu(), labels, table)
    with pytest.raises(RuntimeError):
        ops.skeleton_links(masks, labels.cpu(), table)
    with pytest.raises(ValueError):
        ops.skeleton_links(masks, labels, table, nbr=torch.full((len(masks), 8), -1, dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError):
        big = torch.zeros((1, 1, 4097), dtype=torch.uint8, device="cuda:0")
        ops.skeleton_links(big, big.to(torch.int32), table[:0])
