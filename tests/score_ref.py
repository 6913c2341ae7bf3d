"""What the ``rs features --score`` tests share: the per-component sums of probability bytes (include/robosat_hip.h,
rs_features_scores) restated with ``np.add.at``, and the probability they stand for as ``rs masks`` computes it.  Not a test module."""

import numpy as np


def sums(labels, q):
    """``labels`` int [R, ...] (one independent raster per entry of the first axis, 0 = background) and ``q`` uint8 [K, R, ...] ->
    {(raster, label): int64 [K]}: every model's bytes summed over the component's pixels."""

    labels, q = np.asarray(labels), np.asarray(q)
    assert q.shape[1:] == labels.shape and q.dtype == np.uint8
    out = {}
    for raster in range(labels.shape[0]):
        flat = labels[raster].reshape(-1)
        fg = flat != 0
        names, inverse = np.unique(flat[fg], return_inverse=True)
        total = np.zeros((len(names), q.shape[0]), dtype=np.int64)
        for k in range(q.shape[0]):
            np.add.at(total[:, k], inverse.reshape(-1), q[k, raster].reshape(-1)[fg].astype(np.int64))
        for name, row in zip(names.tolist(), total):
            out[(raster, int(name))] = row
    return out


def rows(table, by_key, k, stitched=False):
    """The restated sums in the order of a component table's rows: int64 [N, K]."""

    table = np.asarray(table)
    keys = [(0, int(r[0])) for r in table] if stitched else [(int(r[0]), int(r[1])) for r in table]
    return np.array([by_key[key] for key in keys], dtype=np.int64).reshape(len(keys), k)


def vote(q, weights=None):
    """uint8 [K, ...] -> float64 [...]: the probability ``rs masks`` votes with (tools/masks.py, the reference's soft voting)."""

    return np.average(np.linspace(0, 1, 256)[np.asarray(q)], axis=0, weights=weights)


def mean_vote(q, mask, weights=None):
    """The mean of ``vote`` over the pixels of ``mask``: what a polygon's ``score`` stands for."""

    return float(vote(q, weights)[np.asarray(mask, dtype=bool)].mean())
