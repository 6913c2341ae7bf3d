"""Numpy / float64 reference of the hard-pixel mining (TEST INFRASTRUCTURE ONLY): include/robosat_hip.h "HARD-PIXEL MINING", DESIGN.md
section 7e.

    keys64(logits, targets, ignore)            float64 [N, H, W]: the cross-entropy lse - x_t of every pixel (0 at an ignored one)
    keys_u32(keys64)                           the float64 keys rounded once to float32, as the uint32 the definition names
    k_of(v, fraction)                          min(V, max(1, ceil(fraction * V))), 0 for V = 0: the same double expression
    select(keys_u32, valid, fraction, cap)     (plane float32 [N, H, W], info int64 [N, 4]) by a full np.sort per image
    select_brute(...)                          the same by counting, for tiny inputs
    loss64(name, logits, targets, weight, plane, ignore)   the `_pw` loss in float64 (boundary_ref.loss64)

Nothing here knows how the device selects: a sort, a count and a comparison."""

import math
import os
import struct
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import boundary_ref as B  # noqa: E402

NO_CAP = 0xFFFFFFFF
IGNORE = 255


def keys64(logits, targets, ignore=None):
    """float64 numpy [N, H, W]: lse - x_t in float64; 0 at an ignored pixel (which ``valid`` leaves out anyway)."""

    x = logits.double()
    t = targets if ignore is None else torch.where(targets == ignore, torch.zeros_like(targets), targets)
    l = torch.logsumexp(x, dim=1) - x.gather(1, t.unsqueeze(1)).squeeze(1)
    if ignore is not None:
        l = torch.where(targets == ignore, torch.zeros_like(l), l)
    return l.numpy()


def keys_u32(k64):
    """bits(float32(l)) if l > 0 else 0."""

    f = np.asarray(k64, dtype=np.float64).astype(np.float32)
    bits = f.view(np.uint32).copy()
    bits[~(f > 0)] = 0
    return bits


def key_floats(keys):
    """uint32 keys as the float64 values of the float32 they are the bits of."""

    return np.ascontiguousarray(keys, dtype=np.uint32).view(np.float32).astype(np.float64)


def valid_of(targets, ignore=None):
    t = targets.numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    return np.ones(t.shape, dtype=bool) if ignore is None else t != ignore


def k_of(v, fraction):
    if v == 0:
        return 0
    return min(int(v), max(1, int(math.ceil(float(fraction) * float(v)))))


def cap_of(below):
    """bits(float32(-ln below)), float64 rounded once; ``None`` -> no cap."""

    if below is None:
        return NO_CAP
    return struct.unpack("<I", struct.pack("<f", -math.log(float(below))))[0]


def select(keys, valid, fraction, cap=NO_CAP, base=None):
    """keys uint32 [N, H, W], valid bool [N, H, W] -> (plane float32 [N, H, W], info int64 [N, 4] = (V, k, tau, kept)); tau = 0 for
    V = 0.  A full sort per image."""

    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    n = keys.shape[0]
    plane = np.zeros(keys.shape, dtype=np.float32)
    info = np.zeros((n, 4), dtype=np.int64)
    for i in range(n):
        mine = keys[i][valid[i]]
        v = int(mine.size)
        k = k_of(v, fraction)
        tau = 0
        if v:
            tau = min(int(np.sort(mine)[v - k]), int(cap))
            keep = valid[i] & (keys[i] >= np.uint32(tau))
            plane[i][keep] = 1.0 if base is None else np.asarray(base, dtype=np.float32)[i][keep]
            info[i, 3] = int(keep.sum())
        info[i, :3] = (v, k, tau)
    return plane, info


def select_brute(keys, valid, fraction, cap=NO_CAP):
    """The definition by counting: tau is the largest key value u among the valid ones with #{valid keys >= u} >= k."""

    keys = np.asarray(keys, dtype=np.uint32)
    n = keys.shape[0]
    plane = np.zeros(keys.shape, dtype=np.float32)
    info = np.zeros((n, 4), dtype=np.int64)
    for i in range(n):
        flat, ok = keys[i].reshape(-1).tolist(), valid[i].reshape(-1).tolist()
        mine = [u for u, o in zip(flat, ok) if o]
        v = len(mine)
        k = k_of(v, fraction)
        tau = 0
        if v:
            tau = max(u for u in mine if sum(1 for q in mine if q >= u) >= k)
            tau = min(tau, cap)
        kept = 0
        out = plane[i].reshape(-1)
        for j, (u, o) in enumerate(zip(flat, ok)):
            if o and v and u >= tau:
                out[j] = 1.0
                kept += 1
        info[i] = (v, k, tau, kept)
    return plane, info


def loss64(name, logits, targets, weight, plane, ignore=None, gamma=2):
    """(loss, gradient float64, denominator) of sum_kept base w l / sum_kept base w in float64."""

    return B.loss64(name, logits, targets, weight, torch.as_tensor(plane), ignore, gamma=gamma)


def selection_is_safe(k64, valid, fraction, below=None, rel=1e-4):
    """On the float64 keys alone: per image the k-th and the (k+1)-th largest differ by more than ``rel`` * tau, and no key lies within
    ``rel`` (relative) of the cap -- so float32 rounding of the keys cannot change the selected set.  Returns the smallest gap found, in
    units of tau; raises AssertionError where the precondition fails (a test error, never a skip)."""

    worst = float("inf")
    for i in range(k64.shape[0]):
        mine = np.sort(k64[i][valid[i]])[::-1]
        v = mine.size
        k = k_of(v, fraction)
        if v == 0:
            continue
        tau = float(mine[k - 1])
        if k < v:
            gap = (tau - float(mine[k])) / tau
            assert gap > rel, "image {}: the {}-th and the next key are {:.3e} tau apart".format(i, k, gap)
            worst = min(worst, gap)
        if below is not None:
            c = -math.log(float(below))
            near = float(np.min(np.abs(mine - c))) / c
            assert near > rel, "image {}: a key lies {:.3e} (relative) from the cap".format(i, near)
            worst = min(worst, near)
    return worst
