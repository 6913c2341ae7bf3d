"""Dihedral test-time augmentation, host side (no GPU): the mode tables of ``ops.tta_ops``, the coordinate maps the kernels use
(include/robosat_hip.h, rs_tta_*), the ``--tta`` flag of ``rs predict`` / ``rs serve`` and the order invariance of the sorted fp32
merge the definition rests on."""

import argparse
import itertools

import numpy as np
import pytest

from robosat_amd import ops


def view(a, op):
    """View of a [H,W,...] array under op = f + 2*k: FLIP_LEFT_RIGHT when f, then k counter-clockwise rot90s."""

    if op & 1:
        a = np.fliplr(a)
    return np.rot90(a, (op >> 1) & 3)


def fwd(op, h, w, y, x):
    """Restatement of tta.hip:tta_fwd: tile pixel (y, x) -> its position in the view."""

    if op & 1:
        x = w - 1 - x
    for _ in range((op >> 1) & 3):
        y, x = w - 1 - x, y
        h, w = w, h
    return y, x


def inv(op, h, w, y, x):
    """Restatement of tta.hip:tta_inv: view pixel (y, x) -> the tile pixel it shows."""

    k = (op >> 1) & 3
    hc = w if k & 1 else h
    for _ in range(k):
        y, x = x, hc - 1 - y
        hc = w if hc == h else h
    if op & 1:
        x = w - 1 - x
    return y, x


def test_mode_tables():
    assert ops.tta_ops("none", 64, 64) == [0]
    assert ops.tta_ops("hflip", 192, 256) == [0, 1]
    assert ops.tta_ops("flips", 192, 256) == [0, 1, 4, 5]
    assert ops.tta_ops("d4", 256, 256) == list(range(8))
    with pytest.raises(ValueError, match="square"):
        ops.tta_ops("d4", 192, 256)
    with pytest.raises(ValueError, match="unknown TTA mode"):
        ops.tta_ops("d8", 256, 256)


@pytest.mark.parametrize("mode", ["none", "hflip", "flips", "d4"])
def test_modes_are_groups(mode):
    """Closure under composition is what makes the sorted merge exactly equivariant."""

    h = w = 8
    a = np.arange(h * w).reshape(h, w)
    ops_ = ops.tta_ops(mode, h, w)
    views = [view(a, op).tobytes() for op in ops_]
    assert len(set(views)) == len(ops_)
    for g, k in itertools.product(ops_, ops_):
        assert view(view(a, g), k).tobytes() in views


@pytest.mark.parametrize("hw", [(8, 8), (4, 6)])
def test_coordinate_maps_match_numpy(hw):
    h, w = hw
    a = np.arange(h * w).reshape(h, w)
    for op in range(8):
        if (op >> 1) & 1 and h != w:
            continue
        v = view(a, op)
        for y in range(h):
            for x in range(w):
                qy, qx = fwd(op, h, w, y, x)
                assert v[qy, qx] == a[y, x], (op, y, x)  # view_v[g_v(p)] = tile[p]
                assert inv(op, h, w, qy, qx) == (y, x)
        for qy in range(v.shape[0]):
            for qx in range(v.shape[1]):
                assert a[inv(op, h, w, qy, qx)] == v[qy, qx]  # view_v[q] = tile[g_v^-1(q)]


def test_coordinate_maps_keep_32_blocks_whole():
    """The kernels move aligned 32 x 32 blocks: every op maps one onto one."""

    s = 96
    for op in range(8):
        for by, bx in itertools.product(range(3), range(3)):
            blocks = {tuple(c // 32 for c in fwd(op, s, s, by * 32 + y, bx * 32 + x)) for y in range(32) for x in range(32)}
            assert len(blocks) == 1


def test_predict_argv_round_trips_tta():
    from robosat_amd.tools import predict

    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    predict.add_parser(sub)
    p = sub._name_parser_map["predict"]
    ns = argparse.Namespace(batch_size=4, checkpoint="c.pth", overlap=16, tile_size=256, workers=2, tiles="t", probs="p", model="m",
                            dataset="d", extra_tiles=[], tta="d4")
    argv = predict.argv_from_args(ns)
    assert argv[argv.index("--tta") + 1] == "d4"
    back = p.parse_args(argv[1:])
    assert (back.tta, back.tiles, back.probs) == ("d4", "t", "p")
    ns.tta = "none"
    argv = predict.argv_from_args(ns)
    assert "--tta" not in argv and p.parse_args(argv[1:]).tta == "none"
    del ns.tta  # (a namespace built without the flag)
    assert "--tta" not in predict.argv_from_args(ns)


def test_serve_takes_tta():
    from robosat_amd.tools import serve

    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    serve.add_parser(sub)
    back = sub._name_parser_map["serve"].parse_args(["--model", "m", "--dataset", "d", "--checkpoint", "c", "--tta", "flips"])
    assert back.tta == "flips"


def sorted_merge(vals):
    """The merge of rs_tta_merge over the view axis 0: sort ascending, fp32 sum from the smallest, times 1/V."""

    vals = np.sort(np.asarray(vals, dtype=np.float32), axis=0)
    acc = vals[0].copy()
    for v in vals[1:]:
        acc = (acc + v).astype(np.float32)
    return (acc * np.float32(1.0 / len(vals))).astype(np.float32)


def test_sorted_merge_is_order_invariant():
    """Adversarial values: a plain sum in view order loses 1e-8 beside 0.5 in some orders and not in others."""

    rng = np.random.default_rng(3)
    base = np.array([1e-8, 0.5, 3e-8, 0.25, 1e-8, 0.125, 0.0625 + 1e-8, 2e-8], dtype=np.float32)
    cols = np.stack([base, rng.permutation(base), rng.random(8, dtype=np.float32),
                     np.array([0.5, 1e-8, 1e-8, 1e-8, 1e-8, 1e-8, 1e-8, 1e-8], dtype=np.float32)], axis=1)
    want = sorted_merge(cols)
    plain = set()
    for perm in itertools.permutations(range(8)):
        assert np.array_equal(sorted_merge(cols[list(perm)]), want)
        acc = np.float32(0)
        for i in perm:
            acc = np.float32(acc + cols[i, 3])
        plain.add(float(acc))
    assert len(plain) > 1  # (the unsorted sum does depend on the order: the test has teeth)
