"""``ops.lovasz_fwd`` (``rs_lovasz_fwd`` / ``rs_lovasz_fwd_ig``, csrc/lovasz.hip) on the MI355X held EXACTLY to the stable-sort
restatement of ``lovasz_hinge_ref``: every gradient entry by value (1 fp32 ulp where N is no power of two), zeros where the
error is not above 0, +0.0 at ignored pixels, the loss to one fp32 ulp.  The kernel's header claims a stable sort and the
reference's fp32 operations; a tied pair in the wrong order, a rank off by one inside a tile or a block offset off by one all
change some entry, and none passes here.

The inputs are the families of ``lovasz_hinge_ref.family`` (one key; two or four; ~60; keys that differ in one byte; a ramp; the
Gaussian of the older tests), the shapes the smallest that reach each shape-dependent branch of the file -- ``SHAPES`` says which,
and ``test_the_shapes_reach_the_branches_they_are_here_for`` holds the table to the library's own tile sizes."""

import functools

import numpy as np
import pytest
import torch

import lovasz_hinge_ref as H
from robosat_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IG = 255

SCAN_CHUNK, SORT_TILE, SMALL_SORT_TILE, SMALL_TILE_FROM = 1024, 8192, 4096, 8 << 20  # csrc/lovasz.hip
EVERY, SOME, BIG = tuple(H.FAMILIES), ("quant", "gauss"), ("quant",)

# (N, C, H, W), families, (sort tiles, scan blocks) per image, what the shape reaches
SHAPES = [
    ((2, 3, 7, 9), EVERY, (1, 1), "P = 189: one partial block; the scalar keys, histogram and load paths"),
    ((3, 2, 16, 32), SOME, (1, 1), "P = 1024: exactly one scan chunk"),
    ((3, 2, 2, 257), EVERY, (1, 2), "P = 1028, HW % 4 != 0 but P % 4 == 0: the scalar keys kernel feeds the 16-byte histogram, "
                                   "block-sum and load paths; the second scan chunk holds 4 entries"),
    ((1, 2, 64, 64), EVERY, (1, 8), "P = 8192: exactly one sort tile"),
    ((1, 2, 63, 65), SOME, (1, 8), "P = 8190: a tile short by 2; everything scalar"),
    ((2, 2, 17, 241), EVERY, (2, 9), "P = 8194: the second tile holds 2 keys; scalar"),
    ((1, 3, 4, 683), SOME, (2, 9), "P = 8196: the second tile holds 4 keys; 16-byte paths"),
    ((1, 5, 90, 91), SOME, (5, 40), "P = 40 950: 5 sort tiles, the last quarter of radix_scan_kernel's blocks is empty"),
    ((8, 2, 16, 16), SOME, (1, 1), "P = 512, N = 8: the apply kernel's XCD-affine order with one scan block"),
    ((8, 3, 20, 20), EVERY, (1, 2), "P = 1200: XCD-affine apply with two scan blocks, three classes"),
    ((16, 2, 65, 64), EVERY, (2, 9), "P = 8320, N = 16: the scatter's and the apply kernel's XCD-affine orders, 2 sort tiles, 9 scan blocks"),
    ((24, 3, 20, 21), SOME, (1, 2), "P = 1260, N = 24: three groups of 8 images in both remaps; N no power of two (the 1-ulp bar)"),
    ((16, 2, 512, 512), BIG, (128, 512), "8 Mi keys: the 4096-key tile, both remaps, lovasz_scan_blocks_kernel with 2 blocks per thread"),
    ((16, 2, 512, 514), BIG, (129, 514), "the 4096-key tile with a half-filled last tile; the apply kernel in natural order (P * 4 > 2 MiB)"),
]
CASES = [(name, shape) for shape, names, _, _ in SHAPES for name in names]
IGNORE_SHAPES = [(2, 3, 7, 9), (3, 2, 2, 257), (2, 2, 17, 241), (16, 2, 65, 64)]
IGNORE_CASES = [(name, shape, pattern) for shape in IGNORE_SHAPES for name in ("quant", "const", "gauss")
                for pattern in ("none", "rows", "scattered", "image")]


def _sid(shape):
    return "x".join(map(str, shape))


def _blocks(shape):
    """(sort tile, sort tiles per image, scan blocks per image, scatter affine, apply affine) by the rules of csrc/lovasz.hip."""

    n, c, h, w = shape
    p = c * h * w
    tile = SMALL_SORT_TILE if n * p >= SMALL_TILE_FROM else SORT_TILE
    return tile, -(-p // tile), -(-p // SCAN_CHUNK), n % 8 == 0 and n >= 16, n % 8 == 0 and p * 4 <= 2 << 20


def test_the_shapes_reach_the_branches_they_are_here_for():
    """The table's block counts follow from P and the tile sizes written above, and the library's workspace has exactly the size
    those tile sizes give: a change of tile size or scan chunk fails here instead of silently moving an edge out of reach."""

    lib = _lib.lib()
    up = lambda b: (b + 255) & ~255  # noqa: E731
    for shape, _, (nblk_sort, nblk_scan), why in SHAPES:
        n, c, h, w = shape
        tile, got_sort, got_scan, _, _ = _blocks(shape)
        assert (got_sort, got_scan) == (nblk_sort, nblk_scan), (shape, why)
        want = 4 * up(n * c * h * w * 4) + up(n * nblk_sort * 256 * 4) + up(n * nblk_scan * 4) + up(n * nblk_scan * 8)
        assert lib.rs_lovasz_workspace_bytes(n, c, h, w) == want, (shape, why)
    by = {shape: _blocks(shape) for shape, _, _, _ in SHAPES}
    p = lambda s: s[1] * s[2] * s[3]  # noqa: E731
    assert p((3, 2, 16, 32)) == SCAN_CHUNK and p((3, 2, 2, 257)) == SCAN_CHUNK + 4 and (2 * 257) % 4 != 0
    assert p((1, 2, 64, 64)) == SORT_TILE and p((1, 2, 63, 65)) == SORT_TILE - 2 and p((2, 2, 17, 241)) == SORT_TILE + 2
    assert p((1, 3, 4, 683)) == SORT_TILE + 4 and (4 * 683) % 4 == 0
    assert 3 * ((by[(1, 5, 90, 91)][1] + 3) // 4) >= by[(1, 5, 90, 91)][1]  # the fourth quarter starts past the last tile
    assert by[(8, 2, 16, 16)][3:] == (False, True) and by[(8, 3, 20, 20)][3:] == (False, True)
    assert by[(16, 2, 65, 64)][3:] == (True, True) and by[(24, 3, 20, 21)][3:] == (True, True)
    assert by[(16, 2, 512, 512)][0] == SMALL_SORT_TILE and by[(16, 2, 512, 512)][3:] == (True, True)
    assert (by[(16, 2, 512, 512)][2] + 255) // 256 == 2 and 16 * p((16, 2, 512, 512)) == SMALL_TILE_FROM
    assert by[(16, 2, 512, 514)][0] == SMALL_SORT_TILE and by[(16, 2, 512, 514)][3:] == (True, False)
    assert p((16, 2, 512, 514)) % SMALL_SORT_TILE == SMALL_SORT_TILE // 2
    assert all(by[s][0] == SORT_TILE for s in by if s[2] < 512)


def _make(name, shape):
    x, y = H.family(name, shape, seed=sum(shape))
    return (x, y) + H.hinge_exact(x, y, detail=True)


_cached = functools.lru_cache(maxsize=None)(_make)


def _case(name, shape):
    """(logits, labels, loss, unit_delta, detail): computed once per (family, shape) and shared; the two 8 Mi-key cases, used once
    each, are not kept."""

    return (_make if shape[2] >= 512 else _cached)(name, shape)


def _run(x, y, ignore=None, want_grad=True):
    loss, grad = ops.lovasz_fwd(x.to(DEV), y.to(DEV), want_grad=want_grad, ignore=ignore)
    torch.cuda.synchronize()
    return loss.cpu(), (grad.cpu() if grad is not None else None)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name,shape", CASES, ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_lovasz_hinge_is_the_stable_sort_reference_exactly(name, shape):
    x, y, want_loss, unit, detail = _case(name, shape)
    loss, grad = _run(x, y)
    print("{} {}: loss {!r} want {!r}".format(name, shape, float(loss), want_loss))
    H.assert_hinge_exact(loss, grad, want_loss, unit, shape[0], detail, what="{} {}".format(name, _sid(shape)))


@pytest.mark.parametrize("shape", [(16, 2, 65, 64), (8, 3, 20, 20)], ids=_sid)
def test_the_xcd_orders_change_no_bit(shape):
    for name in ("quant", "gauss"):
        x, y = _case(name, shape)[:2]
        loss, grad = _run(x, y)
        with ops.knob("lovasz_xcd", 0):
            loss0, grad0 = _run(x, y)
        assert _same_bits(loss, loss0) and _same_bits(grad, grad0), name


@pytest.mark.parametrize("name,shape,pattern", IGNORE_CASES, ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_lovasz_hinge_with_an_ignore_label_is_the_reference_on_the_compaction(name, shape, pattern):
    x, y = _case(name, shape)[:2]
    mask = H.ignored_mask(pattern, shape, seed=sum(shape))
    labels = torch.where(mask, torch.full_like(y, IG), y)
    loss, grad = _run(x, labels, ignore=IG)
    if pattern == "none":  # nothing ignored: the reference already made, and the plain entry point's very bits
        _, _, want_loss, unit, detail = _case(name, shape)
        plain_loss, plain_grad = _run(x, y)
        assert _same_bits(loss, plain_loss) and _same_bits(grad, plain_grad)
    else:
        want_loss, unit, detail = H.hinge_exact(x, labels, ignore=IG, detail=True)
        assert np.array_equal(detail.ignored, mask.numpy())
    H.assert_hinge_exact(loss, grad, want_loss, unit, shape[0], detail, what="{} {} {}".format(name, _sid(shape), pattern))
    if pattern == "image":
        assert int(torch.count_nonzero(grad[-1])) == 0 and not bool(torch.signbit(grad[-1]).any())


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (16, 2, 65, 64)], ids=_sid)
def test_the_loss_alone_has_the_same_bits(shape):
    x, y = _case("quant", shape)[:2]
    mask = H.ignored_mask("scattered", shape, seed=sum(shape))
    labels = torch.where(mask, torch.full_like(y, IG), y)
    for t, ignore in ((y, None), (labels, IG)):
        with_grad, _ = _run(x, t, ignore=ignore)
        alone, none = _run(x, t, ignore=ignore, want_grad=False)
        assert none is None and _same_bits(with_grad, alone), ignore


def test_two_calls_give_the_same_bits():
    x, y = _case("const", (16, 2, 65, 64))[:2]
    loss, grad = _run(x, y)
    again_loss, again_grad = _run(x, y)
    assert _same_bits(loss, again_loss) and _same_bits(grad, again_grad)
