"""Restatement in numpy of the zoom and colour jitter of ``rs train`` (include/robosat_hip.h, rs_augment_tiles_jitter; the draws of
robosat_amd/augment.py): float64 by default, written from the definitions and not from the kernel -- whole arrays, the view made
with ``np.fliplr`` / ``np.rot90`` AFTER the zoom instead of undoing it per pixel.  The integer maps of the header are also stated
by brute force, from pixel centres in exact fractions.  Not a test module."""

from fractions import Fraction

import numpy as np

LUMA = (0.299, 0.587, 0.114)


# ---- the two maps, by definition -----------------------------------------------------------------------------------------

def nearest_by_definition(j, w, size):
    """Frame pixel j covers [j, j+1) of a frame of ``size`` pixels laid over a window of ``w``: its centre, in window pixels,
    falls into window pixel floor((j + 1/2) * w / size)."""

    return int((Fraction(2 * j + 1, 2) * Fraction(w, size)).__floor__())


def bilinear_by_definition(j, w, size):
    """``(i0, i1, f)``: the centre of frame pixel j in the coordinates whose integers are the window's pixel CENTRES is
    (j + 1/2) * w / size - 1/2, kept inside the window; it lies between the centres i0 and i1 = i0 + 1 (or on the last one), a
    fraction f past i0."""

    c = Fraction(2 * j + 1, 2) * Fraction(w, size) - Fraction(1, 2)
    c = min(max(c, Fraction(0)), Fraction(w - 1))
    i0 = int(c.__floor__())
    return i0, min(i0 + 1, w - 1), c - i0


# ---- the integer formulas of the header -------------------------------------------------------------------------------------

def nearest_index(size, w):
    j = np.arange(size, dtype=np.int64)
    return ((2 * j + 1) * w) // (2 * size)


def bilinear_index(size, w, dtype=np.float64):
    j = np.arange(size, dtype=np.int64)
    t = np.maximum((2 * j + 1) * w - size, 0)
    i0 = t // (2 * size)
    f = (t % (2 * size)).astype(dtype) / dtype(2 * size)
    return i0, np.minimum(i0 + 1, w - 1), f


# ---- one item --------------------------------------------------------------------------------------------------------------

def view(a, op):
    """op = f + 2*k on an [S,S,...] array: FLIP_LEFT_RIGHT when f, then k counter-clockwise quarter turns."""

    if op & 1:
        a = np.fliplr(a)
    return np.rot90(a, (op >> 1) & 3)


def jitter(image_u8, mask_u8, op, geom, color, mean, std, rgb, dtype=np.float64):
    """image uint8 [S,S,C], mask uint8 [S,S] -> (image ``dtype`` [C,S,S], mask int64 [S,S]) for the window ``geom`` = (w, x0, y0)
    and the factors ``color`` = (brightness, contrast, saturation, gamma).  ``dtype=np.float32`` is the same chain rounded after
    every operation (what an fp32 implementation without fused multiply-adds computes)."""

    size, _, bands = image_u8.shape
    w, x0, y0 = (int(v) for v in geom)
    b, k, s, g = (dtype(np.float32(v)) for v in color)  # (the factors are float32 values)
    one = dtype(1)
    src = image_u8.astype(dtype)

    near = nearest_index(size, w)
    out_mask = mask_u8[np.ix_(y0 + near, x0 + near)].astype(np.int64)

    i0, i1, f = bilinear_index(size, w, dtype)
    ya, yb, xa, xb = y0 + i0, y0 + i1, x0 + i0, x0 + i1
    fx, fy = f[None, :, None], f[:, None, None]
    p00, p01 = src[np.ix_(ya, xa)], src[np.ix_(ya, xb)]
    p10, p11 = src[np.ix_(yb, xa)], src[np.ix_(yb, xb)]
    top = p00 + fx * (p01 - p00)
    bot = p10 + fx * (p11 - p10)
    v = top + fy * (bot - top)

    v = v / dtype(255)
    if b != one:
        v = np.clip(v * b, 0, 1)
    if k != one:
        sums = image_u8.reshape(-1, bands).astype(np.int64).sum(axis=0)
        m = (sums.astype(np.float64) / (float(size) * float(size) * 255.0)).astype(dtype)
        v = np.clip(m + k * (v - m), 0, 1)
    if rgb and s != one:
        grey = dtype(np.float32(LUMA[0])) * v[..., 0] + dtype(np.float32(LUMA[1])) * v[..., 1] + dtype(np.float32(LUMA[2])) * v[..., 2]
        v = v.copy()
        v[..., :3] = np.clip(grey[..., None] + s * (v[..., :3] - grey[..., None]), 0, 1)
    if g != one:
        v = np.clip(np.power(v, g), 0, 1)
    v = (v - np.asarray(mean, dtype=np.float32).astype(dtype)) / np.asarray(std, dtype=np.float32).astype(dtype)
    assert v.dtype == dtype
    return np.ascontiguousarray(view(v, op).transpose(2, 0, 1)), np.ascontiguousarray(view(out_mask, op))


IDENTITY_COLOR = (1.0, 1.0, 1.0, 1.0)
BAND_MEAN, BAND_STD = [0.485, 0.456, 0.406, 0.449], [0.229, 0.224, 0.225, 0.226]
RANGES = {"brightness": (0.8, 1.2), "contrast": (0.8, 1.2), "saturation": (0.8, 1.2), "gamma": (0.8, 1.25)}  # (the README's table)
OPS = [0, 1, 2, 3, 4, 5, 6, 7]


def tiles(seed, count, size, bands):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(count, size, size, bands), dtype=np.uint8), rng.integers(0, 3, size=(count, size, size), dtype=np.uint8)


def make_case(images, masks, index, op, geom, color, rgb):
    bands = images.shape[3]
    return dict(images=images, masks=masks, index=list(index), op=list(op), geom=[tuple(g) for g in geom],
                color=[tuple(float(np.float32(v)) for v in c) for c in color], mean=BAND_MEAN[:bands], std=BAND_STD[:bands], rgb=rgb)


def image_cases():
    """``(name, case)``: the launches whose images the GPU tests compare with ``jitter`` -- eight items each (all eight ops, the
    cache indexed out of order, the four ``corner_windows`` of zoom 4 twice) at an odd size (one pixel per thread) and at a
    multiple of four (four per thread): every stage alone at both ends of its range, the zoom alone, all stages with different
    factors per item, four bands of which three are colour, and one or two bands that are not."""

    index = [4, 0, 2, 2, 1, 3, 0, 4]
    for size in (33, 96):
        win = corner_windows(size, 4)
        geom = [win[n % 4] for n in range(8)]
        images, masks = tiles(40 + size, 5, size, 3)
        ends = []
        for stage in range(4):
            for v in list(RANGES.values())[stage]:
                ends.append(tuple(v if k == stage else 1.0 for k in range(4)))
        yield "ends-S{}".format(size), make_case(images, masks, index, OPS, [geom[(n + 1) % 8] for n in range(8)], ends, True)
        yield "zoom-S{}".format(size), make_case(images, masks, index, OPS, geom, [IDENTITY_COLOR] * 8, True)
        rng = np.random.default_rng(50 + size)
        for bands, rgb in ((3, True), (4, True), (1, False), (2, False)):
            if bands != 3:
                images, masks = tiles(60 + size + bands, 5, size, bands)
            color = [tuple(lo + rng.random() * (hi - lo) for lo, hi in RANGES.values()) for _ in range(8)]
            yield "all-S{}-C{}".format(size, bands), make_case(images, masks, index, OPS[::-1], geom, color, rgb)


def corner_windows(size, zoom):
    """The windows the tests run: the whole tile, the smallest window in the first and in the last corner (the clamped right and
    bottom taps), and one in the interior."""

    wmin = -(-size // zoom)
    mid = (wmin + size) // 2
    return [(size, 0, 0), (wmin, 0, 0), (wmin, size - wmin, size - wmin), (mid, (size - mid) // 2, max(size - mid - 1, 0))]
