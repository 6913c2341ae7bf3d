"""Restatement in numpy of the free rotation of ``rs train`` (include/robosat_hip.h, rs_augment_tiles_rotate; the draw of
robosat_amd/augment.py): float64 by default, written from the definition and not from the kernel -- whole arrays of fixed-point
source positions, the mirror as an index map, the view made with ``np.fliplr`` / ``np.rot90`` AFTER the rotation instead of undoing
it per pixel.  The colour chain, the normalisation and the view are ``augment_ref.jitter``'s, by import.  The integer maps are also
stated by brute force, from pixel centres in exact fractions.  Not a test module."""

import math
from fractions import Fraction

import numpy as np

import augment_ref as A

ONE = 65536  # the angle's cosine and sine, and the coefficients A and B, are in units of 2**-16


def rot_of(degrees):
    """``(c, s)`` of an angle as the header asks for them: floor(65536 cos + 1/2), floor(65536 sin + 1/2), in Python floats."""

    theta = math.radians(degrees)
    return int(math.floor(ONE * math.cos(theta) + 0.5)), int(math.floor(ONE * math.sin(theta) + 0.5))


# ---- the maps, by definition ---------------------------------------------------------------------------------------------

def coefficients_by_definition(size, w, rot):
    """c * w / S and s * w / S, each rounded to the nearest integer (halves up)."""

    return tuple(int((Fraction(int(v) * w, size) + Fraction(1, 2)).__floor__()) for v in rot)


def position_by_definition(x, y, size, geom, a, b):
    """Where the centre of frame pixel (x, y) falls in the source tile, in pixels (pixel i covers [i, i+1)): its offset from the
    frame's centre, turned and scaled by (a + ib) / 65536, laid at the window's centre."""

    w, x0, y0 = geom
    px, py = Fraction(2 * x + 1 - size, 2), Fraction(2 * y + 1 - size, 2)
    return x0 + Fraction(w, 2) + (a * px - b * py) / ONE, y0 + Fraction(w, 2) + (b * px + a * py) / ONE


def mirror_by_definition(i, size):
    """The tile laid out again and again, every other copy reversed (a mirror at each edge, the edge pixel repeated): the strip has
    period 2S and its second half is the first backwards."""

    r = i % (2 * size)
    return r if r < size else 2 * size - 1 - r


def nearest_by_definition(p):
    return int(p.__floor__())


def bilinear_by_definition(p):
    """``(i0, f)``: in the coordinates whose integers are the pixel CENTRES the position is p - 1/2; it lies a fraction f past
    the centre i0, and the second tap is i0 + 1."""

    c = p - Fraction(1, 2)
    i0 = int(c.__floor__())
    return i0, c - i0


# ---- the integer formulas of the header -----------------------------------------------------------------------------------

def coefficients(size, w, rot):
    c, s = int(rot[0]), int(rot[1])
    return (2 * c * w + size) // (2 * size), (2 * s * w + size) // (2 * size)  # (Python's // is the floor)


def positions(size, geom, rot):
    """``(Ux, Uy)``, int64 [S,S] indexed [y, x]: the source position of every frame pixel's centre in units of 2**-17 pixels."""

    w, x0, y0 = (int(v) for v in geom)
    a, b = coefficients(size, w, rot)
    d = 2 * np.arange(size, dtype=np.int64) + 1 - size
    dx, dy = d[None, :], d[:, None]
    return a * dx - b * dy + (2 * x0 + w) * ONE, b * dx + a * dy + (2 * y0 + w) * ONE


def fold(i, size):
    i = np.asarray(i, dtype=np.int64)
    return np.where(i < 0, -1 - i, np.where(i >= size, 2 * size - 1 - i, i))


def nearest_index(u):
    return u >> 17


def bilinear_index(u, dtype=np.float64):
    """``(i0, f)`` of one axis; the second tap is i0 + 1.  f is a 17-bit integer over 2**17: exact in float32 too."""

    t = u - ONE
    return t >> 17, (t & 131071).astype(dtype) / dtype(131072)


# ---- one item --------------------------------------------------------------------------------------------------------------

class _Interpolated(np.ndarray):
    """The interpolated values standing where ``augment_ref.jitter`` takes its tile, so that the colour chain is that module's
    and not a copy.  With the whole-tile window its zoom reads every value itself (i0 = j, f = 0: a + 0 * (b - a)); the one thing
    it asks of the tile besides the values is the band sums of the contrast stage, ``tile.reshape(-1, bands)`` summed, and those
    stay the SOURCE tile's, so ``reshape`` hands out the source."""

    def __new__(cls, values, source):
        obj = np.asarray(values).view(cls)
        obj.source = source
        return obj

    def __array_finalize__(self, obj):
        self.source = getattr(obj, "source", None)

    def reshape(self, *shape, **kwargs):
        return self.source.reshape(*shape, **kwargs)


def rotate(image_u8, mask_u8, op, geom, rot, color, mean, std, rgb, dtype=np.float64):
    """image uint8 [S,S,C], mask uint8 [S,S] -> (image ``dtype`` [C,S,S], mask int64 [S,S]) for the window ``geom`` = (w, x0, y0)
    turned by ``rot`` = (c, s) and the factors ``color``.  ``dtype=np.float32`` is the same chain rounded after every operation."""

    size = image_u8.shape[0]
    ux, uy = positions(size, geom, rot)
    turned_mask = mask_u8[fold(nearest_index(uy), size), fold(nearest_index(ux), size)]

    src = image_u8.astype(dtype)
    (xi, fx), (yi, fy) = bilinear_index(ux, dtype), bilinear_index(uy, dtype)
    xa, xb, ya, yb = fold(xi, size), fold(xi + 1, size), fold(yi, size), fold(yi + 1, size)
    fx, fy = fx[..., None], fy[..., None]
    p00, p01, p10, p11 = src[ya, xa], src[ya, xb], src[yb, xa], src[yb, xb]
    top = p00 + fx * (p01 - p00)
    bot = p10 + fx * (p11 - p10)
    v = top + fy * (bot - top)
    assert v.dtype == dtype
    return A.jitter(_Interpolated(v, image_u8), turned_mask, op, (size, 0, 0), color, mean, std, rgb, dtype)


def sample_range(size, geom, rot):
    """``(lowest, highest)`` unfolded index any sample of the item reads, over both axes, the mask's and the image's four taps."""

    ux, uy = positions(size, geom, rot)
    lo = min(int(bilinear_index(u)[0].min()) for u in (ux, uy))
    hi = max(int(bilinear_index(u)[0].max()) + 1 for u in (ux, uy))
    return min(lo, int(min(nearest_index(ux).min(), nearest_index(uy).min()))), max(hi, int(max(nearest_index(ux).max(), nearest_index(uy).max())))


# ---- the cases of the GPU tests ----------------------------------------------------------------------------------------------

SIZES = (5, 8, 33, 96)  # one pixel per thread at 5 and 33, four at 8 and 96
ANGLES = (7, -30, 45, -45, 133, 179.999)
INDEX = [4, 0, 2, 2, 1, 3, 0, 4]  # five cached tiles, eight items, out of order


def make_case(images, masks, index, op, geom, rot, color, rgb):
    return dict(A.make_case(images, masks, index, op, geom, color, rgb), rot=[(int(c), int(s)) for c, s in rot])


def oracle(case, n, dtype=np.float64):
    i = case["index"][n]
    return rotate(case["images"][i], case["masks"][i], case["op"][n], case["geom"][n], case["rot"][n], case["color"][n], case["mean"],
                  case["std"], case["rgb"], dtype)


def image_cases():
    """``(name, case)``: per size the six angles crossed with the four ``augment_ref.corner_windows`` of zoom 4, eight items a launch
    over all eight ops, once with identity colour and once with all four stages and different factors per item; then one, two and
    four bands once each."""

    for size in SIZES:
        images, masks = A.tiles(140 + size, 5, size, 3)
        cross = [(angle, win) for angle in ANGLES for win in A.corner_windows(size, 4)]
        rng = np.random.default_rng(150 + size)
        for k in range(0, len(cross), 8):
            part = cross[k:k + 8]
            geom, rot = [win for _, win in part], [rot_of(angle) for angle, _ in part]
            ops = A.OPS[k // 8:] + A.OPS[:k // 8]  # (another op for a given window from launch to launch)
            color = [tuple(lo + rng.random() * (hi - lo) for lo, hi in A.RANGES.values()) for _ in range(8)]
            yield "plain-S{}-{}".format(size, k // 8), make_case(images, masks, INDEX, ops, geom, rot, [A.IDENTITY_COLOR] * 8, True)
            yield "all-S{}-{}".format(size, k // 8), make_case(images, masks, INDEX, ops, geom, rot, color, True)
    for bands, rgb, size in ((1, False, 33), (2, False, 8), (4, True, 96)):
        images, masks = A.tiles(160 + bands, 5, size, bands)
        win = A.corner_windows(size, 4)
        rng = np.random.default_rng(170 + bands)
        color = [tuple(lo + rng.random() * (hi - lo) for lo, hi in A.RANGES.values()) for _ in range(8)]
        geom, rot = [win[n % 4] for n in range(8)], [rot_of(ANGLES[n % 6]) for n in range(8)]
        yield "all-S{}-C{}".format(size, bands), make_case(images, masks, INDEX, A.OPS[::-1], geom, rot, color, rgb)
