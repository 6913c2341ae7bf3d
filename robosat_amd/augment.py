"""The ``[augment]`` table of the model config: a random zoom-in crop and photometric jitter for ``rs train``, on top of the
reference's eight views (an extension; the reference has neither).

    [augment]
      zoom       = 1.5          # largest zoom-in factor, 1 <= zoom <= 4 (1 = off)
      brightness = [0.8, 1.2]   # each: [lo, hi], 0 < lo <= hi <= 4
      contrast   = [0.8, 1.2]
      saturation = [0.8, 1.2]   # needs the first image source in mode RGB or RGBA (robosat_amd.bands)
      gamma      = [0.8, 1.25]
      rotate     = 180          # largest turn of the window about its centre in degrees, 0 <= rotate <= 180 (0 = off)

An absent key is the identity; an absent table is the loaders as they are without this module.  The table applies to the
training split only.  Everything here is host logic: the parsing, and the seven draws per item that follow the four of
``datasets.draw_flip_rotations`` -- eight with ``rotate``, whose draw is made only when the key is set, so that a table without
it yields the batches it always did.  The pixels are made on the device (``ops.augment_tiles_jitter``, or
``ops.augment_tiles_rotate`` for every item of a table with ``rotate``; csrc/augment.hip); what the window, the angle and the
factors mean is stated in include/robosat_hip.h.
"""

import collections
import math
import random

KEYS = ("zoom", "brightness", "contrast", "saturation", "gamma", "rotate")
MAX_ZOOM = MAX_FACTOR = 4.0
MAX_ROTATE = 180.0
ROT_ONE = 65536  # the angle travels as (cos, sin) in units of 2**-16

Jitter = collections.namedtuple("Jitter", ["zoom", "brightness", "contrast", "saturation", "gamma", "rgb", "rotate"], defaults=(0.0,))


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def jitter_from_config(model, bands):
    """The ``Jitter`` of a model config's ``[augment]`` table, or None when it has none.  ``bands`` (``robosat_amd.bands.Bands``)
    says whether bands 0..2 are R, G, B.  Raises ``ValueError("[augment] <key> ...")`` on an unknown key or a bad value."""

    table = model.get("augment")
    if table is None:
        return None
    if not isinstance(table, dict):
        raise ValueError("[augment] must be a table")
    for key in table:
        if key not in KEYS:
            raise ValueError("[augment] {} is not a known key (one of {})".format(key, ", ".join(KEYS)))
    zoom = table.get("zoom", 1.0)
    if not _number(zoom) or not 1.0 <= zoom <= MAX_ZOOM:
        raise ValueError("[augment] zoom must be a number in 1..{:g} (the largest zoom-in factor; 1 = off), got {!r}".format(MAX_ZOOM, zoom))
    ranges = {}
    for key in KEYS[1:5]:
        r = table.get(key, [1.0, 1.0])
        if not (isinstance(r, (list, tuple)) and len(r) == 2 and all(_number(v) for v in r) and 0.0 < r[0] <= r[1] <= MAX_FACTOR):
            raise ValueError("[augment] {} must be [lo, hi] with 0 < lo <= hi <= {:g}, got {!r}".format(key, MAX_FACTOR, r))
        ranges[key] = (float(r[0]), float(r[1]))
    rgb = bands.modes[0] in ("RGB", "RGBA")
    if ranges["saturation"] != (1.0, 1.0) and not rgb:
        raise ValueError("[augment] saturation needs the first image source in mode RGB or RGBA; [common] image_modes gives {!r}"
                         .format(bands.modes[0]))
    rotate = table.get("rotate", 0.0)
    if not _number(rotate) or not 0.0 <= rotate <= MAX_ROTATE:
        raise ValueError("[augment] rotate must be a number of degrees in 0..{:g} (the largest turn either way; 0 = off), got {!r}"
                         .format(MAX_ROTATE, rotate))
    return Jitter(float(zoom), ranges["brightness"], ranges["contrast"], ranges["saturation"], ranges["gamma"], rgb, float(rotate))


def describe(jitter):
    """The table as one line of the training log."""

    line = "zoom <= {:g}, brightness {}, contrast {}, saturation {}, gamma {}".format(
        jitter.zoom, *("[{:g}, {:g}]".format(*r) for r in (jitter.brightness, jitter.contrast, jitter.saturation, jitter.gamma)))
    return line + ", rotate <= {:g} deg".format(jitter.rotate) if jitter.rotate > 0 else line


def window(size, zoom, r_w, r_x, r_y):
    """``(w, x0, y0)``: the square window of the source tile that three uniform draws pick, ``ceil(size / zoom) <= w <= size``."""

    wmin = int(math.ceil(size / zoom))
    w = size - int(r_w * (size - wmin + 1))
    return w, int(r_x * (size - w + 1)), int(r_y * (size - w + 1))


def draw_jitter(jitter, size):
    """The seven draws of one item, from Python's ``random`` in the fixed order r_w, r_x, r_y, r_b, r_k, r_s, r_g whatever
    keys are set (switching one key on never shifts the others): ``((w, x0, y0), (brightness, contrast, saturation, gamma))``.
    A factor is ``lo + r * (hi - lo)`` in Python floats (the caller stores it as float32)."""

    r = [random.random() for _ in range(7)]
    geom = window(size, jitter.zoom, r[0], r[1], r[2])
    color = tuple(lo + v * (hi - lo) for v, (lo, hi) in zip(r[3:], (jitter.brightness, jitter.contrast, jitter.saturation, jitter.gamma)))
    return geom, color


def rotation(rotate, r_a):
    """``(c, s)``: the angle theta = (2 r_a - 1) * rotate degrees that one uniform draw picks, as the two integers the kernel
    takes, floor(65536 cos theta + 1/2) and floor(65536 sin theta + 1/2)."""

    theta = math.radians((2.0 * r_a - 1.0) * rotate)
    return int(math.floor(ROT_ONE * math.cos(theta) + 0.5)), int(math.floor(ROT_ONE * math.sin(theta) + 0.5))


def draw_rotation(jitter):
    """The eighth draw of one item, r_a, behind the seven of ``draw_jitter``.  The caller makes it only when ``jitter.rotate > 0``:
    a table without the key consumes the draws it always did."""

    return rotation(jitter.rotate, random.random())
