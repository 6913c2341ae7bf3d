"""``rs features --width`` without a GPU: the restated distance transform (``edt_ref``) against brute force and scipy, the width
arithmetic (``features.line_width``), the untouched default of ``centerlines``, the boundary (header, signatures, ABI) and the
command line's error exits."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edt_ref as E  # noqa: E402
import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import _lib, png  # noqa: E402
from robosat_amd.colors import make_palette  # noqa: E402
from robosat_amd.features import (Widths, centerlines, centerlines_stitched, ground_resolution, line_width, mosaic_slots,  # noqa: E402
                                  prune_lines, link_lines)
from robosat_amd.tiles import Tile, pixel_to_location  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- edt_ref ---------------------------------------------------------------------------------------------------------------
def test_the_two_passes_equal_brute_force_on_tiny_rasters_with_unknown_pixels():
    rng = np.random.RandomState(0)
    for _ in range(150):
        h, w = rng.randint(1, 24, 2)
        radius = int(rng.randint(1, 14))
        mask = rng.rand(h, w) < rng.choice([0.5, 0.8, 0.95])
        assert (E.edt(mask, radius) == E.edt_brute(mask, radius)).all()
        coded = rng.choice([E.UNSET, E.SET, E.UNKNOWN], size=(h, w), p=[0.15, 0.6, 0.25])
        got = E.edt(coded, radius, coded=True)
        assert (got == E.edt_brute(coded, radius, coded=True)).all()
        assert (got[coded != E.SET] == 0).all() and (got[coded == E.SET] >= 1).all() and got.max(initial=0) <= radius * radius


def test_the_stitched_form_equals_brute_force_with_absent_tiles():
    """The unset pixels of a corner tile count although the tile between is absent."""

    rng = np.random.RandomState(1)
    for _ in range(40):
        h, w = rng.randint(3, 8, 2)
        radius = int(rng.randint(1, min(h, w) + 1))
        image = (rng.rand(3 * h, 3 * w) < 0.9).astype(np.uint8)
        absent = [(c, r) for c in range(3) for r in range(3) if rng.rand() < 0.35][:8]
        grid = S.Grid(S.split(image, h, w, absent=absent), 0)
        assert (E.edt_stitched(grid, radius) == E.edt_stitched(grid, radius, brute=True)).all()
    # tiles (1, 0) and (0, 1) meet at a corner only; (0, 0) and (1, 1) are absent.  The one unset pixel is (1, 0)'s bottom left
    corner = np.ones((4, 4), np.uint8)
    corner[3, 0] = 0
    got = E.edt_stitched(S.Grid({(1, 0): corner, (0, 1): np.ones((4, 4), np.uint8)}, 0), 4)  # slots: (0, 1), then (1, 0)
    assert got[1][3, 0] == 0 and got[0][0, 3] == 2, "one across, one up"
    assert got[0][3, 0] == 16 and got[0][1, 3] == 1 + 4 and got[1][1, 2] == 4 + 4 and got[1][0, 3] == 16, "9 + 9 is beyond the cap"


def _scipy_capped(mask, radius):
    ndimage = pytest.importorskip("scipy.ndimage")
    padded = np.pad(np.asarray(mask) != 0, radius, constant_values=True)
    if padded.all():
        return np.where(np.asarray(mask) != 0, radius * radius, 0)
    d2 = np.rint(ndimage.distance_transform_edt(padded) ** 2).astype(np.int64)[radius:-radius, radius:-radius]
    return np.where(np.asarray(mask) != 0, np.minimum(d2, radius * radius), 0)


@pytest.mark.parametrize("h,w,radius", [(70, 45, 1), (70, 45, 7), (33, 130, 33), (128, 128, 128), (5, 3, 4)])
def test_the_restatement_equals_scipy_padded_with_set_pixels(h, w, radius):
    """Padding with set pixels is "outside is unknown" as long as the pad is as wide as the cap."""

    masks = {"random": np.random.RandomState(h + w).rand(h, w) < 0.9, "roads": T.roads(h, w, 3), "ones": np.ones((h, w), bool),
             "zeros": np.zeros((h, w), bool)}
    for name, mask in masks.items():
        assert (E.edt(mask, radius) == _scipy_capped(mask, radius)).all(), name


# ---- line_width ------------------------------------------------------------------------------------------------------------
def _road(rows, length=60, top=20):
    m = np.zeros((64, length), bool)
    m[top:top + rows] = True
    return m


@pytest.mark.parametrize("rows,want", [(13, 13.0), (12, 11.0), (9, 9.0), (1, 1.0), (2, 1.0)])
def test_an_axis_parallel_road_reads_its_odd_width_and_one_less_than_its_even_width(rows, want):
    road = _road(rows)
    skeleton = T.thin(road)
    ys, xs = np.nonzero(skeleton)
    inner = (xs > rows) & (xs < road.shape[1] - rows)
    assert len(set(ys[inner])) == 1, "the skeleton of a bar is one row"
    d2 = E.edt(road, 34)[ys[inner], xs[inner]]
    assert line_width(d2, 34) == {"width_px": want, "width_min_px": want, "width_max_px": want}


def test_median_extremes_rounding_and_the_capped_mark():
    got = line_width([4, 9, 9, 16, 100], 34)  # widths 3, 5, 5, 7, 19
    assert got == {"width_px": 5.0, "width_min_px": 3.0, "width_max_px": 19.0}
    got = line_width([2, 5], 34)  # 2 sqrt 2 - 1 and 2 sqrt 5 - 1: the median of two is their mean
    assert got == {"width_px": round(math.sqrt(2) + math.sqrt(5) - 1, 3), "width_min_px": 1.828, "width_max_px": 3.472}
    assert "width_capped" not in line_width([15, 9], 4) and "width_capped" not in line_width([16, 9], 5)
    assert line_width([16, 9], 4) == {"width_px": 6.0, "width_min_px": 5.0, "width_max_px": 7.0, "width_capped": True}
    for bad in ([], [17], [-1]):
        with pytest.raises(ValueError):
            line_width(bad, 4)


# ---- centerlines -------------------------------------------------------------------------------------------------------------
def _junction():
    m = np.zeros((64, 64), bool)
    m[20:33, :] = True  # 13 rows
    m[33:, 30:37] = True  # a 7-column road down from it
    return m


def _host_inputs(mask):
    labels = R.label(mask)
    return T.links(T.thin(mask), labels), R.table(labels)


def test_without_widths_the_features_are_what_they_were():
    links, table = _host_inputs(_junction())
    tile = Tile(69623, 104945, 18)
    plain = centerlines(links, table, [tile], (64, 64))
    assert plain == centerlines(links, table, [tile], (64, 64), widths=None) and len(plain) >= 2
    assert all(set(f["properties"]) == {"tile", "component", "length_px", "area_px"} for f in plain)
    stitched_rows = np.asarray(links)[:, 1:]
    stitched_table = np.asarray(table)[:, 1:]
    plain = centerlines_stitched(stitched_rows, stitched_table, [tile], (64, 64))
    assert plain == centerlines_stitched(stitched_rows, stitched_table, [tile], (64, 64), widths=None)
    assert all(set(f["properties"]) == {"tile", "component", "length_px", "area_px", "stitched"} for f in plain)


def test_widths_are_sampled_once_per_call_along_the_pruned_chains():
    mask = _junction()
    links, table = _host_inputs(mask)
    tile = Tile(69623, 104945, 18)
    d2 = E.edt(mask, 34)[None]
    calls = []

    def sample(coords):
        assert coords.dtype == np.int32 and coords.shape[1] == 3
        calls.append(len(coords))
        return d2[coords[:, 0], coords[:, 1], coords[:, 2]]

    plain = centerlines(links, table, [tile], (64, 64))
    got = centerlines(links, table, [tile], (64, 64), widths=Widths(sample, 34))
    lines = prune_lines(link_lines(np.asarray(links).reshape(-1, 5)), 20)
    assert calls == [sum(len(p) for _, _, p in lines)], "one call over every chain pixel of the batch"
    assert len(got) == len(plain) == len(lines)
    for with_width, without, (_, _, points) in zip(got, plain, lines):
        assert with_width["geometry"] == without["geometry"]
        props = dict(with_width["properties"])
        width = line_width(d2[0][points[:, 1], points[:, 0]], 34)
        px, py = points[len(points) // 2]
        lat = pixel_to_location(tile, (px + 0.5) / 64, (py + 0.5) / 64)[1]
        want_m = width["width_px"] * 2 * math.pi * 6378137 * math.cos(math.radians(lat)) / (2 ** 18 * 64)
        assert props.pop("width_m") == pytest.approx(want_m, rel=1e-12)
        assert props == dict(without["properties"], **width)
    assert sorted(f["properties"]["width_px"] for f in got)[0] == 7.0 and max(f["properties"]["width_px"] for f in got) == 13.0
    assert ground_resolution(0.0, 0, 256) == pytest.approx(156543.03392804097)

    # the stitched form: the same raster as a call of one tile, in mosaic pixels
    calls.clear()
    stitched = centerlines_stitched(np.asarray(links)[:, 1:], np.asarray(table)[:, 1:], [tile], (64, 64), widths=Widths(sample, 34))
    assert len(calls) == 1
    assert sorted(f["properties"]["width_px"] for f in stitched) == sorted(f["properties"]["width_px"] for f in got)
    assert all(f["properties"]["stitched"] is True and "width_m" in f["properties"] for f in stitched)


def test_mosaic_pixels_map_to_slot_row_column_through_the_calls_tiles():
    tiles = [Tile(5, 7, 18), Tile(5, 8, 18), Tile(6, 8, 18)]  # slot order (z, x, y); (6, 7) is absent
    got = mosaic_slots(tiles, [[0, 0], [9, 3], [3, 4 + 2], [10 + 1, 4 + 3]], (4, 10))
    assert got.tolist() == [[0, 0, 0], [0, 3, 9], [1, 2, 3], [2, 3, 1]]
    with pytest.raises(ValueError):
        mosaic_slots(tiles, [[10, 0]], (4, 10))
    with pytest.raises(ValueError):
        mosaic_slots(tiles, [[20, 0]], (4, 10))


# ---- boundary ------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_bound_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    assert "int rs_features_edt(const uint8_t* masks, const int32_t* nbr, uint8_t* g, int32_t* d2, int B, int H, int W, int R, rs_stream_t stream);" in header
    assert "rs_features_edt" in _lib.SIGNATURES and len(_lib.SIGNATURES["rs_features_edt"][1]) == 9
    assert _lib.ABI_VERSION == 24


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def small_tiles(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("width_cli")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "road"]\ncolors = ["denim", "orange"]\n')
    for x in (69623, 69624):
        os.makedirs(str(tmp / "masks" / "18" / str(x)), exist_ok=True)
        png.write_png(str(tmp / "masks" / "18" / str(x) / "104945.png"), np.ones((24, 20), np.uint8), "P", make_palette("denim", "orange"))
    return [str(tmp / "masks"), "--type", "road", "--dataset", str(dataset), str(tmp / "out.geojson")]


@pytest.mark.parametrize("extra,message", [
    (["--width"], "Error: --width measures along centerlines: only with --geometry centerline"),
    (["--width", "--geometry", "polygon", "--stitch"], "Error: --width measures along centerlines: only with --geometry centerline"),
    (["--width", "--geometry", "centerline", "--max_width", "0"], "Error: --max_width must be in 1..252"),
    (["--width", "--geometry", "centerline", "--max_width", "253"], "Error: --max_width must be in 1..252"),
    (["--width", "--geometry", "centerline", "--stitch"],
     "Error: --max_width 64 needs a border of 34 pixels from the neighbouring tiles; tiles of 24x20 take at most 20"),
    (["--width", "--geometry", "centerline", "--stitch", "--max_width", "38"],
     "Error: --max_width 38 needs a border of 21 pixels from the neighbouring tiles; tiles of 24x20 take at most 20"),
], ids=["no_geometry", "polygon", "max_width_0", "max_width_253", "stitch_default", "stitch_21"])
def test_the_error_exits_come_before_any_device_is_asked_for(small_tiles, extra, message):
    done = _rs(["features"] + small_tiles + extra)
    assert done.returncode != 0 and done.stderr.strip().splitlines()[-1] == message, done.stderr[-2000:]
