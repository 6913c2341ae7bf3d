"""``./rs features --geometry centerline --width`` end to end on the MI355X: mask PNGs of one 9-pixel road through the two upper
tiles of a 2 x 2 set -> LineStrings with their widths, with and without ``--stitch``.  What the file must hold is worked out from
the restatements (features_ref, thin_ref, edt_ref on the pasted raster) through the host functions; without ``--width`` the file
is what it was."""

import json
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

from robosat_amd import png  # noqa: E402
from robosat_amd.colors import make_palette  # noqa: E402
from robosat_amd.features import FeatureWriter, Widths, centerlines, centerlines_stitched  # noqa: E402
from robosat_amd.tiles import Tile, pixel_to_location  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, X0, Y0, SIZE = 18, 69623, 104945, 64
TOP, WIDTH = 26, 9  # the road: rows 26..34 of the two upper tiles
WIDTH_KEYS = {"width_px", "width_min_px", "width_max_px", "width_m"}


def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


def road_image():
    image = np.zeros((2 * SIZE, 2 * SIZE), np.uint8)
    image[TOP:TOP + WIDTH, :] = 1
    return image


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("width")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "road"]\ncolors = ["denim", "orange"]\n')
    palette = make_palette("denim", "orange")
    for (x, y), tile in S.split(road_image(), SIZE, SIZE, x0=X0, y0=Y0).items():
        os.makedirs(os.path.join(str(tmp / "masks"), str(Z), str(x)), exist_ok=True)
        png.write_png(os.path.join(str(tmp / "masks"), str(Z), str(x), str(y) + ".png"), tile, "P", palette)
    return {"tmp": tmp, "dataset": str(dataset), "masks": str(tmp / "masks")}


def _run(s, name, extra):
    out = str(s["tmp"] / name)
    done = _rs(["features", s["masks"], "--type", "road", "--dataset", s["dataset"], out, "--denoise", "3", "--grow", "3",
                "--geometry", "centerline"] + extra)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(out, "rb") as fp:
        return fp.read()


def _expected(s, stitch, radius):
    """The file's bytes from the restatements and the host functions; ``radius`` None: without ``--width``."""

    tiles_np = S.split(road_image(), SIZE, SIZE, x0=X0, y0=Y0)
    writer = FeatureWriter()
    if stitch:
        grid = S.Grid(tiles_np, S.margin(3, 3))
        inside = grid.index >= 0
        cleaned = R.clean(grid.canvas, 1, 3, 3) * inside
        labels = grid.global_labels(cleaned)
        rows = T.links(T.thin(cleaned), labels)[:, 1:]
        rows[:, 1:3] -= grid.pad
        d2 = grid.cut(E.edt(np.where(inside, cleaned != 0, E.UNKNOWN), radius, coded=True)) if radius else None
        widths = Widths(lambda c: d2[c[:, 0], c[:, 1], c[:, 2]], radius) if radius else None
        writer.add(centerlines_stitched(rows, grid.table(labels), [Tile(x, y, Z) for x, y in grid.coords], (SIZE, SIZE), widths=widths))
    else:
        coords = sorted(tiles_np)
        cleaned = [R.clean(tiles_np[c], 1, 3, 3) for c in coords]
        labels = [R.label(m) for m in cleaned]
        rows = np.concatenate([T.links(T.thin(m), lab, tile=i) for i, (m, lab) in enumerate(zip(cleaned, labels))])
        table = np.concatenate([R.table(lab, tile=i) for i, lab in enumerate(labels)])
        d2 = np.stack([E.edt(m, radius) for m in cleaned]) if radius else None
        widths = Widths(lambda c: d2[c[:, 0], c[:, 1], c[:, 2]], radius) if radius else None
        writer.add(centerlines(rows, table, [Tile(x, y, Z) for x, y in coords], (SIZE, SIZE), widths=widths))
    out = str(s["tmp"] / "expected.geojson")
    writer.save(out)
    with open(out, "rb") as fp:
        return fp.read()


@pytest.mark.parametrize("stitch", [False, True], ids=["per_tile", "stitch"])
def test_every_line_carries_its_width(setup, stitch):
    got = _run(setup, "width.geojson", ["--width"] + (["--stitch"] if stitch else []))
    doc = json.loads(got)
    assert len(doc["features"]) == (1 if stitch else 2)
    for feature in doc["features"]:
        props = feature["properties"]
        assert WIDTH_KEYS <= set(props), sorted(props)
        # (the chain's middle pixel, index len // 2, lies on the road's middle row, far from either end)
        lat = pixel_to_location(Tile(X0, Y0, Z), 0.5, (TOP + WIDTH // 2 + 0.5) / SIZE)[1]
        resolution = 2 * math.pi * 6378137 * math.cos(math.radians(lat)) / (2 ** Z * SIZE)
        assert props["width_m"] == pytest.approx(props["width_px"] * resolution, rel=1e-9)
        assert props["width_min_px"] <= props["width_px"] <= props["width_max_px"] and "width_capped" not in props
    if stitch:
        assert doc["features"][0]["properties"]["width_px"] == 9.0
    assert got == _expected(setup, stitch, 64 // 2 + 2), "every property as line_width gives it on the restated transform, along the same lines"


@pytest.mark.parametrize("stitch", [False, True], ids=["per_tile", "stitch"])
def test_a_road_wider_than_max_width_is_marked_capped(setup, stitch):
    got = _run(setup, "capped.geojson", ["--width", "--max_width", "4"] + (["--stitch"] if stitch else []))
    for feature in json.loads(got)["features"]:
        assert feature["properties"]["width_capped"] is True and feature["properties"]["width_px"] == 2 * 4 - 1
    assert got == _expected(setup, stitch, 4 // 2 + 2)


@pytest.mark.parametrize("stitch", [False, True], ids=["per_tile", "stitch"])
def test_without_the_flag_the_file_is_what_it_was(setup, stitch):
    got = _run(setup, "plain.geojson", ["--stitch"] if stitch else [])
    assert got == _expected(setup, stitch, None)
    assert got == _run(setup, "plain_max_width.geojson", ["--max_width", "10"] + (["--stitch"] if stitch else [])), "--max_width alone does nothing"
    for feature in json.loads(got)["features"]:
        assert set(feature["properties"]) == {"tile", "component", "length_px", "area_px"} | ({"stitched"} if stitch else set())
