"""``rs features --split`` without a GPU: the restatement of the definition (tests/split_ref.py; include/robosat_hip.h) on shapes
whose answer can be written down by hand, the host half (ring linking, featurize) on its labels, and the command line's error exits.
Everything is integer-exact."""

import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edt_ref as E  # noqa: E402
import features_ref as R  # noqa: E402
import split_ref as P  # noqa: E402

from robosat_amd import _lib, png  # noqa: E402
from robosat_amd import features as F  # noqa: E402
from robosat_amd.colors import make_palette  # noqa: E402
from robosat_amd.tiles import Tile  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the dumbbell of split_ref.dumbbell(): squares at columns 4..24 and 34..54, rows 8..28; the neck rows 17..19, columns 25..33
LEFT, NECK, RIGHT, ROWS, NECK_ROWS = slice(4, 25), slice(25, 34), slice(34, 55), slice(8, 29), slice(17, 20)


def test_a_step_takes_the_first_labelled_neighbour_in_the_order_n_w_e_s():
    around = {"n": (0, 1), "w": (1, 0), "e": (1, 2), "s": (2, 1)}
    for present, want in (("nwes", "n"), ("wes", "w"), ("es", "e"), ("s", "s"), ("ne", "n"), ("ws", "w")):
        raster = np.zeros((3, 3), dtype=np.int64)
        raster[1, 1] = -1
        for k, name in enumerate("nwes"):
            if name in present:
                raster[around[name]] = 40 - 10 * k  # (the label's value plays no part: N holds the largest, S the smallest)
        after = P.step(raster)
        assert after[1, 1] == raster[around[want]], present
        after[1, 1] = -1
        assert (after == raster).all(), "nothing else changes"
    lone = np.array([[0, -1, 0], [-1, -1, -1], [0, -1, 0]])
    assert (P.step(lone) == lone).all(), "-1 neighbours and the outside give nothing"
    jacobi = np.array([[7, -1, -1, -1]])
    assert P.step(jacobi).tolist() == [[7, 7, -1, -1]], "one pixel per step: a label set in this step is not seen in it"


def test_the_dumbbell_gives_two_labels_and_the_cut_lies_inside_the_neck():
    mask = P.dumbbell()
    assert mask.sum() == 2 * 21 * 21 + 3 * 9 and len(np.unique(R.label(mask))) == 2
    cores = P.seeds(mask, 4)
    assert not cores[:, NECK].any() and cores[18, 14] and cores[18, 44], "a disc of radius 4 fits the squares, not the neck"
    labels = P.split(mask, 4)
    assert ((labels != 0) == mask).all()
    a, b = int(labels[18, 14]), int(labels[18, 44])
    assert a != b and sorted(np.unique(labels).tolist()) == sorted([0, a, b])
    assert (labels[ROWS, LEFT] == a).all() and (labels[ROWS, RIGHT] == b).all()
    assert a == 1 + np.flatnonzero(R.label(cores) == R.label(cores)[18, 14])[0], "a core is named by its smallest pixel"
    assert labels.ravel()[a - 1] == a and labels.ravel()[b - 1] == b, "and that pixel keeps the name: L[root] == root + 1"


def test_the_symmetric_dumbbells_pin_the_tie_break_pixel_by_pixel():
    """Both fronts reach the neck's middle in the same step: the pixel there sees W before E (N before S in the vertical one), so the
    middle column (row) goes to the left (upper) instance."""

    labels = P.split(P.dumbbell(), 4)
    a, b = int(labels[18, 14]), int(labels[18, 44])
    want = np.zeros((64, 64), dtype=np.int32)
    want[ROWS, LEFT], want[ROWS, RIGHT] = a, b
    want[NECK_ROWS, 25:30], want[NECK_ROWS, 30:34] = a, b  # the neck's nine columns: five to the left, four to the right
    assert (labels == want).all()
    upright = P.split(P.dumbbell(vertical=True), 4)
    a, b = int(upright[14, 18]), int(upright[44, 18])
    assert a != b and (upright == np.where(want.T == want[18, 14], a, np.where(want.T == want[18, 44], b, 0))).all()


def test_a_component_thinner_than_the_disc_keeps_its_own_label():
    mask = P.dumbbell()
    mask[40:45, 3:60] = True  # 5 high: no disc of radius 4 fits
    mask[50, 50] = True
    own = R.label(mask)
    labels = P.split(mask, 4)
    assert (labels[40:45, 3:60] == own[40, 3]).all() and labels[50, 50] == own[50, 50] == 1 + 50 * 64 + 50
    assert len(np.unique(labels)) == 1 + 4
    assert (labels[ROWS] == P.split(P.dumbbell(), 4)[ROWS]).all(), "and the others are split as they were"


def test_a_blob_with_a_long_one_pixel_tail_is_one_label_tail_included():
    mask = np.zeros((40, 90), dtype=bool)
    mask[5:26, 5:26] = True
    mask[15, 26:88] = True
    mask[15:38, 87] = True
    labels, steps = P.grow(P.start_of(mask, 4), want_steps=True)
    assert steps >= 62 + 22 and sorted(np.unique(labels).tolist()) == [0, int(labels[15, 15])]
    assert ((labels != 0) == mask).all()


def test_all_background_and_all_foreground():
    assert (P.split(np.zeros((9, 13), dtype=bool), 3) == 0).all()
    full = np.ones((9, 13), dtype=bool)
    assert P.seeds(full, 3).all(), "nothing unset anywhere: the whole raster is one core"
    assert (P.start_of(full, 3) == 1).all() and (P.split(full, 3) == 1).all()


def test_an_object_cut_by_the_rasters_edge_is_not_eroded_from_that_edge():
    mask = np.zeros((30, 30), dtype=bool)
    mask[:12, :12] = True
    cores = P.seeds(mask, 4)
    assert cores[:9, :9].all() and not cores[9:, :].any() and not cores[:, 9:].any()
    inside = np.pad(mask, 6)  # the same square away from the edge loses its rim on every side
    assert (P.seeds(inside, 4)[6:36, 6:36] == np.pad(np.ones((6, 6), dtype=bool), ((3, 21), (3, 21)))).all()
    coded = np.where(mask, E.SET, E.UNSET)
    coded[:, 20:] = E.UNKNOWN  # an absent tile beside it is the outside too
    assert (P.seeds(coded, 4, coded=True) == cores).all()


def test_the_host_half_makes_two_valid_polygons_of_the_dumbbell():
    mask = P.dumbbell()
    labels = P.split(mask, 4)
    edges, table = R.edges(labels), R.table(labels)
    rings = F.link_rings(edges)
    assert len(rings) == 2 and all(len(r) == 1 for r in rings.values())
    areas = {int(row[1]): int(row[2]) for row in table}
    for (_, label), (ring,) in rings.items():
        assert F.polygon_is_valid([ring]) and F.signed_area(ring) == areas[label]
    warn = io.StringIO()
    features = F.featurize(edges, table, [Tile(69623, 104945, 18)], (64, 64), 0, warn=warn)
    assert len(features) == 2 and warn.getvalue() == ""
    assert sorted(f["properties"]["area_px"] for f in features) == [21 * 21 + 3 * 4, 21 * 21 + 3 * 5]
    assert sum(f["properties"]["area_px"] for f in features) == mask.sum()
    assert all(f["geometry"]["type"] == "Polygon" and len(f["geometry"]["coordinates"]) == 1 for f in features)
    # the two outlines share the cut: its three unit edges are walked once by either polygon, in opposite directions
    left, right = (np.asarray(r[0]) for _, r in sorted(rings.items()))
    shared = {tuple(v) for v in left.tolist()} & {tuple(v) for v in right.tolist()}
    assert shared == {(30, 17), (30, 18), (30, 19), (30, 20)}


def test_the_stitched_restatement_is_the_one_raster_whatever_the_tiling():
    import stitch_ref as S

    image = np.zeros((64, 64), dtype=np.uint8)
    image[:64, :64] = P.dumbbell()
    whole = P.split(image, 4)
    grid = S.Grid(S.split(image, 32, 32), 0)  # the neck crosses the seam at column 32
    tiles = P.split_stitched(grid, 4)
    pasted = grid.paste(tiles)
    pairs = {(int(a), int(b)) for a, b in zip(whole[image != 0], pasted[image != 0])}
    assert len(pairs) == 2 and len({a for a, _ in pairs}) == 2 and len({b for _, b in pairs}) == 2, "the same partition, other names"
    assert ((pasted != 0) == (image != 0)).all()


# ---- boundary ------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_and_bound_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    for name, args in (("rs_features_split_cores", 5), ("rs_features_split_seeds", 7), ("rs_features_grow_workspace_bytes", 3),
                       ("rs_features_grow_config", 3), ("rs_features_grow", 9)):
        assert re.search(r"^(int|long) " + name + r"\(", header, flags=re.M), name
        assert len(_lib.SIGNATURES[name][1]) == args, name
    assert "in the fixed order N (y - 1),\n *          W (x - 1), E (x + 1), S (y + 1)" in header
    assert _lib.ABI_VERSION == 24


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def small_tiles(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("split_cli")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "building"]\ncolors = ["denim", "orange"]\n')
    for x in (69623, 69624):
        os.makedirs(str(tmp / "masks" / "18" / str(x)), exist_ok=True)
        png.write_png(str(tmp / "masks" / "18" / str(x) / "104945.png"), np.ones((24, 20), np.uint8), "P", make_palette("denim", "orange"))
    return [str(tmp / "masks"), "--type", "building", "--dataset", str(dataset), str(tmp / "out.geojson")]


@pytest.mark.parametrize("extra,message", [
    (["--split", "4", "--geometry", "centerline"],
     "Error: --split separates areas, which says nothing about lines: not with --geometry centerline"),
    (["--split", "65"], "Error: --split must be in 1..64 (0 = off)"),
    (["--split", "-1"], "Error: --split must be in 1..64 (0 = off)"),
    (["--split", "65", "--stitch"], "Error: --split must be in 1..64 (0 = off)"),
    (["--split", "21", "--stitch"],
     "Error: --split 21 needs a border of 21 pixels from the neighbouring tiles; tiles of 24x20 take at most 20"),
], ids=["centerline", "split_65", "split_negative", "split_65_stitch", "stitch_21"])
def test_the_error_exits_come_before_any_device_is_asked_for(small_tiles, extra, message):
    done = _rs(["features"] + small_tiles + extra)
    assert done.returncode != 0 and done.stderr.strip().splitlines()[-1] == message, done.stderr[-2000:]
    assert not os.path.exists(small_tiles[-1])


def test_the_help_says_what_simplification_does_to_a_shared_border(small_tiles):
    done = _rs(["features", "--help"])
    text = " ".join(done.stdout.split())
    assert done.returncode == 0 and "--split R" in text
    assert "their shared border may overlap or gap by up to the epsilon" in text
