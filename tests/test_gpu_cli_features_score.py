"""``./rs features --score`` end to end on the MI355X: a 2 x 2 block of 64 x 64 mask tiles and probability directories as
``rs predict`` writes them -> GeoJSON, every polygon's ``score`` against the probability ``rs masks`` votes with
(``np.average(linspace(0, 1, 256)[q], axis=0, weights=w)``) averaged over that polygon's pixels.  Cleaning is the identity here
(``--denoise 0 --grow 0``).  The bound of 1e-9 is derived: the device's sums are exact integers, the host divides once, and numpy's
float64 mean over at most 2^14 pixels errs by under 2^14 * 2^-53, about 2e-12."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import features_ref as R  # noqa: E402
import score_ref as C  # noqa: E402
import stitch_ref as S  # noqa: E402

from robosat_amd import png  # noqa: E402
from robosat_amd.colors import make_palette  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, X0, Y0, SIZE = 18, 69623, 104945, 64
WEIGHTS = [2.0, 1.0]
BOUND = 1e-9


def _rs(args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _write(root, tiles, mode, palette=None):
    for (x, y), image in tiles.items():
        os.makedirs(os.path.join(root, str(Z), str(x)), exist_ok=True)
        png.write_png(os.path.join(root, str(Z), str(x), str(y) + ".png"), image, mode, palette)


def _mask():
    """128 x 128, objects of different areas: one across the seam at x = 64, one across the seam at y = 64, three inside a tile."""

    mask = np.zeros((2 * SIZE, 2 * SIZE), dtype=bool)
    mask[10:20, 40:90] = True  # 500 pixels: 240 left of the seam, 260 right of it
    mask[50:81, 8:20] = True  # 372 pixels: 168 above the seam, 204 below it
    mask[30:37, 4:33] = True  # 203, in the top left tile
    mask[100:111, 80:101] = True  # 231, in the bottom right tile
    mask[40:45, 100:109] = True  # 45, in the top right tile
    return mask


def _probabilities():
    """Two models' bytes over the raster: noise around a level that differs from object to object, so no two polygons score alike."""

    rng = np.random.RandomState(3)
    yy, xx = np.mgrid[:2 * SIZE, :2 * SIZE]
    a = np.clip(140 + 60 * np.sin(xx / 17.0) + 40 * np.cos(yy / 11.0) + rng.randint(-20, 21, size=xx.shape), 0, 255).astype(np.uint8)
    b = rng.randint(0, 256, size=xx.shape).astype(np.uint8)
    return np.stack([a, b])


def _expected(labels, q, weights):
    """[(area, score)] of a label raster's components, sorted."""

    vote = C.vote(q, weights)
    return sorted((int((labels == name).sum()), float(vote[labels == name].mean())) for name in np.unique(labels[labels != 0]).tolist())


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("features_score")
    dataset = tmp / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "building"]\ncolors = ["denim", "orange"]\n')
    four = tmp / "four.toml"
    four.write_text('[common]\nclasses = ["background", "water", "road", "building"]\ncolors = ["denim", "orange", "green", "purple"]\n')
    mask, q = _mask(), _probabilities()
    _write(str(tmp / "masks"), S.split(mask.astype(np.uint8), SIZE, SIZE, x0=X0, y0=Y0), "P", make_palette("denim", "orange"))
    _write(str(tmp / "masks4"), S.split(mask.astype(np.uint8) * 3, SIZE, SIZE, x0=X0, y0=Y0), "P",
           make_palette("denim", "orange", "green", "purple"))
    grey = [v for i in range(256) for v in (i, i, i)]
    _write(str(tmp / "a"), S.split(q[0], SIZE, SIZE, x0=X0, y0=Y0), "P", grey)
    _write(str(tmp / "b"), S.split(q[1], SIZE, SIZE, x0=X0, y0=Y0), "P", grey)
    rgb = np.stack([255 - q[0], q[1] // 2, q[0]], axis=2)  # (the class's channel is the third; the other two hold other bytes)
    _write(str(tmp / "rgb"), S.split(rgb, SIZE, SIZE, x0=X0, y0=Y0), "RGB")
    corners = [(r, c) for r in (0, SIZE) for c in (0, SIZE)]
    per_tile = sorted(pair for r, c in corners
                      for pair in _expected(R.label(mask[r:r + SIZE, c:c + SIZE]), q[:, r:r + SIZE, c:c + SIZE], WEIGHTS))
    return {"tmp": tmp, "dataset": str(dataset), "four": str(four), "masks": str(tmp / "masks"), "masks4": str(tmp / "masks4"),
            "a": str(tmp / "a"), "b": str(tmp / "b"), "rgb": str(tmp / "rgb"), "mask": mask, "q": q, "per_tile": per_tile,
            "whole": _expected(R.label(mask), q, WEIGHTS)}


def _run(s, name, extra, masks="masks", dataset="dataset"):
    out = str(s["tmp"] / name)
    done = _rs(["features", s[masks], "--type", "building", "--dataset", s[dataset], out, "--denoise", "0", "--grow", "0", "--simplify", "0"]
               + extra)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(out, "rb") as fp:
        raw = fp.read()
    return json.loads(raw), done.stderr, raw


def _close(doc, want):
    got = sorted((f["properties"]["area_px"], f["properties"]["score"]) for f in doc["features"])
    print("scores", [(a, s, t, abs(s - t)) for (a, s), (_, t) in zip(got, want)])
    assert [a for a, _ in got] == [a for a, _ in want]
    assert all(abs(s - t) <= BOUND for (_, s), (_, t) in zip(got, want)), [(s, t) for (_, s), (_, t) in zip(got, want)]


TWO = ["--score", "{a}", "--score", "{b}", "--score_weights", "2", "1"]


def _two(s):
    return [e.format(a=s["a"], b=s["b"]) for e in TWO]


def test_the_expectations_show_something(setup):
    assert [a for a, _ in setup["per_tile"]] == [45, 168, 203, 204, 231, 240, 260]
    assert [a for a, _ in setup["whole"]] == [45, 203, 231, 372, 500]
    for name in ("per_tile", "whole"):
        scores = [s for _, s in setup[name]]
        assert min(abs(s - t) for i, s in enumerate(scores) for t in scores[:i]) > 1e-4, "two polygons score alike"
        assert all(0 < s < 1 for s in scores)


def test_every_polygon_carries_the_weighted_mean_probability_of_its_pixels(setup):
    doc, stderr, _ = _run(setup, "per_tile.geojson", _two(setup))
    assert all(set(f["properties"]) == {"tile", "area_px", "score"} for f in doc["features"])
    _close(doc, setup["per_tile"])
    assert "7 components scored, 0 dropped" in stderr


def test_stitched_the_object_across_the_seam_is_one_feature_with_the_score_of_the_whole(setup):
    doc, stderr, _ = _run(setup, "stitched.geojson", ["--stitch"] + _two(setup))
    assert all(set(f["properties"]) == {"tile", "area_px", "stitched", "score"} for f in doc["features"])
    _close(doc, setup["whole"])
    whole, pieces = dict(setup["whole"]), dict(setup["per_tile"])
    assert abs(whole[500] - (240 * pieces[240] + 260 * pieces[260]) / 500) < 1e-12 and abs(pieces[240] - pieces[260]) > 1e-4
    assert "5 components scored, 0 dropped" in stderr


def test_min_score_between_two_scores_drops_exactly_the_lower_one(setup):
    ranked = sorted(setup["per_tile"], key=lambda pair: pair[1])
    bound = (ranked[0][1] + ranked[1][1]) / 2
    doc, stderr, _ = _run(setup, "min_score.geojson", _two(setup) + ["--min_score", repr(bound)])
    _close(doc, sorted(ranked[1:]))
    assert "7 components scored, 1 dropped" in stderr


def test_an_rgb_directory_of_four_classes_reads_the_channel_of_the_third(setup):
    doc, _, _ = _run(setup, "rgb.geojson", ["--score", setup["rgb"]], masks="masks4", dataset="four")
    mask, q = setup["mask"], setup["q"]
    want = sorted(pair for r in (0, SIZE) for c in (0, SIZE)
                  for pair in _expected(R.label(mask[r:r + SIZE, c:c + SIZE]), q[:1, r:r + SIZE, c:c + SIZE], None))
    _close(doc, want)


def _parent_path(s, stitch):
    """The file as the tool wrote it before the flag existed: the stages of its loop without the scoring stage, run in this process."""

    import torch
    from PIL import Image

    from robosat_amd import ops
    from robosat_amd.features import FeatureWriter, featurize, featurize_stitched, group_clusters, pack_clusters, stitch_tables
    from robosat_amd.tiles import tiles_from_slippy_map

    items = sorted(tiles_from_slippy_map(s["masks"]), key=lambda t: (t[0].z, t[0].x, t[0].y))
    paths = dict(items)
    writer = FeatureWriter()

    def load(tiles):
        return torch.from_numpy(np.stack([np.array(Image.open(paths[t]).convert("P"), dtype=np.uint8) for t in tiles])).to("cuda:0")

    if stitch:
        for tiles in pack_clusters(group_clusters(paths), SIZE * SIZE, side=SIZE):
            nbr, origin, _ = stitch_tables(tiles, (SIZE, SIZE))
            table, rows = ops.stitched_features(load(tiles), torch.from_numpy(nbr).to("cuda:0"), torch.from_numpy(origin).to("cuda:0"), 1, 0, 0, 0)
            writer.add(featurize_stitched(rows.cpu().numpy(), table.cpu().numpy(), tiles, (SIZE, SIZE), 0.0))
    else:
        tiles = [tile for tile, _ in items]
        labels = ops.label_components(ops.clean_masks(load(tiles), 1, 0, 0))
        table = ops.component_table(labels, 0)
        writer.add(featurize(ops.boundary_edges(labels, table).cpu().numpy(), table.cpu().numpy(), tiles, (SIZE, SIZE), 0.0))
    out = str(s["tmp"] / ("parent_stitched.geojson" if stitch else "parent.geojson"))
    writer.save(out)
    with open(out, "rb") as fp:
        return fp.read()


@pytest.mark.parametrize("stitch", [False, True], ids=["per_tile", "stitched"])
def test_without_the_flag_the_file_is_byte_for_byte_what_the_unchanged_stages_write(setup, stitch):
    flags = ["--stitch"] if stitch else []
    doc, stderr, raw = _run(setup, "plain.geojson", flags)
    assert "score" not in stderr.lower() and not any("score" in f["properties"] for f in doc["features"])
    assert raw == _parent_path(setup, stitch)
    # and the flag adds the property and nothing else
    scored, _, _ = _run(setup, "scored.geojson", flags + _two(setup))
    for feature in scored["features"]:
        del feature["properties"]["score"]
    assert scored == doc


def test_a_missing_tile_another_size_and_too_few_channels_name_the_tile_and_the_path(setup):
    out = str(setup["tmp"] / "bad.geojson")
    base = ["features", setup["masks"], "--type", "building", "--dataset", setup["dataset"], out, "--denoise", "0", "--grow", "0"]
    q = setup["q"]
    tiles = S.split(q[0], SIZE, SIZE, x0=X0, y0=Y0)
    grey = [v for i in range(256) for v in (i, i, i)]
    name = "{}/{}/{}".format(Z, X0 + 1, Y0)

    def refused(extra, *words):
        done = _rs(base + extra)
        assert done.returncode != 0 and "Error" in done.stderr and "Traceback" not in done.stderr and not os.path.exists(out), done.stderr
        for word in words:
            assert word in done.stderr, (word, done.stderr)

    missing = str(setup["tmp"] / "missing")
    _write(missing, {k: v for k, v in tiles.items() if k != (X0 + 1, Y0)}, "P", grey)
    refused(["--score", missing], name, missing)
    small = str(setup["tmp"] / "small")
    other = dict(tiles)
    other[(X0 + 1, Y0)] = np.zeros((32, 64), dtype=np.uint8)
    _write(small, other, "P", grey)
    refused(["--score", small], name, os.path.join(small, str(Z), str(X0 + 1), str(Y0) + ".png"))
    refused(["--score", setup["a"], "--score", setup["rgb"]], "{}/{}/{}".format(Z, X0, Y0), os.path.join(setup["rgb"], str(Z), str(X0)))
    base[base.index("--dataset") + 1] = setup["four"]  # class 3 of 4 from a binary model's tiles
    base[1] = setup["masks4"]
    refused(["--score", setup["a"]], "{}/{}/{}".format(Z, X0, Y0), os.path.join(setup["a"], str(Z), str(X0), str(Y0) + ".png"))
