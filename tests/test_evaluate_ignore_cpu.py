"""``rs evaluate --type --ignored unknown`` without a GPU: the numpy restatement (tests/eval_ignore_ref.py) against the brute-force
transform, the properties that say what "unknown" means (a strip of ignored columns is a narrower raster, a wholly ignored tile is
an absent tile), the identities the device path rests on, the flag's validation before any device is asked for, the report's key,
and the declaration and binding of the two entry points.  Integers throughout: every comparison is equality."""

import argparse
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import centerline_eval_ref as C  # noqa: E402
import edt_ref as E  # noqa: E402
import eval_ignore_ref as N  # noqa: E402
import features_ref as R  # noqa: E402
import stitch_ref as S  # noqa: E402
import thin_ref as T  # noqa: E402

from robosat_amd import evaluate as H  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = 255


def _random_pair(rng, shape, share):
    """(p, a): random bytes of three classes, ``share`` of the label pixels ignored."""

    p = rng.randint(0, 3, size=shape).astype(np.uint8)
    a = rng.randint(0, 3, size=shape).astype(np.uint8)
    a[rng.rand(*shape) < share] = IGNORE
    return p, a


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_coded_is_the_definition():
    p = np.array([[1, 1, 0, 2, 1, 255]], dtype=np.uint8)
    a = np.array([[1, 0, 255, 255, 2, 1]], dtype=np.uint8)
    cp, cg = N.coded(p, a, 1, IGNORE)
    assert cp.tolist() == [[1, 1, 2, 2, 1, 0]]  # (a mask byte of 255 is no class and not set; refusing it is the confusion count's part)
    assert cg.tolist() == [[1, 0, 2, 2, 0, 1]]
    cp, cg = N.coded(p, a, 2, IGNORE)
    assert cp.tolist() == [[0, 0, 2, 2, 0, 0]] and cg.tolist() == [[0, 0, 2, 2, 1, 0]]  # the prediction under U is no part of P


@pytest.mark.parametrize("share", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("seed, shape", [(0, (20, 20)), (1, (13, 20)), (2, (20, 7)), (3, (1, 17)), (4, (9, 1))])
def test_the_coded_band_is_the_brute_force_definition(seed, shape, share):
    rng = np.random.RandomState(10 * seed + int(10 * share))
    p, a = _random_pair(rng, shape, share)
    blobs = R.blobs(shape[0], shape[1], seed, count=3)
    for t, (pp, aa) in ((1, (p, a)), (2, (np.where(blobs, 2, p).astype(np.uint8), np.where(np.roll(blobs, 1, axis=1) & (a != IGNORE), 2, a).astype(np.uint8)))):
        for c in N.coded(pp, aa, t, IGNORE):
            assert ((c == E.UNKNOWN) == (aa == IGNORE)).all()
            for d in (1, 3):
                d2 = E.edt_brute(c, d + 1, coded=True)
                want = (d2 >= 1) & (d2 <= d * d)
                got = N.band(c, d)
                assert (got == want).all()
                assert not got[c != E.SET].any()  # an unknown pixel is in no band
                # what the device computes: the transform that takes non-zero for set has the definition's value at every SET pixel
                assert (E.edt(c != 0, d + 1)[c == E.SET] == d2[c == E.SET]).all()


def test_the_edge_of_an_ignored_region_is_no_boundary():
    a = np.zeros((12, 12), dtype=np.uint8)
    a[:, :6] = 1
    a[4:8, :] = IGNORE  # a band of ignored rows through the object and the background
    cp, cg = N.coded(a, a, 1, IGNORE)
    band = N.band(cg, 1)
    assert band.sum() == 8 and band[:4, 5].all() and band[8:, 5].all()  # the column beside the background, known rows only
    assert not band[3, :5].any() and not band[8, :5].any()  # the rows beside U have no band of their own


# ---- a strip of ignored columns is a narrower raster ---------------------------------------------------------------------------
def _scene(h, w, seed):
    """(p, a) uint8 [h, w]: class 1 = five boxes and a road, the prediction the label moved by (1, 1) with a box more."""

    rng = np.random.RandomState(seed)
    g = np.zeros((h, w), dtype=bool)
    for _ in range(5):
        y, x = rng.randint(0, h - 4), rng.randint(0, w - 4)
        g[y:y + rng.randint(3, 8), x:x + rng.randint(3, 8)] = True
    g |= T.roads(h, w, seed, count=1, width=3)
    p = np.roll(g, (1, 1), axis=(0, 1))
    y, x = rng.randint(0, h - 4), rng.randint(0, w - 4)
    p[y:y + 4, x:x + 4] = True
    return p.astype(np.uint8), g.astype(np.uint8)


def _all_counts(cp, cg, d, rho):
    cp, cg = np.asarray(cp)[None], np.asarray(cg)[None]
    return N.band_counts(cp, cg, d).tolist(), N.objects(cp, cg, 0.5), N.objects(cp, cg, 0.25, min_area=4), N.centerline_counts(cp, cg, rho)


@pytest.mark.parametrize("k", [1, 5, 11])
@pytest.mark.parametrize("seed", [2, 3])
def test_an_ignored_strip_counts_what_the_raster_without_it_does(seed, k):
    p, a = _scene(24, 32, seed)
    a_cut = a.copy()
    a_cut[:, -k:] = IGNORE
    p_noise = p.copy()
    p_noise[::2, -k:] = 1  # whatever is predicted under the strip has no say
    full = _all_counts(*N.coded(p_noise, a_cut, 1, IGNORE), 3, 2)
    narrow = _all_counts(*N.coded(p[:, :-k], a[:, :-k], 1, IGNORE), 3, 2)
    assert full == narrow
    assert full[0][0][2] > 0 and full[1][0] > 0 and full[3][0][0] > 0  # (bands, matches and links: the case shows something)
    assert full != _all_counts(*N.coded(p_noise, a, 1, IGNORE), 3, 2)  # (with the strip known, what lies in it counts)


# ---- a wholly ignored tile is an absent tile -----------------------------------------------------------------------------------
def _grids(p, a, absent=(), ignored=()):
    tiles_p, tiles_a = S.split(p, 16, 16, absent=absent), S.split(a, 16, 16, absent=absent)
    coded_p, coded_g = {}, {}
    for key in tiles_p:
        label = np.full_like(tiles_a[key], IGNORE) if key in ignored else tiles_a[key]
        coded_p[key], coded_g[key] = N.coded(tiles_p[key], label, 1, IGNORE)
    return N.grid(coded_p), N.grid(coded_g)


def _all_counts_grid(gp, gg, d, rho):
    return N.band_counts_grid(gp, gg, d).tolist(), N.objects_grid(gp, gg, 0.5), N.centerline_counts_grid(gp, gg, rho)


@pytest.mark.parametrize("tile", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("d", [1, 3, 15])
def test_a_wholly_ignored_tile_counts_what_the_grid_without_it_does(tile, d):
    p, a = _scene(32, 32, 5)
    with_ignored = _all_counts_grid(*_grids(p, a, ignored={tile}), d, min(d, 15))
    without = _all_counts_grid(*_grids(p, a, absent={tile}), d, min(d, 15))
    assert with_ignored == without
    assert with_ignored != _all_counts_grid(*_grids(p, a), d, min(d, 15))
    assert with_ignored[0][2] > 0 and with_ignored[1][1] > 0 and with_ignored[2][0] > 0


# ---- the centre lines need no coded transform ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_the_reach_of_a_skeleton_outside_u_is_the_plain_reach_at_every_known_pixel(seed):
    rng = np.random.RandomState(seed)
    h, w = rng.randint(1, 21), rng.randint(1, 21)
    unknown = rng.rand(h, w) < (0.0, 0.1, 0.5)[seed % 3]
    skeleton = (rng.rand(h, w) < 0.08) & ~unknown
    for rho in (1, 3, 6):
        assert (C.near(skeleton, rho, known=~unknown) == (C.near(skeleton, rho) & ~unknown)).all()
        assert (C.near(skeleton, rho) == C.near_brute(skeleton, rho)).all()


# ---- the flag ------------------------------------------------------------------------------------------------------------------
def _parser():
    from robosat_amd.tools import evaluate as tool

    parser = argparse.ArgumentParser()
    tool.add_parser(parser.add_subparsers())
    return parser, tool


def _dirs(tmp_path, ignore):
    from robosat_amd import png
    from robosat_amd.colors import make_palette

    dataset = tmp_path / "dataset.toml"
    dataset.write_text('[common]\nclasses = ["background", "road"]\ncolors = ["denim", "orange"]\n' + ("ignore = 255\n" if ignore else ""))
    for name in ("masks", "labels"):
        os.makedirs(str(tmp_path / name / "18" / "5"))
        png.write_png(str(tmp_path / name / "18" / "5" / "7.png"), np.zeros((8, 6), dtype=np.uint8), "P", make_palette("denim", "orange"))
    return ["evaluate", str(tmp_path / "masks"), str(tmp_path / "labels"), "--dataset", str(dataset), str(tmp_path / "report.json")]


def test_the_flag_parses_and_defaults_to_refuse(tmp_path):
    parser, _ = _parser()
    base = _dirs(tmp_path, True)
    assert parser.parse_args(base).ignored == "refuse"
    assert parser.parse_args(base + ["--type", "road", "--ignored", "unknown"]).ignored == "unknown"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--ignored", "background"])
    help_text = " ".join(parser._subparsers._group_actions[0].choices["evaluate"].format_help().split())
    assert "--ignored {refuse,unknown}" in help_text and "on both sides alike" in help_text


@pytest.mark.parametrize("ignore, extra, words", [
    (True, ["--ignored", "unknown"], ["--ignored unknown", "--type"]),
    (True, ["--ignored", "unknown", "--probs", "nowhere"], ["--ignored unknown", "--type"]),
    (False, ["--type", "road", "--ignored", "unknown"], ["--ignored unknown", "[common] ignore"]),
    (False, ["--type", "road", "--boundary", "2", "--stitch", "--ignored", "unknown"], ["--ignored unknown", "[common] ignore"]),
])
def test_main_rejects_the_flag_before_it_needs_a_device(tmp_path, monkeypatch, ignore, extra, words):
    import torch

    parser, tool = _parser()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flag is checked before the device is"))
    with pytest.raises(SystemExit) as exc:
        tool.main(parser.parse_args(_dirs(tmp_path, ignore) + extra))
    assert isinstance(exc.value.code, str) and exc.value.code.startswith("Error: --ignored unknown")
    for word in words:
        assert word in exc.value.code, (word, exc.value.code)
    assert not os.path.exists(str(tmp_path / "report.json"))


@pytest.mark.parametrize("extra", [["--type", "road", "--ignored", "unknown"], ["--type", "road", "--ignored", "refuse"], ["--ignored", "refuse"]])
def test_with_a_good_flag_main_goes_on_to_ask_for_the_device(tmp_path, monkeypatch, extra):
    import torch

    parser, tool = _parser()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as exc:
        tool.main(parser.parse_args(_dirs(tmp_path, True) + extra))
    assert exc.value.code == "Error: this build computes on the MI355X only"


def test_a_namespace_without_the_attribute_is_refuse(tmp_path, monkeypatch):
    """Callers that build the arguments themselves predate the flag."""

    import torch

    parser, tool = _parser()
    args = parser.parse_args(_dirs(tmp_path, True) + ["--type", "road"])
    del args.ignored
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as exc:
        tool.main(args)
    assert exc.value.code == "Error: this build computes on the MI355X only" and args.ignored == "refuse"


# ---- the report ----------------------------------------------------------------------------------------------------------------
def test_the_report_gains_one_key_behind_ignored():
    matrix = [[5, 1], [2, 4]]
    plain = H.build_report(["background", "road"], matrix, 1, 0, kind="road", objects={}, ignore=255, ignored=7)
    flagged = H.build_report(["background", "road"], matrix, 1, 0, kind="road", objects={}, ignore=255, ignored=7, ignored_as="unknown")
    assert "ignored_as" not in plain and flagged["ignored_as"] == "unknown"
    keys = list(flagged)
    assert keys.index("ignored_as") == keys.index("ignored") + 1 == keys.index("ignore") + 2
    assert {k: v for k, v in flagged.items() if k != "ignored_as"} == plain and [k for k in keys if k != "ignored_as"] == list(plain)


# ---- the entry points ----------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_in_the_header_and_bound():
    from robosat_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    assert re.search(r"\bint rs_eval_select\(const uint8_t\* predicted, const uint8_t\* actual, uint8_t\* coded_p, uint8_t\* coded_g, "
                     r"uint8_t\* mask_p, uint8_t\* mask_g,\s+long pixels, int C, int cls, int ignore, rs_stream_t stream\);", header)
    assert re.search(r"\bint rs_eval_boundary_coded\(const int32_t\* d2_a, const int32_t\* d2_b, const uint8_t\* coded, int64_t\* counts, "
                     r"long pixels, long group, int D,\s+rs_stream_t stream\);", header)
    text = " ".join(header.replace(" * ", " ").split())
    assert "U = {a == I}" in text and "P = {p == t} \\ U" in text and "an unknown pixel is in no band" in text
    assert len(_lib.SIGNATURES["rs_eval_select"][1]) == 11 and len(_lib.SIGNATURES["rs_eval_boundary_coded"][1]) == 8
    assert len(_lib.SIGNATURES["rs_eval_boundary"][1]) == 7  # (the entry point without a coded plane is as it was)
    assert _lib.ABI_VERSION == 24  # (two new symbols, no old one changed)
    assert callable(ops.select_known)
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.lib(), "rs_eval_select") and hasattr(_lib.lib(), "rs_eval_boundary_coded")
