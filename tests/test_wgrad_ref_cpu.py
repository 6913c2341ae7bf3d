"""Pins tests/wgrad_ref.py without a GPU: every case of tests/test_gpu_wgrad_edges.py still aims at the chunk / split edge it was
chosen for.  Three parties are compared per case and knob setting -- the figures written next to the case (``aim``), the Python
restatement of the launch plans, and the library's own answers (rs_conv2d_wgrad_bf16_tile / _form, rs_conv2d_wgrad_form and the
split count inside the workspace sizes; the library loads without a GPU, no kernel is launched).  Also: the integer-range
precondition of every case, and the float64 reference against two independent restatements on tiny shapes."""

import contextlib
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wgrad_ref as W  # noqa: E402


def _lib():
    from robosat_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        pytest.skip("librobosat_hip.so not built (run __graft_entry__.build())")
    return L


@contextlib.contextmanager
def _knobs(settings):
    from robosat_amd import ops

    with contextlib.ExitStack() as stack:
        for name, value in settings.items():
            stack.enter_context(ops.knob(name, value))
        yield


def _desc(case):
    return _lib().ConvDesc(*case.desc())


def test_shipped_knobs_are_the_ones_the_restatements_start_from():
    from robosat_amd import ops

    _lib()
    assert {k: ops.get_knob(k) for k in W.DEFAULT_KNOBS} == W.DEFAULT_KNOBS


def test_case_names_are_unique_and_every_table_is_used():
    names = [c.name for c, _ in W.TAP_CASES + W.DEC_CASES + W.THIN_CASES] + [c.name for c in W.COMBINE_CASES + W.THIN_PULSE_CASES]
    assert len(names) == len(set(names))
    assert len(W.PULSE_CASES) == 5 and len(W.GAUSS_CASES) == 7


# ---------------------------------------------------------------------------------------------------------------------------------
# aim == restatement == library
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,aim", W.TAP_CASES + W.DEC_CASES, ids=[c.name for c, _ in W.TAP_CASES + W.DEC_CASES])
def test_aims_match_the_restated_plans_at_the_shipped_knobs(case, aim):
    b = W.bf16_plan(case)
    assert (b["tile_name"] if b["form"] == 0 else b["name"][len("conv_wgrad_bf16<"):-1], b["chunks"], b["cps"], b["splits"]) == aim["bf16"]
    # the tap-per-block / phase plan of conv_wgrad.hip, whatever Winograd form is shipped on top of it
    f = W.f32_plan(case, {"wgrad_f32_wino": 0, "wgrad_f32_wino33": 0})
    assert (f["tile_name"], f["chunks"], f["cps"], f["splits"]) == aim["f32"]
    shipped = W.f32_plan(case)
    for key, form in (("w33", 4), ("ww", 3)):
        if key in aim:
            assert shipped["form"] == form and (shipped["chunks"], shipped["cps"], shipped["splits"]) == aim[key]
        else:
            assert shipped["form"] != form
    # ragged tails and boundaries inside images, from the figures above
    if case.name.endswith("_two_chunks"):
        assert case.m == 126 and case.m - 64 == 62 and case.m - 3 * 32 == 30
    if case.name.endswith("_splits"):
        assert case.ho * case.wo == 323 and b["cps"] * 64 % 323 != 0 and all(s * f["cps"] * 32 % 323 for s in (1, 2))
        assert b["chunks"] - b["cps"] < b["cps"] and case.m % 64 and case.m % 32  # a short last split with a ragged last chunk
    if case.name.startswith("m"):
        assert case.m == int(case.name[1:])
    if case.name.startswith("two_level"):
        for key, pl in (("bf16", b), ("f32", f), ("w33", shipped)):
            if key in aim["L"]:
                assert pl["splits"] > 8 and pl["reduce"]["levels"] == 2 and pl["reduce"]["L"] == aim["L"][key]
        assert b["chunks"] - (b["splits"] - 1) * b["cps"] == 3 and f["chunks"] - (f["splits"] - 1) * f["cps"] == 6
        assert W.thin_plan(case) is None  # (W = 50 keeps the 3x3 off the all-taps kernel)
    if case.name.startswith("straddle"):
        assert case.h * case.w == 195 and b["cps"] * 64 % 195 and f["cps"] * 32 % 195
    if case.name == "grid_5x13":
        assert case.n * case.h * case.w == 65
    if case.name.startswith("tiles_"):
        assert W.wino_tiles(case) == int(case.name[6:])
    if case.name == "two_sources_128+64":
        assert b["launches"] == 2
    # fewer chunks than the ring has buffers, where the case says so
    if case.name in ("m63", "m64", "m65", "image_2x2", "image_1x3"):
        assert b["chunks"] < b["ring"] == 3


@pytest.mark.parametrize("launch", W.all_launches(), ids=W.launch_id)
def test_restated_plan_matches_the_library(launch):
    case, dtype, label, knobs = launch
    lib = _lib().lib()
    d = _desc(case)
    with _knobs(knobs):
        pl = W.plan(case, dtype, knobs)
        assert pl["name"] == W.expected_name(case, dtype, label), (pl["name"], label)
        if dtype == "bf16":
            from robosat_amd import ops

            assert lib.rs_conv2d_wgrad_bf16_form(ctypes.byref(d)) == pl["form"]
            assert lib.rs_conv2d_wgrad_bf16_tile(ctypes.byref(d)) == pl["tile"]
            assert ops.wgrad_kernel_name(d) == pl["name"]
            assert lib.rs_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d)) == pl["workspace"]
            assert pl["workspace"] == (pl["splits"] * pl["n"] + pl["reduce"]["scratch"] + (pl["n"] if pl["form"] == 2 else 0)) * 4
        else:
            assert lib.rs_conv2d_wgrad_form(ctypes.byref(d)) == pl["form"]
            assert lib.rs_conv2d_wgrad_workspace_bytes(ctypes.byref(d)) == pl["workspace"]
            if label in ("dma", "phase", "direct", "staged"):  # the split count of the launch itself, where the Winograd plan's workspace does not cover it
                own = (pl["splits"] * pl["n"] + pl["reduce"]["scratch"] + (pl["n"] if pl["form"] == 2 else 0)) * 4
                assert own <= pl["workspace"]
                with _knobs({"wgrad_f32_wino_blocks": 1, "wgrad_f32_wino33_blocks": 1}):  # (one Winograd split: the smaller workspace)
                    assert lib.rs_conv2d_wgrad_workspace_bytes(ctypes.byref(d)) == W.plan(
                        case, dtype, dict(knobs, wgrad_f32_wino_blocks=1, wgrad_f32_wino33_blocks=1))["workspace"]
    from robosat_amd import ops as _ops

    assert W.DEFAULT_KNOBS == {k: _ops.get_knob(k) for k in W.DEFAULT_KNOBS}  # (the knobs are back)


@pytest.mark.parametrize("case,aim", W.THIN_CASES, ids=[c.name for c, _ in W.THIN_CASES])
def test_thin_plan_matches_its_aim_and_the_library(case, aim):
    lib = _lib().lib()
    d = _desc(case)
    pl = W.bf16_plan(case)
    assert pl["form"] == 1 == lib.rs_conv2d_wgrad_bf16_form(ctypes.byref(d)) and lib.rs_conv2d_wgrad_bf16_tile(ctypes.byref(d)) == 0
    assert (pl["patches"], pl["cps"], pl["splits"], pl["last"], pl["slices"]) == aim
    assert lib.rs_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d)) == pl["workspace"] == (pl["slices"] * pl["n"] + pl["reduce"]["scratch"]) * 4
    if case.name.endswith("_runs"):
        ppr, ppi = case.wo // 8, (case.ho // 8) * (case.wo // 8)
        assert ppr % pl["cps"] and ppi % pl["cps"], "runs must cross output rows and images"
    if case.name.endswith("_groups"):
        assert pl["groups"] == 2
        small = W.THIN_TOO_SMALL
        assert small.n * (small.ho // 8) * (small.wo // 8) == pl["patches"] - 1
        ds = _desc(small)
        assert W.thin_plan(small) is None and lib.rs_conv2d_wgrad_bf16_form(ctypes.byref(ds)) == 0  # nothing smaller is admitted


@pytest.mark.parametrize("case", W.THIN_PULSE_CASES + W.COMBINE_CASES, ids=lambda c: c.name)
def test_probe_cases_take_the_kernels_they_are_meant_for(case):
    lib = _lib().lib()
    d = _desc(case)
    pl = W.bf16_plan(case)
    assert lib.rs_conv2d_wgrad_bf16_form(ctypes.byref(d)) == pl["form"] == (2 if case.name.startswith("combine") else 1)
    assert lib.rs_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d)) == pl["workspace"]
    if pl["form"] == 1:
        assert (pl["cps"], pl["splits"]) == (1, 12)
    else:
        assert pl["name"] == {"combine_64": "conv_wgrad_bf16<phase,64x64>", "combine_128": "conv_wgrad_bf16<phase4,128x128>"}[case.name]
        assert lib.rs_conv2d_wgrad_form(ctypes.byref(d)) == 3 == W.f32_plan(case)["form"]


def test_reduce_plan():
    assert W.reduce_plan(1024, 8) == dict(levels=1, L=1, scratch=0)
    assert W.reduce_plan(1024, 9) == dict(levels=2, L=4, scratch=32 * 1024)
    assert W.reduce_plan(1024, 100)["L"] == 32                # 131072 / 256 = 512 -> 32
    assert W.reduce_plan(4 * 131072, 100)["L"] == 2           # one lane's worth of columns -> the floor of 2
    assert W.reduce_plan(4 * 8192, 100)["L"] == 16


# ---------------------------------------------------------------------------------------------------------------------------------
# preconditions of the exact tests
# ---------------------------------------------------------------------------------------------------------------------------------
_EXACT_CASES = [c for c, _ in W.TAP_CASES + W.DEC_CASES + W.THIN_CASES] + W.COMBINE_CASES


@pytest.mark.parametrize("case", _EXACT_CASES, ids=lambda c: c.name)
def test_integer_operands_stay_exact_in_fp32(case):
    """S = sum |dy| |x| < 2^24 (a condition on the inputs), and 256 D X T < 2^24 where a Winograd-domain kernel runs the case."""
    if case.m > 20000:  # the three big thin cases: S <= 4 M by the operands' range alone, without a second backward pass
        assert 4 * case.m < W.EXACT
        return
    a, b, dy, ref, mag = W.exact_problem(case)
    assert float(a.abs().max()) <= 2 and float(dy.abs().max()) <= 2
    assert float(mag.max()) < W.EXACT and float(ref.abs().max()) <= float(mag.max())
    assert torch.equal(ref, ref.float().double())
    if W.f32_plan(case)["form"] in (3, 4):
        assert W.wino_bound(case, 2, 2) < W.EXACT


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference against its independent restatements
# ---------------------------------------------------------------------------------------------------------------------------------
_TINY = [W.plain("tiny_3x3", 2, 4, 5, 3, 2), W.plain("tiny_3x3_s2", 2, 5, 7, 3, 2, stride=2), W.plain("tiny_1x1_s2", 1, 5, 4, 2, 3, k=1, stride=2),
         W.plain("tiny_small_image", 2, 1, 2, 2, 2), W.plain("tiny_two_sources", 1, 3, 4, 2, 3, c2=3), W.decoder("tiny_decoder", 2, 3, 2, 2, 1, 3),
         W.decoder("tiny_decoder_1x1", 1, 1, 1, 2, 0, 2)]


@pytest.mark.parametrize("case", _TINY, ids=lambda c: c.name)
def test_reference_matches_the_loop_over_taps(case):
    a, b, dy = W.operands(case, "int", seed=7)
    ref = W.wgrad(case, a, b, dy)
    assert tuple(ref.shape) == (case.cout, case.k, case.k, case.cin)
    assert torch.equal(ref, W.wgrad_loops(case, a, b, dy))
    a, b, dy = W.operands(case, "randn", seed=8)
    ref, loops = W.wgrad(case, a, b, dy), W.wgrad_loops(case, a, b, dy)
    assert float((ref - loops).abs().max()) <= 1e-12 * float(W.magnitude(case, a, b, dy).max())


@pytest.mark.parametrize("case", _TINY, ids=lambda c: c.name)
def test_pulse_rows_are_windows_of_the_input(case):
    """dy = one 1 per output channel at its own pixel: row co of the reference is the window under that pixel."""
    a, b, _ = W.operands(case, "int", seed=9)
    positions = [(n, oy, ox) for n in range(case.n) for oy in range(case.ho) for ox in range(case.wo)][-case.cout:]
    dy = torch.zeros(case.n, case.cout, case.ho, case.wo, dtype=torch.float64)
    for co, (n, oy, ox) in enumerate(positions):
        dy[n, co, oy, ox] = 1.0
    ref = W.wgrad(case, a, b, dy)
    for co, pos in enumerate(positions):
        assert torch.equal(ref[co], W.pulse_window(case, a, b, pos)), (co, pos)


@pytest.mark.parametrize("case", W.PULSE_CASES + W.THIN_PULSE_CASES, ids=lambda c: c.name)
def test_pulse_positions_cover_the_split_boundaries(case):
    for dtype in ("bf16", "f32"):
        for label, knobs in W.variants(case, dtype):
            pl = W.plan(case, dtype, knobs)
            if dtype == "f32" and W.bf16_plan(case)["form"] == 1:
                continue  # (the thin cases run in bf16 only)
            pos = W.pulse_positions(case, pl)
            assert len(pos) == len(set(pos)) and (case.n - 1, case.ho - 1, case.wo - 1) in pos and (0, 0, 0) in pos
            per_unit = 4 if pl["kind"] in ("src", "ww") else 1
            # both sides of each boundary are there (clipped tiles at odd edges may coincide with other positions)
            assert len(pos) >= 6 + min(2, pl["splits"] - 1) * per_unit, (label, len(pos))
            if pl["kind"] == "pix":  # boundary pixels, spelled out
                for s in range(1, pl["splits"]):
                    m = s * pl["cps"] * pl["pk"]
                    for mm in (m - 1, m):
                        assert (mm // (case.ho * case.wo), mm % (case.ho * case.wo) // case.wo, mm % case.wo) in pos
