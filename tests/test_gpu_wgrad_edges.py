"""The weight-gradient kernels other than the stem's, exactly at their chunk and split edges: conv_wgrad_bf16<...> (seven tiles, RING 2
and 3, the PHASE form), conv_wgrad_phase4_bf16, combine_phase_wgrad_kernel, conv_wgrad_thin_bf16<1|2|4, ups 0|1>, conv_wgrad_f32_dma,
the register-staged conv_wgrad_f32 (plain, phase and direct forms), conv_wgrad_wino_f32, conv_wgrad_wino33_f32 and reduce.hip's one-
and two-level sums.

A weight gradient is a reduction over M = N Ho Wo pixels: its largest element grows like sqrt(M) while one pixel contributes O(1), so a
bound relative to the largest element lets a dropped, doubled or misplaced pixel through.  Here, as in tests/test_gpu_stem.py:

  exact   integer operands in [-2, 2]: every product and partial sum is an integer (a dyadic number in the Winograd domain) that fp32
          holds exactly, so torch.equal against float64 autograd holds in any summation order (preconditions and their derivation per
          kernel: tests/wgrad_ref.py, asserted there per case by tests/test_wgrad_ref_cpu.py and again here before each launch).
  pulse   dy = one 1 per output channel, each at its own pixel: row co of the result IS the window of x under that pixel, bit for bit.
          The pixels are the image corners, the ends of the first, a middle and the last chunk, both sides of every split boundary of
          the restated plan and the last pixel of all: a failure names the pixel and the tap.
  float   Gaussian data, per element |err| <= 1e-5 * S with S = sum |dy| |x| in float64 (the bound of tests/test_gpu_stem.py); bf16
          operands are rounded on the host.  Not for the Winograd-domain kernels: S does not bound a transform's cancellation.
  twice   every launch of the exact tests is repeated and must give the same bits: splits are summed in fixed order, no atomics.

Every launch asserts the kernel that ran (ops.PROFILE's record: for bf16 the library's tile and form, ops.wgrad_kernel_name).  What
each shape aims at -- tiles, chunks, splits, reduction levels -- is written next to it in tests/wgrad_ref.py and held against the
library's plans by tests/test_wgrad_ref_cpu.py, which needs no GPU."""

import contextlib
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wgrad_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def _nhwc(t, dtype):
    return None if t is None else t.float().permute(0, 2, 3, 1).contiguous().to(DEV).to(dtype)


def _launch(case, dtype, knobs, a, b, dy, name, twice=True):
    """a, b, dy NCHW float64 on the host -> the KRSC fp32 gradient on the device, under ``knobs``; asserts that kernel ``name`` ran and,
    with ``twice``, that a second launch gives the same bits."""
    from robosat_amd import ops

    act = BF if dtype == "bf16" else torch.float32
    args = (_nhwc(dy, act), _nhwc(a, act), case.k, case.k)
    kw = dict(src2=_nhwc(b, act), ups=case.ups, stride=case.stride, pad=case.pad)
    with contextlib.ExitStack() as stack:
        for k, v in knobs.items():
            stack.enter_context(ops.knob(k, v))
        ops.PROFILE = []
        try:
            dw = ops.conv2d_wgrad(*args, **kw)
            ran = [r[0] for r in ops.PROFILE]
        finally:
            ops.PROFILE = None
        assert ran == [name], (ran, name)
        assert dw.dtype == torch.float32 and tuple(dw.shape) == (case.cout, case.k, case.k, case.cin)
        if twice:
            assert torch.equal(dw, ops.conv2d_wgrad(*args, **kw)), "a second launch gave other bits"
    return dw


def _same_bits(dw, ref):
    """torch.equal(dw, ref.float()), and where not: the worst element."""
    got = dw.cpu()
    if torch.equal(got, ref.float()):
        return True, None
    err = (got.double() - ref).abs()
    at = tuple(int(i) for i in torch.nonzero(err == err.max())[0])
    return False, dict(wrong=int((err > 0).sum()), of=err.numel(), worst=float(err.max()), at_co_ky_kx_ci=at, got=float(got[at]), want=float(ref[at]))


def _exact(case, dtype, label, knobs):
    a, b, dy, ref, mag = W.exact_problem(case)
    pl = W.plan(case, dtype, knobs)
    assert float(mag.max()) < W.EXACT, "precondition: sum |dy| |x| < 2^24"
    if pl["kind"] in ("w33", "ww"):
        assert W.wino_bound(case, float(dy.abs().max()), float(a.abs().max())) < W.EXACT, "precondition: 256 D X T < 2^24"
    dw = _launch(case, dtype, knobs, a, b, dy, pl["name"])
    ok, why = _same_bits(dw, ref)
    assert ok, (case.name, dtype, label, why)
    return pl


# ---------------------------------------------------------------------------------------------------------------------------------
# 1 + 2 + 6: exact, tap-per-block and DecoderBlock forms, bf16 and fp32 from one case table
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", W.all_launches(), ids=W.launch_id)
def test_wgrad_exact(launch):
    """Integer operands: the kernel's bits are float64 autograd's, twice.  bf16: RING 3 (shipped) and wgrad_ring = 2; the phase form with
    conv_wgrad_phase4_bf16 and with wgrad_phase4 = 0.  fp32: the Winograd-domain form where the layer has one (shipped), the LDS-DMA
    kernel, the register-staged kernel (wgrad_f32_dma = 0) and, for DecoderBlock, the direct form (wgrad_f32_phase = 0)."""
    from robosat_amd import _lib

    case, dtype, label, knobs = launch
    assert W.plan(case, dtype, knobs)["name"] == W.expected_name(case, dtype, label)
    pl = _exact(case, dtype, label, knobs)
    if case.name.startswith("two_level"):  # reduce.hip's two levels with a short last split
        aim = dict(W.TAP_CASES)[case]["L"]
        key = "w33" if label == "wino33" else dtype
        assert pl["splits"] > 8 and pl["reduce"] == dict(levels=2, L=aim[key], scratch=32 * pl["n"]), pl
        assert pl["chunks"] % pl["cps"] or label == "wino33"
        # the library's own split count, from its workspace (bf16: splits partial tiles + 32 tiles of scratch)
        if dtype == "bf16":
            d = _lib.ConvDesc(*case.desc())
            assert _lib.lib().rs_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d)) == (pl["splits"] + 32) * pl["n"] * 4


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: combine_phase_wgrad_kernel (and its fp32 twin, and the Winograd finish kernel's same rule) with per-tap distinct data
# ---------------------------------------------------------------------------------------------------------------------------------
def _combine_problem(case):
    """One image, 3 x 3 source grid, the source a pulse at its centre (1, 1).  The sixteen (parity, offset) reductions
    G[(py, px), (r, s)] then each pick ONE dz pixel -- (4 - py - 2 r, 4 - px - 2 s): the inner 4 x 4 of the 6 x 6 output, each pixel once --
    so with dz = 2^(4 (y - 1) + (x - 1)) there every G plane is its own bit, and each of the nine filter taps, a sum of four planes, its
    own 4-bit mask: a swapped (py, px, r, s) index in the combine changes the result.  The outer ring of dz meets only zeros."""
    assert (case.n, case.h, case.w, case.c2) == (1, 3, 3, 0)
    a = torch.zeros(1, case.c1, 3, 3, dtype=torch.float64)
    a[0, :, 1, 1] = 1.0
    dy = W.ints(-2, 2, 1, case.cout, 6, 6, seed=77)
    for y in range(1, 5):
        for x in range(1, 5):
            dy[0, :, y, x] = float(1 << (4 * (y - 1) + (x - 1)))
    return a, dy


@pytest.mark.parametrize("dtype,label,knobs", [("bf16", "shipped", {}), ("bf16", "phase", {"wgrad_phase4": 0}), ("f32", "wino", {}),
                                               ("f32", "phase", {"wgrad_f32_wino": 0}), ("f32", "staged", {"wgrad_f32_dma": 0})])
@pytest.mark.parametrize("case", W.COMBINE_CASES, ids=lambda c: c.name)
def test_phase_combine_taps(case, dtype, label, knobs):
    """Every intermediate is a signed sum of the sixteen powers of two in which each appears at most 16 times (once per plane, four
    planes per Winograd g, four g per tap): below 16 * 2^16 = 2^20, exact in fp32 in every form."""
    a, dy = _combine_problem(case)
    ref = W.wgrad(case, a, None, dy)
    assert 16 * float(dy[0, 0].abs().sum()) < W.EXACT and float(W.magnitude(case, a, None, dy).max()) < W.EXACT
    masks = [int(v) for v in ref[0, :, :, 0].flatten()]
    assert len(set(masks)) == 9 and all(bin(m).count("1") == 4 for m in masks), masks
    got_or = 0
    for m in masks:
        got_or |= m
    assert got_or == 0xFFFF, "every G plane reaches a tap"
    dw = _launch(case, dtype, knobs, a, None, dy, W.plan(case, dtype, knobs)["name"])
    ok, why = _same_bits(dw, ref)
    assert ok, (case.name, dtype, label, why, "taps as bit masks", [hex(int(v)) for v in dw[0, :, :, 0].flatten().cpu()], [hex(m) for m in masks])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3 + 6: exact, the thin bf16 kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,aim", W.THIN_CASES, ids=[c.name for c, _ in W.THIN_CASES])
def test_wgrad_thin_exact(case, aim):
    """conv_wgrad_thin_bf16<1|2|4, ups 0|1>: one 8 x 8 patch (every halo side padding), runs of patches that cross an output row and
    an image inside a block with a ragged last block, and the groups > 1 path at the smallest size its plan admits (the one large
    case; that nothing smaller is admitted: tests/test_wgrad_ref_cpu.py).  The slices handed to reduce.hip are the plan's."""
    from robosat_amd import _lib

    pl = W.bf16_plan(case)
    assert pl["kind"] == "thin" and (pl["patches"], pl["cps"], pl["splits"], pl["last"], pl["slices"]) == aim
    d = _lib.ConvDesc(*case.desc())
    assert _lib.lib().rs_conv2d_wgrad_bf16_workspace_bytes(ctypes.byref(d)) == (pl["slices"] + (32 if pl["slices"] > 8 else 0)) * pl["n"] * 4
    assert pl["reduce"]["levels"] == (2 if pl["slices"] > 8 else 1)
    _exact(case, "bf16", "thin", {})


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: pulse probes
# ---------------------------------------------------------------------------------------------------------------------------------
def _pulse_launches():
    out = []
    for case in W.PULSE_CASES:
        for dtype in ("bf16", "f32"):
            out += [(case, dtype, label, knobs) for label, knobs in W.variants(case, dtype)]
    return out + [(case, "bf16", "thin", {}) for case in W.THIN_PULSE_CASES]


@pytest.mark.parametrize("launch", _pulse_launches(), ids=W.launch_id)
def test_wgrad_pulses(launch):
    """Channel co of dy is zero but for a 1 at its own pixel; x holds integers.  Row co of the gradient must be the k x k x Cin window
    of the gathered input under that pixel, zeros outside the image; channels without a pulse must give zero rows."""
    case, dtype, label, knobs = launch
    pl = W.plan(case, dtype, knobs)
    a, b, _ = W.operands(case, "int", seed=2000)
    positions = W.pulse_positions(case, pl)
    for s in range(1, pl["splits"]):  # both sides of every split boundary are among them
        for pos in W.chunk_ends(case, pl, s * pl["cps"] - 1)[1] + W.chunk_ends(case, pl, s * pl["cps"])[0]:
            assert pos in positions
    for start in range(0, len(positions), case.cout):
        batch = positions[start:start + case.cout]
        dy = torch.zeros(case.n, case.cout, case.ho, case.wo, dtype=torch.float64)
        for co, (n, oy, ox) in enumerate(batch):
            dy[n, co, oy, ox] = 1.0
        dw = _launch(case, dtype, knobs, a, b, dy, pl["name"], twice=False).cpu().double()
        for co, pos in enumerate(batch):
            want = W.pulse_window(case, a, b, pos)
            if not torch.equal(dw[co], want):
                bad = torch.nonzero(dw[co] != want)
                raise AssertionError("{} {} {}: pulse at (n, oy, ox) = {} (channel {}): {} wrong elements, first at (ky, kx, ci) = {}: got {}, want {}".format(
                    case.name, dtype, label, pos, co, len(bad), tuple(int(i) for i in bad[0]), float(dw[co][tuple(bad[0])]), float(want[tuple(bad[0])])))
        if len(batch) < case.cout:
            assert float(dw[len(batch):].abs().max()) == 0.0, "a channel without a pulse must give a zero row"


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: Gaussian data against float64, the tap-per-block, phase and thin kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _gauss_launches():
    out = []
    for case in W.GAUSS_CASES:
        thin = W.bf16_plan(case)["form"] == 1
        for dtype in ("bf16",) if thin else ("bf16", "f32"):
            out += [(case, dtype, label, knobs) for label, knobs in W.variants(case, dtype) if label not in ("wino", "wino33")]
    return out


@pytest.mark.parametrize("launch", _gauss_launches(), ids=W.launch_id)
def test_wgrad_float64(launch):
    """|got - ref| <= 1e-5 * S per element, S = sum |dy| |x| in float64 (the same autograd on absolute values)."""
    case, dtype, label, knobs = launch
    a, b, dy = W.operands(case, "randn_bf16" if dtype == "bf16" else "randn", seed=3000)
    ref, s = W.wgrad(case, a, b, dy), W.magnitude(case, a, b, dy)
    dw = _launch(case, dtype, knobs, a, b, dy, W.plan(case, dtype, knobs)["name"], twice=False).cpu().double()
    ratio = float(((dw - ref).abs() / s.clamp_min(1e-300)).max())
    print("{} {} {}: max |err| / S = {:.3e}".format(case.name, dtype, label, ratio))
    assert float(((dw - ref).abs() - 1e-5 * s).max()) <= 0.0, (case.name, dtype, label, ratio)
