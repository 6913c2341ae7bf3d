"""Split K of the fp32 implicit-GEMM convolution (csrc/conv_igemm_dma_kernel.h, EPI_SPLITK + splitk_reduce_f32): a launch runs
as S slices of its K loop per output tile, the partial sums go through a workspace and a second kernel adds them in fixed order
and applies the epilogue.  Knob ``conv_splitk`` forces S so that small problems reach the kernels.

Parity is judged against fp64 ``F.conv2d`` on the CPU, RELATIVE to the unsplit launch on the same inputs: the re-associated sum
of S partials is the only new error source, so the split launch's max error must stay within 2x the unsplit launch's.  Both
errors are printed.

Shapes: the dispatcher takes channel counts that are multiples of 32 only (``valid()`` in conv_igemm_dma.hip), so the ragged-split
case runs 160 input channels (five 32-channel groups per tap, 20 over the phase form's four taps: S = 3 cuts 6 + 7 + 7) where a
first draft of this test asked for 144, which no launch of the kernel can run."""

import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
CENTER = dict(hs=8, ws=8, cin=2048, cout=256)  # UNet.center at 512 x 512: 2048 -> 256 on the 16x16 stage's 8x8 source


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def krsc(w):
    return w.permute(0, 2, 3, 1).contiguous().to(DEV)


# name -> (form, N, H, W, Cin, Cout, k, stride, pad, slices to run)
CASES = {
    "phase_ragged_k": ("phase", 3, 4, 4, 160, 64, 3, 1, 1, (1, 2, 3, 4)),  # 20 groups of 32 channels: S = 3 is ragged
    "phase_m_n_tails": ("phase", 2, 3, 5, 256, 96, 3, 1, 1, (3,)),         # 15-row images inside a 64-row tile, 96 couts = 1.5 N tiles
    "plain_1x1_residual": ("plain", 2, 8, 8, 256, 64, 1, 1, 0, (1, 3)),    # 8 groups: S = 3 is ragged
    "plain_3x3_stride2": ("plain", 2, 8, 8, 64, 64, 3, 2, 1, (4,)),        # 18 groups: S = 4 is ragged; 32 output rows: an M tail
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """Inputs, the fp64 CPU reference and the unsplit launch's output of a case (computed once, shared, never written to)."""
    from robosat_amd import ops

    form, n, h, w, cin, cout, k, stride, pad, _ = CASES[name]
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(cout, cin, k, k, seed=2) * (2.0 / (cin * k * k)) ** 0.5
    if form == "phase":  # DecoderBlock: upsample x2 nearest, 3x3 / pad 1, ReLU
        want = F.relu(F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), wt.double(), padding=1))
        xd, wp = nhwc(x), ops.pack_phase_weight(krsc(wt))
        run = lambda: ops.conv2d_phase(xd, wp, relu=True)
    else:  # scale, shift, residual, ReLU
        sc, sh = torch.rand(cout, generator=torch.Generator().manual_seed(3)) + 0.5, rnd(cout, seed=4)
        y = F.conv2d(x.double(), wt.double(), stride=stride, padding=pad)
        res = rnd(*y.shape, seed=5)
        want = F.relu(y * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1) + res.double())
        xd, wd, scd, shd, resd = nhwc(x), krsc(wt), sc.to(DEV), sh.to(DEV), nhwc(res)
        run = lambda: ops.conv2d(xd, wd, stride=stride, pad=pad, scale=scd, shift=shd, residual=resd, relu=True)
    with ops.knob("conv_splitk", 0):
        unsplit = run().cpu()
    return run, want.permute(0, 2, 3, 1).contiguous(), unsplit


def desc(name, n=None):
    from robosat_amd import _lib

    form, n0, h, w, cin, cout, k, stride, pad, _ = CASES[name]
    n = n or n0
    if form == "phase":
        return _lib.ConvDesc(n, h, w, cin, 0, 1, 3, 3, 1, 1, 2 * h, 2 * w, cout, 1, 0)
    return _lib.ConvDesc(n, h, w, cin, 0, 0, k, k, stride, pad, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1, cout, 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,s", [(name, s) for name, c in CASES.items() for s in c[9]])
def test_split_launch_is_as_close_to_fp64_as_the_unsplit_one(name, s):
    from robosat_amd import ops

    run, want, unsplit = problem(name)
    with ops.knob("conv_splitk", s):
        assert ops.conv_splitk_name(desc(name), phase=CASES[name][0] == "phase").endswith(",k{}>".format(s))  # the split kernels run
        got = run().cpu()
    err_unsplit = float((unsplit.double() - want).abs().max())
    err_split = float((got.double() - want).abs().max())
    print("{} S={}: max |err| vs fp64: unsplit {:.3e}, split {:.3e}".format(name, s, err_unsplit, err_split))
    assert err_unsplit > 0.0 and err_split <= 2.0 * err_unsplit
    if s == 1:  # one slice through the split path: the same sum in the same order, the same epilogue arithmetic
        assert torch.equal(got, unsplit)


@pytest.mark.gpu
def test_split_launch_is_deterministic():
    from robosat_amd import ops

    run, _, _ = problem("phase_ragged_k")
    with ops.knob("conv_splitk", 3):
        a, b = run().cpu(), run().cpu()
    assert torch.equal(a, b)


def center_desc(n):
    from robosat_amd import _lib

    c = CENTER
    return _lib.ConvDesc(n, c["hs"], c["ws"], c["cin"], 0, 1, 3, 3, 1, 1, 2 * c["hs"], 2 * c["ws"], c["cout"], 1, 0)


def shipped_split(n):
    from robosat_amd import _lib

    rowb = ctypes.c_int(0)
    return _lib.lib().rs_conv2d_splitk(ctypes.byref(center_desc(n)), 1, ctypes.byref(rowb))


def test_split_rule_looks_at_the_geometry_only():
    """(CPU) the dispatcher's S for UNet.center: split, and the same at every batch size."""
    from robosat_amd import ops

    assert ops.get_knob("conv_splitk") == -1  # the shipped rule, not an override
    assert shipped_split(1) == shipped_split(16) == shipped_split(32) >= 2


@pytest.mark.gpu
def test_tile_output_does_not_depend_on_the_batch():
    """UNet.center with the shipped rule: tile 0 alone and tile 0 in a batch of three, bit for bit (and twice the same)."""
    from robosat_amd import ops

    c = CENTER
    assert ops.get_knob("conv_splitk") == -1 and shipped_split(1) >= 2 and shipped_split(1) == shipped_split(3)
    x = nhwc(rnd(3, c["cin"], c["hs"], c["ws"], seed=7))
    wp = ops.pack_phase_weight((torch.randn(c["cout"], 3, 3, c["cin"], device=DEV, generator=torch.Generator(DEV).manual_seed(8)) * 0.01))
    three = ops.conv2d_phase(x, wp, relu=True)
    one = ops.conv2d_phase(x[:1].contiguous(), wp, relu=True)
    assert float(one.abs().max()) > 0.0
    assert torch.equal(one[0], three[0])
    assert torch.equal(three, ops.conv2d_phase(x, wp, relu=True))
