"""Thin tensor-level wrappers over the C ABI (``include/robosat_hip.h``).

Tensors are torch CUDA(=HIP) fp32 tensors used purely as device memory: activations are contiguous ``[N,H,W,C]``
(NHWC), convolution weights contiguous ``[Cout,kh,kw,Cin]`` (KRSC).  Work is enqueued on torch's current stream.
Nothing here computes with torch; a CPU tensor is an error (there is no CPU path).
"""

import ctypes
import os

import torch

from . import _lib
from ._lib import RS_BF16, RS_F32, ConvDesc, check

BF16 = torch.bfloat16


def _dt(t):
    """dtype code of an activation tensor (or of a dtype) for the ``*_dt`` entry points."""

    dtype = getattr(t, "dtype", t)
    if dtype == torch.float32:
        return RS_F32
    if dtype == torch.bfloat16:
        return RS_BF16
    raise TypeError("robosat_amd: activations are fp32 or bf16, got {}".format(dtype))


def _esize(t):
    """Bytes per element of an fp32 / bf16 tensor (or dtype)."""

    return 2 if getattr(t, "dtype", t) == BF16 else 4


def _dev(t, name, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("robosat_amd: `{}` is on {} -- the hot path only runs on the MI355X (no CPU fallback)".format(name, t.device))
    if t.dtype != dtype:
        raise TypeError("robosat_amd: `{}` must be {}, got {}".format(name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("robosat_amd: `{}` must be contiguous".format(name))
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, *args):
    """Calls the entry point ``name`` and checks its status under that same name (for the entry points that return one)."""

    rc = getattr(_lib.lib(), name)(*args)
    if rc:
        check(rc, name)


# Kernel-selection switches of the Python side, read from the environment at every call (the tests and bench.py flip them
# mid-process): unset = on, "0" = off, anything else = on.  (The library's own measurement switches: csrc/knobs.hip.)
SWITCHES = {
    "ROBOSAT_WINOGRAD": "fp32 Winograd forward forms (DecoderBlock, stride-1 3x3); off: the generic phase / implicit-GEMM kernels",
    "ROBOSAT_WINO_DGRAD": "Winograd data gradient of the fp32 DecoderBlock; off: the 4x4 / stride-2 kernel",
    "ROBOSAT_WINO33_STATS": "train-mode fp32 conv3x3 -> BatchNorm front half in the Winograd form; off: conv2d_bnstats",
    "ROBOSAT_WINO33_BWD": "Winograd data gradient of the fp32 stride-1 3x3 convolutions; off: the generic kernel",
    "ROBOSAT_FUSED_HEAD": "dec5 + self.final in one launch; off: two launches",
    "ROBOSAT_TAIL_FUSE": "layer1's fused Bottleneck tail and its wave 1x1 kernel; off: the generic 1x1 convolutions",
    "ROBOSAT_S2_DGRAD": "stride-2 data gradients in compact form (3x3: phase form, 1x1: scatter-add); off: zero-insertion convolutions",
    "ROBOSAT_S2_DGRAD_3X3": "the 3x3 half of ROBOSAT_S2_DGRAD alone",
    "ROBOSAT_WGRAD_STREAM": "weight gradients on a side stream; off: serial backward (clean per-kernel timings)",
}


def switch(name):
    """Whether the kernel-selection switch ``name`` (a key of ``SWITCHES``) is on."""

    if name not in SWITCHES:
        raise KeyError("robosat_amd: unknown switch {!r}: one of {}".format(name, ", ".join(SWITCHES)))
    return os.environ.get(name, "1") != "0"


# When set to a list, every conv launch is bracketed by HIP events on the launch stream and the 7-tuple
# (kernel name, algorithmic flops, shape, start event, end event, bytes, executed flops) is appended: bench.py's roofline leg.
PROFILE = None


def _start():
    """Opens the roofline bracket of a launch: None when ``PROFILE`` is off, else the two events, the first recorded on the
    current stream.  A wrapper calls it right before the launch and, when it got events, ``_stop`` right after it, then ``_record``."""

    if PROFILE is None:
        return None
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev[0].record()
    return ev


def _stop(ev):
    ev[1].record()


def _record(ev, name, flops, shape, nbytes, executed=None):
    """One roofline record: ALGORITHMIC flops / bytes of the launch (reference shapes) and the flops
    the kernel actually executes (smaller for the phase-form decoder kernels: 4/9)."""

    PROFILE.append((name, flops, shape, ev[0], ev[1], nbytes, flops if executed is None else executed))


def _shape(d):
    """The launch-shape tuple of a roofline record: (Cin, Cout, k, stride, ups, Ho, Wo)."""

    return (d.C1 + d.C2, d.Cout, d.kh, d.stride, d.ups, d.Ho, d.Wo)


def _partial(rows_fn, d, device, *args):
    """The fp32 buffer [rows, 2, Cout] of a statistics epilogue's per-tile partial sums; ``rows_fn`` answers how many tiles."""

    rows = getattr(_lib.lib(), rows_fn)(ctypes.byref(d), *args)
    if rows <= 0:
        raise ValueError("{}: invalid arguments".format(rows_fn))
    return torch.empty((rows, 2, d.Cout), device=device, dtype=torch.float32)


def _splitk(d, device, phase=False, plain=True):
    """Workspace of a split-K launch (``rs_conv2d_splitk``: the dispatcher's choice for the layer's geometry, fp32 only): the fp32
    buffer [S, rows, Cout] of the slices' partial sums and the launch's K-chunk row size, or (None, 0) when the launch stays unsplit."""

    rowb = ctypes.c_int(0)
    s = _lib.lib().rs_conv2d_splitk(ctypes.byref(d), int(bool(phase)) | (0 if plain else 2), ctypes.byref(rowb))
    if s < 0:
        check(s, "rs_conv2d_splitk")
    if s == 0:
        return None, 0
    return torch.empty((s, d.N * d.Ho * d.Wo, d.Cout), device=device, dtype=torch.float32), rowb.value


def _splitk_name(ws, rowb, phase=False, split=False):
    """Report name of a split-K launch: the 64x64 tile of the implicit-GEMM kernel it runs (the name the roofline tables group
    it under); ``split``: with the number of slices, ``conv_igemm_f32<[phase,]64x64,r<row bytes>,k<S>>``."""

    return "conv_igemm_f32<{}64x64,r{}{}>".format("phase," if phase else "", rowb, ",k{}".format(ws.shape[0]) if split else "")


def conv_splitk_name(d, phase=False, plain=True):
    """``conv_igemm_f32<[phase,]64x64,r<row bytes>,k<S>>`` when the fp32 launch ``d`` runs as S slices of its K loop
    (``rs_conv2d_splitk``: by the layer's geometry, or knob ``conv_splitk``), else None.  Allocates nothing."""

    rowb = ctypes.c_int(0)
    s = _lib.lib().rs_conv2d_splitk(ctypes.byref(d), int(bool(phase)) | (0 if plain else 2), ctypes.byref(rowb))
    if s < 0:
        check(s, "rs_conv2d_splitk")
    return "conv_igemm_f32<{}64x64,r{},k{}>".format("phase," if phase else "", rowb.value, s) if s else None


def conv_flops(d):
    """Algorithmic FLOPs of one launch: 2*N*Cout*Cin*kh*kw*Ho*Wo on the reference's shapes."""

    cin = 3 if d.stem else d.C1 + d.C2  # the stem's 4th (zero) band and 8th (zero) tap are not algorithmic work
    return 2.0 * d.N * d.Cout * cin * d.kh * d.kw * d.Ho * d.Wo


def conv_bytes(d, esize, epilogue_tensors=0):
    """Algorithmic HBM bytes of one launch: every tensor once -- the PRE-upsample sources, the
    weights, the output, and the ``epilogue_tensors`` output-shaped operands the fused epilogue reads (residual, ReLU
    mask, the BatchNorm input of the fused backward statistics)."""

    cin = 4 if d.stem else d.C1 + d.C2
    return esize * (d.N * d.Hs * d.Ws * cin + d.Cout * d.kh * d.kw * cin + (1 + epilogue_tensors) * d.N * d.Ho * d.Wo * d.Cout)


def conv_desc(src1, weight, src2=None, ups=0, stride=1, pad=0, relu=False, stem=0, out_hw=None, bands=4):
    n, hs, ws, c1 = src1.shape
    cout, kh, kw_, _ = weight.shape
    c2 = 0 if src2 is None else src2.shape[3]
    kw = int(stem) if stem else kw_  # packed stem weights are [Cout][kh][8][4]; `stem` carries the true kw (7)
    if out_hw is None:
        assert ups in (0, 1)
        hv, wv = (hs * 2, ws * 2) if ups == 1 else (hs, ws)
        out_hw = ((hv + 2 * pad - kh) // stride + 1, (wv + 2 * pad - kw) // stride + 1)
    # rs_conv_desc.stem: 1 = the packed stem layout; 3 = ... and the caller vouches that the 4th band of the input and the
    # filter's c = 3 entries are zeros (an RGB image through nchw_to_nhwc4 / pack_stem_weight): the kernel skips them
    return ConvDesc(n, hs, ws, c1, c2, ups, kh, kw, stride, pad, out_hw[0], out_hw[1], cout, int(relu),
                    (3 if bands <= 3 else 1) if stem else 0)


def conv2d(src1, weight, src2=None, ups=0, stride=1, pad=0, scale=None, shift=None, residual=None, relu=False,
           stem=0, out_hw=None, out=None, relu_mask=None, alg_scale=1.0, bands=4):
    """``rs_conv2d_fwd``: out = relu?(conv(gather(src1|src2)) * scale + shift + residual).

    ``stem``: 0, or the true filter width (7) when ``weight`` is the packed ``[Cout,kh,8,4]`` stem filter; ``bands``: 3 when
    the image had three bands (its 4th NHWC4 channel and the packed filter's 4th entries are zeros and are skipped).
    ``relu_mask``: tensor shaped like ``out``; the result is zeroed where it is <= 0 (fused ReLU backward)."""

    d = conv_desc(src1, weight, src2, ups, stride, pad, relu, stem, out_hw, bands)
    act = src1.dtype  # fp32: exact-fp32 MFMA kernels; bf16: bf16 operands, fp32 accumulation
    bf = act == BF16
    if bf and stem:
        raise ValueError("the 7x7 stem runs on the fp32 kernel (cast happens at the stem max-pool)")
    if out is None:
        out = torch.empty((d.N, d.Ho, d.Wo, d.Cout), device=src1.device, dtype=act)
    if src2 is not None:
        assert src2.shape[:3] == src1.shape[:3]
    if not stem:
        assert weight.shape[3] == d.C1 + d.C2, "weight Cin {} != {}+{}".format(weight.shape[3], d.C1, d.C2)
    if residual is not None:
        assert residual.shape == out.shape
    if relu_mask is not None:
        assert relu_mask.shape == out.shape
    ws, ws_rowb = (None, 0) if bf or stem else _splitk(d, src1.device, plain=relu_mask is None)
    ev = _start()
    if ws is not None:
        _call("rs_conv2d_fwd_splitk", ctypes.byref(d), 0, _dev(src1, "src1"), _dev(src2, "src2"), _dev(weight, "weight"), _dev(scale, "scale"),
              _dev(shift, "shift"), _dev(residual, "residual"), _dev(out, "out"), _dev(ws, "ws"), ws.shape[0], _stream())
    else:
        _call("rs_conv2d_fwd_bf16" if bf else "rs_conv2d_fwd", ctypes.byref(d), _dev(src1, "src1", act), _dev(src2, "src2", act),
              _dev(weight, "weight", act), _dev(scale, "scale"), _dev(shift, "shift"), _dev(residual, "residual", act),
              _dev(relu_mask, "relu_mask", act), _dev(out, "out", act), _stream())
    if ev:
        _stop(ev)
        name = conv_tile_name(d, bf, plain=relu_mask is None) if ws is None else _splitk_name(ws, ws_rowb)
        if alg_scale != 1.0 and not name.startswith(("conv_thin", "conv_halo")):  # phase-form data gradient: 16 taps at source resolution stand for 9 at the upsampled one
            name = name.replace("<", "<dgrad4x4,")
        _record(ev, name, conv_flops(d) * alg_scale, _shape(d),
                conv_bytes(d, _esize(act), (residual is not None) + (relu_mask is not None)) + (0 if ws is None else 8 * ws.numel()),
                conv_flops(d))
    return out


def conv2d_bnstats(src1, weight, src2=None, ups=0, stride=1, pad=0):
    """Train-mode ``conv -> BatchNorm`` front half: the raw convolution output plus the per-tile partial sums of its
    BatchNorm statistics, produced in the convolution's epilogue (``rs_conv2d_fwd_bnstats_dt``).
    Returns (out, partial [tiles,2,Cout] fp32)."""

    d = conv_desc(src1, weight, src2, ups, stride, pad, False, 0, None)
    act = src1.dtype
    out = torch.empty((d.N, d.Ho, d.Wo, d.Cout), device=src1.device, dtype=act)
    partial = _partial("rs_conv2d_bnstats_rows_dt", d, src1.device, _dt(src1))
    assert weight.shape[3] == d.C1 + d.C2
    ev = _start()
    _call("rs_conv2d_fwd_bnstats_dt", ctypes.byref(d), _dt(src1), _dev(src1, "src1", act), _dev(src2, "src2", act),
          _dev(weight, "weight", act), _dev(out, "out", act), _dev(partial, "partial"), _stream())
    if ev:
        _stop(ev)
        _record(ev, conv_tile_name(d, act == BF16, plain=False), conv_flops(d), _shape(d), conv_bytes(d, _esize(act)))
    return out, partial


def conv2d_dgrad_bnstats(dy, wd, out_hw, bn_y, bn_mean, bn_invstd, ups=0, pad=0, residual=None, relu_mask=None,
                         relu_mask_bits=None, stride=1):
    """Data-gradient convolution whose output g is the gradient at a BatchNorm+ReLU output: ``rs_conv2d_fwd`` semantics
    (``wd`` = packed dgrad weights, optional residual, relu_mask = z) + per-tile partial sums of BatchNorm's two backward
    reductions (``rs_conv2d_dgrad_bnstats_dt``).  ``relu_mask_bits`` (from ``bn_apply(..., want_bits=True)``) replaces
    ``relu_mask`` by one bit per element (``rs_conv2d_dgrad_bnstats_bits_dt``).  Returns (g, partial [tiles,2,C])."""

    d = conv_desc(dy, wd, None, ups, stride, pad, False, 0, out_hw)
    act = dy.dtype
    out = torch.empty((d.N, d.Ho, d.Wo, d.Cout), device=dy.device, dtype=act)
    assert bn_y.shape == out.shape
    partial = _partial("rs_conv2d_bnstats_rows_dt", d, dy.device, _dt(dy))
    ev = _start()
    if relu_mask_bits is not None:
        assert relu_mask_bits.numel() * 8 == out.numel(), "one mask bit per output element"
        _call("rs_conv2d_dgrad_bnstats_bits_dt", ctypes.byref(d), _dt(dy), _dev(dy, "dy", act), _dev(wd, "weight", act),
              _dev(residual, "residual", act), _dev(relu_mask_bits, "relu_mask_bits", torch.uint8), _dev(bn_y, "bn_y", act),
              _dev(bn_mean, "bn_mean"), _dev(bn_invstd, "bn_invstd"), _dev(out, "out", act), _dev(partial, "partial"), _stream())
    else:
        _call("rs_conv2d_dgrad_bnstats_dt", ctypes.byref(d), _dt(dy), _dev(dy, "dy", act), _dev(wd, "weight", act),
              _dev(residual, "residual", act), _dev(relu_mask, "relu_mask", act), _dev(bn_y, "bn_y", act), _dev(bn_mean, "bn_mean"),
              _dev(bn_invstd, "bn_invstd"), _dev(out, "out", act), _dev(partial, "partial"), _stream())
    if ev:
        _stop(ev)
        _record(ev, conv_tile_name(d, act == BF16, plain=False), conv_flops(d), _shape(d),
                conv_bytes(d, _esize(act), 1 + (residual is not None) + (relu_mask is not None))
                + (out.numel() // 8 if relu_mask_bits is not None else 0))
    return out, partial


def bn_bwd_from_partials(g, y, mean, invstd, gamma, partial, dgamma=None, dbeta=None):
    """BatchNorm backward from ``conv2d_dgrad_bnstats``'s partial sums: returns (dy, dgamma, dbeta); ``g`` is already
    masked by the ReLU, so it is also the gradient of a residual branch."""

    c = y.shape[-1]
    m = y.numel() // c
    dy = torch.empty_like(y)
    if dgamma is None:
        dgamma = torch.empty(c, device=y.device, dtype=torch.float32)
    if dbeta is None:
        dbeta = torch.empty(c, device=y.device, dtype=torch.float32)
    t = y.dtype
    _call("rs_bn_bwd_from_partials_dt", _dev(g, "g", t), _dev(y, "y", t), _dev(mean, "mean"), _dev(invstd, "invstd"), _dev(gamma, "gamma"),
          _dev(dy, "dy", t), _dev(dgamma, "dgamma"), _dev(dbeta, "dbeta"), _dev(partial, "partial"), partial.shape[0], _dt(y), m, c,
          _workspace(64 * 2 * c * 8 + 3 * c * 4, y.device), _stream())
    return dy, dgamma, dbeta


def bn_finalize_stats(partial, m, gamma, beta, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None):
    """(mean, invstd, scale, shift) from ``conv2d_bnstats``'s partial sums; updates the running buffers like bn_train_stats."""

    rows, _, c = partial.shape
    mean, invstd, scale, shift = (torch.empty(c, device=partial.device, dtype=torch.float32) for _ in range(4))
    _call("rs_bn_finalize_stats", _dev(partial, "partial"), rows, m, c, ctypes.c_float(eps), ctypes.c_float(momentum), _dev(gamma, "gamma"),
          _dev(beta, "beta"), _dev(mean, "mean"), _dev(invstd, "invstd"), _dev(scale, "scale"), _dev(shift, "shift"),
          _dev(running_mean, "running_mean"), _dev(running_var, "running_var"),
          _dev(num_batches_tracked, "num_batches_tracked", torch.int64), _workspace(64 * 2 * c * 8, partial.device), _stream())
    return mean, invstd, scale, shift


def pack_phase_weight(w_krsc, dtype=torch.float32):
    """fp32 KRSC [Cout,3,3,Cin] -> [4,Cout,2,2,Cin] in ``dtype``: the four parity-specific 2x2 filters that a 3x3 / pad-1
    convolution over a nearest-x2 upsampled input collapses to (``rs_pack_phase_weight_dt``)."""

    cout, kh, kw, cin = w_krsc.shape
    assert kh == 3 and kw == 3
    out = torch.empty((4, cout, 2, 2, cin), device=w_krsc.device, dtype=dtype)
    _call("rs_pack_phase_weight_dt", _dev(w_krsc, "w"), _dev(out, "out", dtype), _dt(dtype), cout, cin, _stream())
    return out


def pack_s2_dgrad_phase_weight(w_krsc, dtype=torch.float32):
    """fp32 KRSC [Cout,3,3,Cin] of a 3x3 / stride-2 / pad-1 convolution -> [4,Cin,2,2,Cout] in ``dtype``: the phase pack of its DATA
    gradient (``rs_pack_s2_dgrad_phase_weight_dt``) -- ``conv2d_phase(dy, pack)`` is the gradient wrt the input (even sizes)."""

    cout, kh, kw, cin = w_krsc.shape
    assert kh == 3 and kw == 3
    out = torch.empty((4, cin, 2, 2, cout), device=w_krsc.device, dtype=dtype)
    _call("rs_pack_s2_dgrad_phase_weight_dt", _dev(w_krsc, "w"), _dev(out, "out", dtype), _dt(dtype), cout, cin, _stream())
    return out


def pack_dgrad_phase_weight(w_krsc, dtype=torch.float32):
    """fp32 KRSC [Cout,3,3,Cin] -> [Cin,4,4,Cout] in ``dtype``: weights of the 4x4 / stride-2 convolution over dz that is
    the data gradient of DecoderBlock wrt its pre-upsample input (``rs_pack_dgrad_phase_weight_dt``)."""

    cout, kh, kw, cin = w_krsc.shape
    assert kh == 3 and kw == 3
    out = torch.empty((cin, 4, 4, cout), device=w_krsc.device, dtype=dtype)
    # two coalesced steps: LDS-tiled transpose to [Cin,3,3,Cout] (rs_pack_dgrad_weight), then the tap sums along Cout
    wt = pack_dgrad_weight(w_krsc, torch.float32)
    _call("rs_combine_dgrad_phase_weight_dt", _dev(wt, "wt"), _dev(out, "out", dtype), _dt(dtype), cout, cin, _stream())
    return out


def conv2d_split(src, weight, c1, stride=1, pad=0, out_hw=None, mask1=None, mask2=None, alg_scale=1.0):
    """``rs_conv2d_fwd_split_dt``: one convolution whose output channels [0, c1) and [c1, Cout) land in two tensors (the
    backward of torch.cat fused into the store), each with its optional ReLU mask.  Returns (out1, out2)."""

    d = conv_desc(src, weight, None, 0, stride, pad, False, 0, out_hw)
    act = src.dtype
    c2 = d.Cout - c1
    out1 = torch.empty((d.N, d.Ho, d.Wo, c1), device=src.device, dtype=act)
    out2 = torch.empty((d.N, d.Ho, d.Wo, c2), device=src.device, dtype=act)
    ev = _start()
    _call("rs_conv2d_fwd_split_dt", ctypes.byref(d), _dt(src), _dev(src, "src", act), _dev(weight, "weight", act), _dev(out1, "out1", act),
          _dev(mask1, "mask1", act), _dev(out2, "out2", act), _dev(mask2, "mask2", act), c1, _stream())
    if ev:
        _stop(ev)
        name = conv_tile_name(d, act == BF16, plain=False)
        if alg_scale != 1.0 and not name.startswith("conv_halo"):
            name = name.replace("<", "<dgrad4x4,")
        _record(ev, name, conv_flops(d) * alg_scale, _shape(d),
                conv_bytes(d, _esize(act), ((mask1 is not None) * c1 + (mask2 is not None) * (d.Cout - c1)) / d.Cout), conv_flops(d))
    return out1, out2


def cat_split_bwd(dcat, c1, c2=0, mask1=None, mask2=None, out1=None):
    """dcat [N,H,W,C1+C2] -> (d1 [N,H,W,C1], d2 [N,H,W,C2] or None): the torch.cat split + ReLU masks; ``out1`` given =>
    accumulate into it."""

    n, h, w, ct = dcat.shape
    assert ct == c1 + c2
    t = dcat.dtype
    acc = out1 is not None
    d1 = out1 if acc else torch.empty((n, h, w, c1), device=dcat.device, dtype=t)
    d2 = torch.empty((n, h, w, c2), device=dcat.device, dtype=t) if c2 else None
    _call("rs_cat_split_bwd_dt", _dev(dcat, "dcat", t), _dev(d1, "d1", t), _dev(d2, "d2", t), _dev(mask1, "mask1", t),
          _dev(mask2, "mask2", t), _dt(dcat), n, h, w, c1, c2, int(acc), _stream())
    return d1, d2


def _phase_desc(n, hs, ws, c1, c2, cout, relu=False):
    """DecoderBlock: sources [n,hs,ws,c1(+c2)], nearest x2, 3x3 / pad 1 -> [n,2hs,2ws,cout]."""

    return ConvDesc(n, hs, ws, c1, c2, 1, 3, 3, 1, 1, 2 * hs, 2 * ws, cout, int(relu), 0)


def _conv33_desc(src, cout, relu):
    n, h, w, c = src.shape
    return ConvDesc(n, h, w, c, 0, 0, 3, 3, 1, 1, h, w, cout, int(relu), 0)


def conv2d_phase(src1, weight_phase, src2=None, scale=None, shift=None, residual=None, relu=False, relu_mask=None):
    """DecoderBlock in phase form: relu?(conv3x3(interpolate(cat[src1, src2], x2 nearest), pad 1)) computed as four 2x2
    convolutions on the source grid (``rs_conv2d_fwd_phase_dt``); ``weight_phase`` from ``pack_phase_weight``."""

    n, hs, ws, c1 = src1.shape
    c2 = 0 if src2 is None else src2.shape[3]
    cout = weight_phase.shape[1]
    assert tuple(weight_phase.shape) == (4, cout, 2, 2, c1 + c2)
    if src2 is not None and tuple(src2.shape[:3]) != (n, hs, ws):
        # what torch.cat raises in the reference (unet.py:134-137) when a skip and the decoder tensor disagree
        raise RuntimeError("Sizes of tensors must match except in dimension 1: skip {} vs decoder {}".format(
            tuple(src1.shape[:3]), tuple(src2.shape[:3])))
    act = src1.dtype
    d = _phase_desc(n, hs, ws, c1, c2, cout, relu)
    out = torch.empty((n, 2 * hs, 2 * ws, cout), device=src1.device, dtype=act)
    ws, ws_rowb = (None, 0) if act == BF16 else _splitk(d, src1.device, phase=True, plain=relu_mask is None)
    ev = _start()
    if ws is not None:
        _call("rs_conv2d_fwd_splitk", ctypes.byref(d), 1, _dev(src1, "src1"), _dev(src2, "src2"), _dev(weight_phase, "weight"),
              _dev(scale, "scale"), _dev(shift, "shift"), _dev(residual, "residual"), _dev(out, "out"), _dev(ws, "ws"), ws.shape[0], _stream())
    else:
        _call("rs_conv2d_fwd_phase_dt", ctypes.byref(d), _dt(src1), _dev(src1, "src1", act), _dev(src2, "src2", act),
              _dev(weight_phase, "weight", act), _dev(scale, "scale"), _dev(shift, "shift"), _dev(residual, "residual", act),
              _dev(relu_mask, "relu_mask", act), _dev(out, "out", act), _stream())
    if ev:
        _stop(ev)
        _record(ev, conv_tile_name(d, act == BF16, phase=True, plain=relu_mask is None) if ws is None else _splitk_name(ws, ws_rowb, phase=True), conv_flops(d), _shape(d),
                conv_bytes(d, _esize(act), (residual is not None) + (relu_mask is not None)) + (0 if ws is None else 8 * ws.numel()),
                conv_flops(d) * 4.0 / 9.0)
    return out


def wino_ok(src1, src2, cout, force=False):
    """Whether the fp32 Winograd form of DecoderBlock (``conv2d_phase_wino``) should run this layer
    (``rs_conv2d_phase_wino_ok``: it can, and the launch is large enough to fill the chip); ``force``: whether it CAN (the
    parity tests reach the kernel with small problems).  ROBOSAT_WINOGRAD=0 switches it off (A/B measurements: the generic
    phase kernel then runs every layer)."""

    if src1.dtype != torch.float32 or not (force or switch("ROBOSAT_WINOGRAD")):
        return False
    d = _phase_desc(*src1.shape, 0 if src2 is None else src2.shape[3], cout)
    rc = _lib.lib().rs_conv2d_phase_wino_ok(ctypes.byref(d))
    return rc != 0 if force else rc == 1


def pack_wino_phase_weight(weight_phase):
    """Phase pack [4,Cout,2,2,Cin] fp32 -> U = G g G^T, [4,9,Cout,Cin]: the transformed filters of the Winograd form."""

    _, cout, _, _, cin = weight_phase.shape
    u = torch.empty((4, 9, cout, cin), device=weight_phase.device, dtype=torch.float32)
    _call("rs_pack_wino_phase_weight", _dev(weight_phase, "w_phase"), _dev(u, "u"), cout, cin, _stream())
    return u


def conv2d_phase_wino(src1, u, src2=None, relu=False, upsampled=False):
    """DecoderBlock in fp32 as a Winograd F(2x2, 2x2) convolution on the phase form (``rs_conv2d_fwd_phase_wino``): same
    result as ``conv2d_phase`` up to fp32 summation order, 9/16 of its multiply-adds.  ``upsampled``: ``u`` comes from
    ``pack_phase_weight`` -- a 3x3 filter over the nearest-x2 upsample, whose parity filters are sums of the same three taps per
    axis --, which lets the kernel compute all four parities per source pixel (``rs_conv2d_fwd_upsampled_wino``, the pixel form);
    False: four free 2x2 parity filter sets (any phase pack, e.g. ``pack_s2_dgrad_phase_weight``'s), one parity per work item."""

    n, hs, ws, c1 = src1.shape
    c2 = 0 if src2 is None else src2.shape[3]
    cout = u.shape[2]
    assert tuple(u.shape) == (4, 9, cout, c1 + c2)
    if src2 is not None and tuple(src2.shape[:3]) != (n, hs, ws):
        raise RuntimeError("Sizes of tensors must match except in dimension 1: skip {} vs decoder {}".format(
            tuple(src1.shape[:3]), tuple(src2.shape[:3])))
    d = _phase_desc(n, hs, ws, c1, c2, cout, relu)
    out = torch.empty((n, 2 * hs, 2 * ws, cout), device=src1.device, dtype=torch.float32)
    ev = _start()
    _call("rs_conv2d_fwd_upsampled_wino" if upsampled else "rs_conv2d_fwd_phase_wino", ctypes.byref(d),
          _dev(src1, "src1"), _dev(src2, "src2"), _dev(u, "u"), _dev(out, "out"), _stream())
    if ev:
        _stop(ev)
        name = _lib.lib().rs_conv2d_phase_wino_name(ctypes.byref(d)).decode()
        # executed: 9 multiply-adds per 2x2 outputs of a parity = 1/4 of the reference-shape count (the phase form: 4/9)
        _record(ev, name, conv_flops(d), _shape(d), conv_bytes(d, 4), conv_flops(d) * 0.25)
    return out


def wino_dgrad_ok(n, hs, ws, c1, c2, cout):
    """Whether the fp32 DecoderBlock (sources [n,hs,ws,c1(+c2)] -> cout at 2 hs x 2 ws) can take its data gradient through the Winograd
    form (``rs_conv2d_dgrad_phase_wino_ok``: geometry only; ROBOSAT_WINO_DGRAD=0 keeps the 4x4 / stride-2 kernel for A/B runs)."""

    if not switch("ROBOSAT_WINO_DGRAD"):
        return False
    return _lib.lib().rs_conv2d_dgrad_phase_wino_ok(ctypes.byref(_phase_desc(n, hs, ws, c1, c2, cout))) == 1


def pack_wino_dgrad_weight(wd4x4):
    """[Cin,4,4,Cout] fp32 (``pack_dgrad_phase_weight``) -> the transformed data-gradient filters [4,9,Cin,Cout]
    (``rs_pack_wino_dgrad_weight``)."""

    cin, kh, kw, cout = wd4x4.shape
    assert kh == 4 and kw == 4 and wd4x4.dtype == torch.float32
    u = torch.empty((4, 9, cin, cout), device=wd4x4.device, dtype=torch.float32)
    _call("rs_pack_wino_dgrad_weight", _dev(wd4x4, "wd"), _dev(u, "u"), cin, cout, _stream())
    return u


def conv2d_dgrad_phase_wino(dz, u, c1, c2=0, mask1=None, mask2=None, split=False):
    """Data gradient of the fp32 DecoderBlock wrt cat[skip, prev] at source resolution (``rs_conv2d_dgrad_phase_wino``): ``dz``
    [N,2Hs,2Ws,Cout], ``u`` from ``pack_wino_dgrad_weight``.  ``split``: two tensors ([..,c1], [..,c2]) with their optional ReLU masks
    (torch.cat's backward fused into the store); else one tensor [..,c1+c2] with ``mask1``.  Returns (d1, d2 | None)."""

    n, ho, wo, cout = dz.shape
    hs, ws = ho // 2, wo // 2
    assert tuple(u.shape) == (4, 9, c1 + c2, cout) and dz.dtype == torch.float32 and (ho, wo) == (2 * hs, 2 * ws)
    d = _phase_desc(n, hs, ws, c1, c2, cout)
    if split:
        out1 = torch.empty((n, hs, ws, c1), device=dz.device, dtype=torch.float32)
        out2 = torch.empty((n, hs, ws, c2), device=dz.device, dtype=torch.float32)
    else:
        out1, out2 = torch.empty((n, hs, ws, c1 + c2), device=dz.device, dtype=torch.float32), None
        assert mask2 is None
    for m, o in ((mask1, out1), (mask2, out2)):
        assert m is None or tuple(m.shape) == tuple(o.shape)
    ev = _start()
    _call("rs_conv2d_dgrad_phase_wino", ctypes.byref(d), _dev(dz, "dz"), _dev(u, "u"), _dev(out1, "out"), _dev(mask1, "mask"),
          _dev(out2, "out2"), _dev(mask2, "mask2"), c1 if split else 0, _stream())
    if ev:
        _stop(ev)
        # algorithmic: the reference's 3x3 at the upsampled resolution; the 4x4 / stride-2 form executes 16 taps at source resolution,
        # this form 9/16 of those
        alg = 2.0 * n * ho * wo * cout * (c1 + c2) * 9
        ex4 = 2.0 * n * hs * ws * cout * (c1 + c2) * 16
        nbytes = 4 * (n * ho * wo * cout + 16 * cout * (c1 + c2) + n * hs * ws * (c1 + c2) * (1 + (mask1 is not None) * (c1 if split else c1 + c2) / (c1 + c2)
                                                                                            + (mask2 is not None) * c2 / (c1 + c2)))
        _record(ev, _lib.lib().rs_conv2d_dgrad_phase_wino_name(ctypes.byref(d)).decode(), alg, (cout, c1 + c2, 4, 2, 0, hs, ws), nbytes,
                ex4 * 9.0 / 16.0)
    return out1, out2


def wino33_ok(src, cout):
    """Whether the fp32 Winograd F(2x2, 3x3) kernel runs a stride-1 3x3 / pad-1 convolution of ``src`` to ``cout`` channels
    (``rs_conv2d_wino33_ok``: the layer's geometry only, never the batch size); ROBOSAT_WINOGRAD=0 switches it off."""

    if src.dtype != torch.float32 or not switch("ROBOSAT_WINOGRAD"):
        return False
    return _lib.lib().rs_conv2d_wino33_ok(ctypes.byref(_conv33_desc(src, cout, False))) == 1


def pack_wino33_weight(w_krsc):
    """fp32 KRSC [Cout,3,3,Cin] -> U = G g G^T, [16,Cout,Cin]: the transformed filters of the F(2x2, 3x3) form."""

    cout, kh, kw, cin = w_krsc.shape
    assert kh == 3 and kw == 3
    u = torch.empty((16, cout, cin), device=w_krsc.device, dtype=torch.float32)
    _call("rs_pack_wino33_weight", _dev(w_krsc, "w"), _dev(u, "u"), cout, cin, _stream())
    return u


def conv2d_wino33(src, u, scale=None, shift=None, relu=False):
    """relu?(conv3x3(src, pad 1) * scale + shift) in fp32 as a Winograd F(2x2, 3x3) convolution (``rs_conv2d_fwd_wino33``):
    the eval-mode Bottleneck conv2 / dec5 of the predict path; 4/9 of the direct form's multiply-adds."""

    n, h, w, c = src.shape
    cout = u.shape[1]
    assert tuple(u.shape) == (16, cout, c)
    d = _conv33_desc(src, cout, relu)
    out = torch.empty((n, h, w, cout), device=src.device, dtype=torch.float32)
    ev = _start()
    _call("rs_conv2d_fwd_wino33", ctypes.byref(d), _dev(src, "src"), _dev(u, "u"), _dev(scale, "scale"), _dev(shift, "shift"),
          _dev(out, "out"), _stream())
    if ev:
        _stop(ev)
        name = _lib.lib().rs_conv2d_wino33_name(ctypes.byref(d)).decode()
        _record(ev, name, conv_flops(d), _shape(d), conv_bytes(d, 4), conv_flops(d) * 4.0 / 9.0)
    return out


def conv2d_wino33_bnstats(src, u):
    """Train-mode ``conv3x3 -> BatchNorm`` front half in the fp32 Winograd form (``rs_conv2d_fwd_wino33_stats``): the raw output and
    the per-block partial sums of its statistics, as ``conv2d_bnstats`` returns them.  ROBOSAT_WINO33_STATS=0 at the call site keeps
    the generic kernel (A/B runs)."""

    n, h, w, c = src.shape
    cout = u.shape[1]
    assert tuple(u.shape) == (16, cout, c) and src.dtype == torch.float32
    d = _conv33_desc(src, cout, False)
    out = torch.empty((n, h, w, cout), device=src.device, dtype=torch.float32)
    partial = _partial("rs_conv2d_wino33_stats_rows", d, src.device)
    ev = _start()
    _call("rs_conv2d_fwd_wino33_stats", ctypes.byref(d), _dev(src, "src"), _dev(u, "u"), _dev(out, "out"), _dev(partial, "partial"),
          _stream())
    if ev:
        _stop(ev)
        _record(ev, _lib.lib().rs_conv2d_wino33_name(ctypes.byref(d)).decode().replace("<3x3,", "<3x3+stats,"), conv_flops(d), _shape(d),
                conv_bytes(d, 4), conv_flops(d) * 4.0 / 9.0)
    return out, partial


def wino33_dgrad_ok(dy, cout):
    """Whether the fp32 data gradient of a stride-1 3x3 / pad-1 convolution (dy [n,h,w,c] -> [n,h,w,cout]) takes the Winograd form
    (``rs_conv2d_dgrad_wino33``: ``wino33_ok`` on the gradient's convolution, cout % 32 == 0); ROBOSAT_WINO33_BWD=0 keeps the generic
    kernel (A/B runs)."""

    if not switch("ROBOSAT_WINO33_BWD") or cout % 32:
        return False
    return wino33_ok(dy, cout)


def conv2d_wino33_dgrad(dy, u, relu_mask=None, relu_mask_bits=None, bn=None):
    """``rs_conv2d_dgrad_wino33``: the data gradient of a stride-1 3x3 convolution in the fp32 Winograd form -- ``u`` =
    ``pack_wino33_weight(pack_dgrad_weight(w))`` -- masked by the ReLU it arrives at (``relu_mask``: the forward activation;
    ``relu_mask_bits``: its bit form) and, with ``bn`` = (y, mean, invstd), with the partial sums of BatchNorm's two backward reductions,
    as ``conv2d_dgrad_bnstats`` returns them.  Returns (g, partial or None)."""

    n, h, w, c = dy.shape
    cout = u.shape[1]
    assert tuple(u.shape) == (16, cout, c) and dy.dtype == torch.float32
    d = _conv33_desc(dy, cout, False)
    out = torch.empty((n, h, w, cout), device=dy.device, dtype=torch.float32)
    partial = None
    y = mean = invstd = None
    if bn is not None:
        y, mean, invstd = bn
        assert y.shape == out.shape
        partial = _partial("rs_conv2d_wino33_stats_rows", d, dy.device)
    if relu_mask is not None:
        assert relu_mask.shape == out.shape
    if relu_mask_bits is not None:
        assert relu_mask_bits.numel() * 8 == out.numel(), "one mask bit per output element"
    ev = _start()
    _call("rs_conv2d_dgrad_wino33", ctypes.byref(d), _dev(dy, "dy"), _dev(u, "u"), _dev(relu_mask, "relu_mask"),
          _dev(relu_mask_bits, "relu_mask_bits", torch.uint8), _dev(y, "bn_y"), _dev(mean, "bn_mean"), _dev(invstd, "bn_invstd"),
          _dev(out, "out"), _dev(partial, "partial"), _stream())
    if ev:
        _stop(ev)
        _record(ev, _lib.lib().rs_conv2d_wino33_name(ctypes.byref(d)).decode().replace("<3x3,", "<3x3+bwd,"), conv_flops(d), _shape(d),
                conv_bytes(d, 4, 1 + (relu_mask is not None) + (bn is not None)) + (out.numel() // 8 if relu_mask_bits is not None else 0),
                conv_flops(d) * 4.0 / 9.0)
    return out, partial


def wino33_head_ok(src, cout, classes):
    """Whether dec5 + ``self.final`` run as one launch (``rs_conv2d_wino33_head_ok``: the Winograd 3x3 form on a 32-cout
    layer, <= 8 classes); ROBOSAT_FUSED_HEAD=0 keeps the two launches (A/B runs)."""

    if not wino33_ok(src, cout) or not switch("ROBOSAT_FUSED_HEAD"):
        return False
    return _lib.lib().rs_conv2d_wino33_head_ok(ctypes.byref(_conv33_desc(src, cout, True)), int(classes)) == 1


def conv2d_wino33_head(src, u, final_w, final_b, mode="logits", overlap=0, relu=True):
    """``final(relu(conv3x3(src, pad 1)))`` in one launch (``rs_conv2d_fwd_wino33_head``; reference unet.py:139-141) and, by
    ``mode``, what the ``final_conv1x1*`` functions return: "logits" / "softmax" -> fp32 NCHW [N,C,H,W]; "quantize" ->
    uint8 quantised probabilities of the crop without the ``overlap`` border; "argmax" -> uint8 [N,H,W] class indices."""

    n, h, w, c = src.shape
    cout, classes = u.shape[1], final_w.shape[0]
    assert tuple(u.shape) == (16, cout, c) and tuple(final_w.shape) == (classes, cout)
    d = _conv33_desc(src, cout, relu)
    m = {"logits": 0, "softmax": 1, "quantize": 2, "argmax": 3}[mode]
    out = qout = anchors = None
    if m <= 1:
        out = torch.empty((n, classes, h, w), device=src.device, dtype=torch.float32)
    elif m == 2:
        shape = (n, h - 2 * overlap, w - 2 * overlap) + ((classes - 1,) if classes > 2 else ())
        qout = torch.empty(shape, device=src.device, dtype=torch.uint8)
        anchors = _anchors(src.device)
    else:
        qout = torch.empty((n, h, w), device=src.device, dtype=torch.uint8)
    ev = _start()
    _call("rs_conv2d_fwd_wino33_head", ctypes.byref(d), _dev(src, "src"), _dev(u, "u"), None, None, _dev(final_w, "final_w"),
          _dev(final_b, "final_b"), classes, m, _dev(anchors, "anchors", torch.float64), int(overlap), _dev(out, "out"),
          _dev(qout, "qout", torch.uint8), _stream())
    if ev:
        _stop(ev)
        fl = conv_flops(d) + 2.0 * n * h * w * cout * classes  # (the 1x1 rides along: < 1 % of the launch)
        nbytes = 4 * (n * h * w * c + 9 * cout * c + classes * cout) + (4 * classes if m <= 1 else 1) * n * h * w
        _record(ev, _lib.lib().rs_conv2d_wino33_head_name().decode(), fl, _shape(d), nbytes,
                conv_flops(d) * 4.0 / 9.0 + 2.0 * n * h * w * cout * classes)
    return out if m <= 1 else qout


def bottleneck_tail_ok(x, w3, w1):
    """Whether ``bottleneck_tail`` can run these operands: fp32, layer1's widths (64 -> 256 -> 64), whole 32-pixel sub-tiles."""

    m = x.numel() // x.shape[-1]
    return (x.dtype == torch.float32 and x.shape[-1] == 64 and tuple(w3.shape) == (256, 1, 1, 64) and tuple(w1.shape) == (64, 1, 1, 256)
            and m % 32 == 0 and switch("ROBOSAT_TAIL_FUSE"))


def bottleneck_tail(x, w3, scale3, shift3, identity, w1, scale1, shift1):
    """``rs_bottleneck_tail_f32``: out = relu(conv1x1(x; w3) * scale3 + shift3 + identity) and z = relu(conv1x1(out; w1) * scale1 +
    shift1) in one launch -- the last convolution of a layer1 Bottleneck and the first of the next (eval mode, fp32).  Returns (out, z)."""

    n, h, w, c1 = x.shape
    cm, c2 = w3.shape[0], w1.shape[0]
    assert identity.shape == (n, h, w, cm) and w1.shape[3] == cm
    out = torch.empty((n, h, w, cm), device=x.device, dtype=torch.float32)
    z = torch.empty((n, h, w, c2), device=x.device, dtype=torch.float32)
    ev = _start()
    _call("rs_bottleneck_tail_f32", _dev(x, "x"), _dev(w3, "w3"), _dev(scale3, "scale3"), _dev(shift3, "shift3"),
          _dev(identity, "identity"), _dev(w1, "w1"), _dev(scale1, "scale1"), _dev(shift1, "shift1"), _dev(out, "out"), _dev(z, "z"),
          n * h * w, c1, cm, c2, _stream())
    if ev:
        _stop(ev)
        m = n * h * w
        fl = 2.0 * m * cm * (c1 + c2)
        _record(ev, "bottleneck_tail_f32", fl, (c1, cm, 1, 1, 0, h, w), 4 * (m * (c1 + 2 * cm + c2) + cm * (c1 + c2)), fl)
    return out, z


def conv1x1_wave_ok(x, w):
    """Whether ``conv1x1_wave`` can run: fp32, 64 -> 256, 1x1, whole 32-pixel sub-tiles (layer1's downsample branch)."""

    m = x.numel() // x.shape[-1]
    return (x.dtype == torch.float32 and x.shape[-1] == 64 and tuple(w.shape) == (256, 1, 1, 64) and m % 32 == 0
            and switch("ROBOSAT_TAIL_FUSE"))


def conv1x1_wave(x, w, scale, shift, residual=None, relu=False):
    """``rs_conv1x1_wave_f32``: [relu](conv1x1(x; w) * scale + shift [+ residual]) on the fused tail's first stage alone."""

    n, h, wd, c1 = x.shape
    cout = w.shape[0]
    out = torch.empty((n, h, wd, cout), device=x.device, dtype=torch.float32)
    if residual is not None:
        assert residual.shape == out.shape
    ev = _start()
    _call("rs_conv1x1_wave_f32", _dev(x, "x"), _dev(w, "w"), _dev(scale, "scale"), _dev(shift, "shift"), _dev(residual, "residual"),
          int(relu), _dev(out, "out"), n * h * wd, c1, cout, _stream())
    if ev:
        _stop(ev)
        m = n * h * wd
        fl = 2.0 * m * cout * c1
        _record(ev, "conv1x1_wave_f32", fl, (c1, cout, 1, 1, 0, h, wd), 4 * (m * (c1 + cout * (2 if residual is not None else 1)) + cout * c1), fl)
    return out


def conv_tile_name(d, bf16=False, phase=False, plain=True):
    """Report name of the kernel a convolution launch runs, 1:1 with the launched symbol:
    ``conv_igemm_<f32|bf16><[phase,]BMxBN,r<row bytes>>`` (or the stem kernel).  ``plain=False``: a launch with fused
    BatchNorm statistics / a ReLU mask / two destinations: never the plain-epilogue 1x1 kernel of conv1x1_ew_f32.hip, and in bf16 never
    the thin phase kernel, which has no mask input -- a 128 -> 32 phase launch is then reported as the generic tile that runs it."""

    lib = _lib.lib()
    if d.stem:
        return lib.rs_conv2d_tile_name(lib.rs_conv2d_tile(ctypes.byref(d))).decode()
    tile, rowb = ctypes.c_int(0), ctypes.c_int(0)
    form = int(bool(phase)) | (0 if plain else 2)  # (the library answers for the epilogue kind: no knob is touched around the query)
    _call("rs_conv2d_config", ctypes.byref(d), 2 if bf16 else 4, form, ctypes.byref(tile), ctypes.byref(rowb))
    base = (lib.rs_conv2d_tile_name_bf16 if bf16 else lib.rs_conv2d_tile_name)(tile.value).decode()
    if tile.value == TILES["thin"]:  # conv_thin_bf16.hip: named by the form it computes
        return "{}<{}>".format(base, "phase" if phase else ("dgrad4x4" if d.kh == 4 else "3x3"))
    if tile.value == TILES["halo"]:  # halo-once forms of the kernel: form + patch pixels x N tile (`rowb` carries the N tile)
        return "{}<{},{}x{}>".format(base, "phase" if phase else ("dgrad4x4" if d.kh == 4 else "3x3"),
                                     512 if rowb.value & 0x1000 else 256, rowb.value & 0xFFF)
    return base.replace("<", "<phase," if phase else "<").replace(">", ",r{}>".format(rowb.value))


TILES = {"128x128": 0, "128x64": 1, "128x32": 2, "64x64": 3, "256x128": 5, "256x256": 6, "thin": 7, "halo": 8}


class tuning:
    """``with ops.tuning(tile="256x256", rowb=128): ...`` -- force the convolution dispatcher (``rs_conv2d_set_tuning``) for
    the launches inside: the parity tests use it to reach every kernel symbol with small problems, the layer benchmarks
    for A/B runs.  Process-global; restores the measured heuristics on exit."""

    def __init__(self, tile=None, rowb=0):
        self.tile = -1 if tile is None else (TILES[tile] if isinstance(tile, str) else int(tile))
        self.rowb = int(rowb)

    def __enter__(self):
        _call("rs_conv2d_set_tuning", self.tile, self.rowb)
        return self

    def __exit__(self, *exc):
        _call("rs_conv2d_set_tuning", -1, 0)
        return False


def get_knob(name):
    """Current value of one of the library's measurement switches (``rs_get_knob``; the table is in csrc/knobs.hip)."""

    v = ctypes.c_int(0)
    check(_lib.lib().rs_get_knob(name.encode(), ctypes.byref(v)), "rs_get_knob({})".format(name))
    return v.value


def set_knob(name, value):
    """``rs_set_knob`` (process-global; prefer ``with ops.knob(...)`` where the old value should come back)."""

    check(_lib.lib().rs_set_knob(name.encode(), int(value)), "rs_set_knob({})".format(name))


class knob:
    """``with ops.knob("conv1x1_ew", 0): ...`` -- set a measurement switch of the library (``rs_set_knob``) for the launches
    inside and restore it on exit.  Process-global, like ``ops.tuning``: for tests and A/B scripts, not a tuning API."""

    def __init__(self, name, value):
        self.name, self.value, self.old = name, int(value), None

    def __enter__(self):
        self.old = get_knob(self.name)
        set_knob(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_knob(self.name, self.old)
        return False


def cast_bf16(t):
    """fp32 -> bf16 copy (round to nearest even); used for the per-step compute copies of the fp32 master weights."""

    out = torch.empty(t.shape, device=t.device, dtype=BF16)
    _call("rs_cast_f32_to_bf16", _dev(t, "src"), _dev(out, "dst", BF16), t.numel(), _stream())
    return out


def cast_bf16_scaled(t, scale):
    """bf16(t * scale): a gradient bucket on its way to a bf16 exchange, already divided by the world size."""

    out = torch.empty(t.shape, device=t.device, dtype=BF16)
    _call("rs_cast_f32_to_bf16_scaled", _dev(t, "src"), _dev(out, "dst", BF16), t.numel(), ctypes.c_float(scale), _stream())
    return out


def cast_f32_scaled(src_bf16, dst_f32, scale):
    """dst (fp32, in place) = float(src bf16) * scale: the way back from a bf16 gradient exchange (``GradReducer``)."""

    assert src_bf16.numel() == dst_f32.numel()
    _call("rs_cast_bf16_to_f32_scaled", _dev(src_bf16, "src", BF16), _dev(dst_f32, "dst"), src_bf16.numel(), ctypes.c_float(scale),
          _stream())
    return dst_f32


class _WPrepItem(ctypes.Structure):  # rs_wprep_item (include/robosat_hip.h)
    _fields_ = [("w", ctypes.c_void_p), ("cast", ctypes.c_void_p), ("dgrad", ctypes.c_void_p), ("Cout", ctypes.c_int),
                ("taps", ctypes.c_int), ("Cin", ctypes.c_int), ("tile_begin", ctypes.c_int)]


class WeightPrep:
    """One launch (``rs_weight_prep_bf16``) that refreshes the bf16 compute copies of a fixed set of fp32 KRSC weights:
    the bf16 KRSC cast and the transposed, tap-flipped data-gradient layout of each -- bit-identical to ``cast_bf16`` /
    ``pack_dgrad_weight(w, bfloat16)`` per tensor.  The destination buffers and the device-side item table are allocated
    once; ``run()`` is what a training step calls after the optimizer moved the master weights."""

    def __init__(self, weights_krsc, want_dgrad=True, dtype=BF16):
        """``dtype=torch.float32`` (round 5, ``rs_weight_prep_f32``): the fp32 training step's data-gradient layouts only -- the
        fp32 KRSC master is its own compute copy, so ``cast`` stays empty."""

        assert weights_krsc and all(w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 4 for w in weights_krsc)
        assert dtype == BF16 or want_dgrad
        dev = weights_krsc[0].device
        self.dtype = dtype
        self.weights = list(weights_krsc)
        self.cast = [torch.empty(w.shape, device=dev, dtype=BF16) if dtype == BF16 else None for w in self.weights]
        self.dgrad = [torch.empty((w.shape[3], w.shape[1], w.shape[2], w.shape[0]), device=dev, dtype=dtype) if want_dgrad else None
                      for w in self.weights]
        items = (_WPrepItem * len(self.weights))()
        tiles = 0
        for i, w in enumerate(self.weights):
            cout, kh, kw, cin = w.shape
            items[i] = _WPrepItem(_dev(w, "w").value, _dev(self.cast[i], "cast", BF16).value if dtype == BF16 else None,
                                  _dev(self.dgrad[i], "dgrad", dtype).value if want_dgrad else None, cout, kh * kw, cin, tiles)
            tiles += kh * kw * ((cin + 31) // 32) * ((cout + 31) // 32)
        self.tiles = tiles
        self.table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
        self.ptrs = tuple(w.data_ptr() for w in self.weights)

    def run(self):
        _call("rs_weight_prep_bf16" if self.dtype == BF16 else "rs_weight_prep_f32", _dev(self.table, "items", torch.uint8),
              len(self.weights), self.tiles, _stream())


def pack_stem_weight(w_krsc, dtype=torch.float32):
    """fp32 [Cout,kh,kw<=8,Cin<=4] -> [Cout,kh,8,4] (zero padded) in ``dtype``."""

    cout, kh, kw, cin = w_krsc.shape
    out = torch.empty((cout, kh, 8, 4), device=w_krsc.device, dtype=dtype)
    _call("rs_pack_stem_weight_bf16" if dtype == BF16 else "rs_pack_stem_weight", _dev(w_krsc, "w"), _dev(out, "out", dtype), cout, kh, kw,
          cin, _stream())
    return out


def nchw_to_nhwc4(x, dtype=torch.float32):
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, 4), device=x.device, dtype=dtype)
    _call("rs_nchw_to_nhwc4_bf16" if dtype == BF16 else "rs_nchw_to_nhwc4", _dev(x, "x"), _dev(out, "out", dtype), n, c, h, w, _stream())
    return out


def stem_conv_bf16(x4, w_packed, scale=None, shift=None, relu=False):
    """resnet.conv1 (7x7/2, pad 3) on NHWC4 bf16 input with packed bf16 weights [64,7,8,4] -> [N,H/2,W/2,64] bf16."""

    n, h, w, _ = x4.shape
    out = torch.empty((n, h // 2, w // 2, 64), device=x4.device, dtype=BF16)
    ev = _start()
    _call("rs_stem_conv_fwd_bf16", _dev(x4, "x4", BF16), _dev(w_packed, "w", BF16), _dev(scale, "scale"), _dev(shift, "shift"),
          _dev(out, "out", BF16), n, h, w, int(relu), _stream())
    if ev:
        _stop(ev)
        flops = 2.0 * n * 64 * 3 * 49 * (h // 2) * (w // 2)
        _record(ev, "stem_conv_bf16", flops, (3, 64, 7, 2, 0, h // 2, w // 2), 2 * (x4.numel() + out.numel()))
    return out


def wgrad_kernel_name(d, form=None):
    """The bf16 weight-gradient kernel ``rs_conv2d_wgrad_bf16`` launches for ``d``, named like its instantiation (rocprofv3
    shows ``conv_wgrad_bf16<128, 128, 2, 2, 64, false>`` for ``conv_wgrad_bf16<128x128>``; ``phase`` = the last flag)."""

    lib = _lib.lib()
    if form is None:
        form = lib.rs_conv2d_wgrad_bf16_form(ctypes.byref(d))
    if form == 1:  # all-taps kernel: instantiated per input-channel slab (32 / 64 / 128) and for the fused x2 upsample
        return "conv_wgrad_thin_bf16<{}{}>".format(min(d.C1, 128), ",ups" if d.ups else "")
    t = lib.rs_conv2d_wgrad_bf16_tile(ctypes.byref(d))
    if t <= 0:
        raise ValueError("rs_conv2d_wgrad_bf16_tile: invalid arguments")
    tile = "{}x{}".format(t >> 16, t & 255) + ("+{}x{}".format(t >> 16, (t >> 8) & 255) if (t >> 8) & 255 else "")
    # phase form: its 128 x 128 launch is conv_wgrad_phase4_bf16 (one dz plane x four source offsets per block) unless knob wgrad_phase4 = 0
    phase = "" if form != 2 else ("phase4," if (t >> 16, t & 255) == (128, 128) and get_knob("wgrad_phase4") else "phase,")
    return "conv_wgrad_bf16<{}{}>".format(phase, tile)


def stem_conv_wgrad_bf16(dy, x4):
    """Packed fp32 gradient [64,7,8,4] of the stem filter from bf16 dy [N,H/2,W/2,64] and the NHWC4 bf16 input."""

    n, h, w, _ = x4.shape
    lib = _lib.lib()
    dw = torch.empty((64, 7, 8, 4), device=dy.device, dtype=torch.float32)
    ev = _start()
    _call("rs_stem_conv_wgrad_bf16", _dev(dy, "dy", BF16), _dev(x4, "x4", BF16), _dev(dw, "dw"), n, h, w,
          _workspace(lib.rs_stem_conv_wgrad_bf16_workspace_bytes(n, h, w), dy.device), _stream())
    if ev:
        _stop(ev)
        flops = 2.0 * n * 64 * 3 * 49 * (h // 2) * (w // 2)
        _record(ev, "stem_wgrad_bf16", flops, (3, 64, 7, 2, 0, h // 2, w // 2), 2 * (x4.numel() + dy.numel()))
    return dw


def u8_to_nhwc4_norm(img, mean, std):
    """uint8 HWC tiles [N,H,W,C] -> normalised NHWC4 fp32: ToTensor + Normalize (tools/predict.py:71) on the device."""

    n, h, w, c = img.shape
    assert len(mean) == c and len(std) == c
    out = torch.empty((n, h, w, 4), device=img.device, dtype=torch.float32)
    fm, fs = (ctypes.c_float * c)(*mean), (ctypes.c_float * c)(*std)
    _call("rs_u8_to_nhwc4_norm", _dev(img, "img", torch.uint8), _dev(out, "out"), fm, fs, n, h, w, c, _stream())
    return out


_ANCHORS = {}


def _anchors(device):
    import numpy as np

    anchors = _ANCHORS.get(device)
    if anchors is None:
        anchors = torch.from_numpy(np.linspace(0, 1, 256)).to(device)  # numpy's own float64 anchors
        _ANCHORS[device] = anchors
    return anchors


def final_conv1x1_quantize(x, w, bias, overlap):
    """self.final + softmax + crop of the `overlap` border + np.digitize(p_c, linspace(0,1,256)).astype(uint8) of every
    non-background class (tools/predict.py:87,96-103) in one kernel: uint8 [N, H-2*overlap, W-2*overlap] for a binary
    model (the reference's case, byte for byte), [N, H', W', C-1] for C > 2 classes."""

    n, h, wd, cin = x.shape
    c = w.shape[0]
    shape = (n, h - 2 * overlap, wd - 2 * overlap) + ((c - 1,) if c > 2 else ())
    out = torch.empty(shape, device=x.device, dtype=torch.uint8)
    _call("rs_final_conv1x1_quantize_dt", _dev(x, "x", x.dtype), _dt(x), _dev(w, "w"), _dev(bias, "bias"),
          _dev(_anchors(x.device), "anchors", torch.float64), _dev(out, "out", torch.uint8), n, h, wd, cin, c, overlap, _stream())
    return out


def final_conv1x1_argmax(x, w, bias):
    """self.final + argmax over the classes: uint8 [N,H,W] class indices (tools/serve.py:160-164)."""

    n, h, wd, cin = x.shape
    out = torch.empty((n, h, wd), device=x.device, dtype=torch.uint8)
    _call("rs_final_conv1x1_argmax_dt", _dev(x, "x", x.dtype), _dt(x), _dev(w, "w"), _dev(bias, "bias"), _dev(out, "out", torch.uint8), n,
          h, wd, cin, w.shape[0], _stream())
    return out


# dihedral test-time augmentation (csrc/tta.hip): ops in the encoding of augment_tiles, op = f + 2*k (FLIP_LEFT_RIGHT when f,
# then k counter-clockwise rot90s).  Every mode is a group, which makes the sorted merge exactly equivariant.
TTA_MODES = {"none": (0,), "hflip": (0, 1), "flips": (0, 1, 4, 5), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def tta_ops(mode, h, w):
    """The op list of a TTA mode for h x w tiles; ValueError on an unknown mode or on ``d4`` (90-degree turns) off the square."""

    if mode not in TTA_MODES:
        raise ValueError("unknown TTA mode {!r}: one of {}".format(mode, ", ".join(TTA_MODES)))
    op_list = list(TTA_MODES[mode])
    if h != w and any((op >> 1) & 1 for op in op_list):
        raise ValueError("TTA mode {!r} rotates by 90 degrees and needs square tiles, got {}x{}".format(mode, h, w))
    return op_list


def _tta_fan_out(x, kind, mean, std, op_list, dtype, n, h, w, c):
    v = len(op_list)
    out = torch.empty((n * v, h, w, 4), device=x.device, dtype=dtype)
    fm = fs = None
    if mean is not None:
        assert len(mean) == c and len(std) == c
        fm, fs = (ctypes.c_float * c)(*mean), (ctypes.c_float * c)(*std)
    _call("rs_tta_fan_out", _dev(x, "x", x.dtype), kind, fm, fs, _dev(out, "out", dtype), _dt(dtype), (ctypes.c_int * v)(*op_list), v, n, h,
          w, c, _stream())
    return out


def tta_fan_out_u8(img, mean, std, op_list, dtype=torch.float32):
    """uint8 HWC tiles [N,H,W,C] -> the views' normalised NHWC4 [N*V,H,W,4] in ``dtype``: view v of tile n (batch index
    n*V + v) is ``u8_to_nhwc4_norm`` of the tile transformed by op_list[v], bit for bit."""

    n, h, w, c = img.shape
    return _tta_fan_out(img, _lib.RS_TTA_IN_U8, mean, std, op_list, dtype, n, h, w, c)


def tta_fan_out_f32(x, op_list, dtype=torch.float32):
    """fp32 NCHW images [N,C,H,W] -> the views' NHWC4 [N*V,H,W,4] in ``dtype`` (``nchw_to_nhwc4`` of each transformed image)."""

    n, c, h, w = x.shape
    return _tta_fan_out(x, _lib.RS_TTA_IN_F32, None, None, op_list, dtype, n, h, w, c)


def tta_merge(probs, op_list, mode="probs", overlap=0):
    """The views' fp32 probabilities [N*V,C,H,W] -> per pixel and class the sorted fp32 sum of the V view values times 1/V, then
    by ``mode``: "probs" -> fp32 [N,C,H,W]; "quantize" -> the bytes of ``final_conv1x1_quantize`` (crop of ``overlap``);
    "argmax" -> uint8 [N,H,W], the first maximum of the merged probabilities."""

    nv, c, h, w = probs.shape
    v = len(op_list)
    assert nv % v == 0
    n = nv // v
    m = {"probs": _lib.RS_TTA_PROBS, "quantize": _lib.RS_TTA_QUANTIZE, "argmax": _lib.RS_TTA_ARGMAX}[mode]
    anchors = None
    if m == _lib.RS_TTA_PROBS:
        out = torch.empty((n, c, h, w), device=probs.device, dtype=torch.float32)
    elif m == _lib.RS_TTA_QUANTIZE:
        out = torch.empty((n, h - 2 * overlap, w - 2 * overlap) + ((c - 1,) if c > 2 else ()), device=probs.device, dtype=torch.uint8)
        anchors = _dev(_anchors(probs.device), "anchors", torch.float64)
    else:
        out = torch.empty((n, h, w), device=probs.device, dtype=torch.uint8)
    _call("rs_tta_merge", _dev(probs, "probs"), (ctypes.c_int * v)(*op_list), v, m, anchors, int(overlap), _dev(out, "out", out.dtype), n,
          c, h, w, _stream())
    return out


def maxpool2d(x, k, stride, pad, want_argmax=False, out_dtype=None):
    """``out_dtype`` (default: x.dtype): torch.bfloat16 on an fp32 input is the precision boundary of the bf16 path."""

    n, h, w, c = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    out = torch.empty((n, ho, wo, c), device=x.device, dtype=out_dtype or x.dtype)
    amax = torch.empty((n, ho, wo, c), device=x.device, dtype=torch.uint8) if want_argmax else None
    _call("rs_maxpool2d_fwd_dt", _dev(x, "x", x.dtype), _dt(x), _dev(out, "out", out.dtype), _dt(out), _dev(amax, "argmax", torch.uint8), n,
          h, w, c, k, stride, pad, ho, wo, _stream())
    return (out, amax) if want_argmax else out


def bn_fold(gamma, beta, mean, var, eps):
    c = gamma.numel()
    scale = torch.empty(c, device=gamma.device, dtype=torch.float32)
    shift = torch.empty(c, device=gamma.device, dtype=torch.float32)
    _call("rs_bn_fold", _dev(gamma, "gamma"), _dev(beta, "beta"), _dev(mean, "mean"), _dev(var, "var"), ctypes.c_float(eps),
          _dev(scale, "scale"), _dev(shift, "shift"), c, _stream())
    return scale, shift


def final_conv1x1(x, w, bias, softmax=False):
    """x [N,H,W,Cin] NHWC, w [C,Cin] -> NCHW [N,C,H,W] logits (or probabilities if ``softmax``)."""

    n, h, wd, cin = x.shape
    c = w.shape[0]
    out = torch.empty((n, c, h, wd), device=x.device, dtype=torch.float32)
    _call("rs_final_conv1x1_dt", _dev(x, "x", x.dtype), _dt(x), _dev(w, "w"), _dev(bias, "bias"), _dev(out, "out"), n, h, wd, cin, c,
          int(softmax), _stream())
    return out


# ------------------------------------------------------------------------------------------------------------------
# training path
# ------------------------------------------------------------------------------------------------------------------

_WORKSPACE = {}


def _workspace(nbytes, device):
    """A scratch buffer per (device, stream), grown on demand: users on one stream serialise; the weight-gradient side
    stream of the backward pass (robosat_amd.autograd) gets its own."""

    if nbytes < 0:
        raise ValueError("workspace query failed (RS_EINVAL)")
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _WORKSPACE.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), device=device, dtype=torch.uint8)
        _WORKSPACE[key] = ws
    return ctypes.c_void_p(ws.data_ptr())


def pack_dgrad_weight(w_krsc, dtype=torch.float32):
    """fp32 [Cout,kh,kw,Cin] -> [Cin,kh,kw,Cout] in ``dtype``, taps flipped (weights of the data-gradient convolution)."""

    cout, kh, kw, cin = w_krsc.shape
    out = torch.empty((cin, kh, kw, cout), device=w_krsc.device, dtype=dtype)
    _call("rs_pack_dgrad_weight_bf16" if dtype == BF16 else "rs_pack_dgrad_weight", _dev(w_krsc, "w"), _dev(out, "out", dtype), cout, kh,
          kw, cin, _stream())
    return out


def unpack_stem_weight(packed, kw, cin, out=None):
    cout, kh = packed.shape[:2]
    if out is None:
        out = torch.empty((cout, kh, kw, cin), device=packed.device, dtype=torch.float32)
    assert tuple(out.shape) == (cout, kh, kw, cin)
    _call("rs_unpack_stem_weight", _dev(packed, "packed"), _dev(out, "out"), cout, kh, kw, cin, _stream())
    return out


def conv2d_wgrad(dy, src1, kh, kw, src2=None, ups=0, stride=1, pad=0, stem=0, out=None):
    """``rs_conv2d_wgrad``: KRSC filter gradient [Cout,kh,kw,Cin] (packed [Cout,kh,8,4] for the stem)."""

    n, ho, wo, cout = dy.shape
    _, hs, ws, c1 = src1.shape
    c2 = 0 if src2 is None else src2.shape[3]
    d = ConvDesc(n, hs, ws, c1, c2, ups, kh, kw, stride, pad, ho, wo, cout, 0, int(bool(stem)))
    lib = _lib.lib()
    act = dy.dtype
    bf = act == BF16
    shape = (cout, kh, 8, 4) if stem else (cout, kh, kw, c1 + c2)
    dw = out if out is not None else torch.empty(shape, device=dy.device, dtype=torch.float32)
    assert tuple(dw.shape) == shape
    wsb = (lib.rs_conv2d_wgrad_bf16_workspace_bytes if bf else lib.rs_conv2d_wgrad_workspace_bytes)(ctypes.byref(d))
    ev = _start()
    _call("rs_conv2d_wgrad_bf16" if bf else "rs_conv2d_wgrad", ctypes.byref(d), _dev(dy, "dy", act), _dev(src1, "src1", act),
          _dev(src2, "src2", act), _dev(dw, "dw"), _workspace(wsb, dy.device), _stream())
    if ev:
        _stop(ev)
        nbytes = _esize(act) * (d.N * d.Ho * d.Wo * d.Cout + d.N * d.Hs * d.Ws * (4 if stem else d.C1 + d.C2)) + 4 * dw.numel()
        form = lib.rs_conv2d_wgrad_bf16_form(ctypes.byref(d)) if bf else 0
        if not bf and not stem:
            # conv_wgrad.hip: 2 = the fp32 phase form of DecoderBlock (16 / 36 of the MACs), 3 = that in the Winograd domain (9 / 36),
            # 4 = a stride-1 3x3 convolution in the Winograd domain of F(2x2, 3x3) (16 / 36)
            form = lib.rs_conv2d_wgrad_form(ctypes.byref(d))
        # fp32: the LDS-DMA kernel (conv_wgrad_f32_dma.hip) for everything but the packed stem, unless knob wgrad_f32_dma = 0
        name = wgrad_kernel_name(d, form) if bf else ("conv_wgrad_f32" if stem or get_knob("wgrad_f32_dma") == 0 else
                                                      "conv_wgrad_wino_f32" if form == 3 else "conv_wgrad_wino33_f32" if form == 4 else
                                                      "conv_wgrad_f32_dma")
        _record(ev, name, conv_flops(d), _shape(d), nbytes, conv_flops(d) * (0.25 if form == 3 else 4.0 / 9.0 if form in (2, 4) else 1.0))
    return dw


def _bn_ws(m, c, device):
    return _workspace(_lib.lib().rs_bn_workspace_bytes(m, c) + 3 * c * 4, device)


def bn_train_stats(y, gamma, beta, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None):
    """Batch statistics of y [N,H,W,C]; returns (mean, invstd, scale, shift) and updates the running buffers."""

    c = y.shape[-1]
    m = y.numel() // c
    mean, invstd, scale, shift = (torch.empty(c, device=y.device, dtype=torch.float32) for _ in range(4))
    _call("rs_bn_train_stats_dt", _dev(y, "y", y.dtype), _dt(y), m, c, ctypes.c_float(eps), ctypes.c_float(momentum), _dev(gamma, "gamma"),
          _dev(beta, "beta"), _dev(mean, "mean"), _dev(invstd, "invstd"), _dev(scale, "scale"), _dev(shift, "shift"),
          _dev(running_mean, "running_mean"), _dev(running_var, "running_var"),
          _dev(num_batches_tracked, "num_batches_tracked", torch.int64), _bn_ws(m, c, y.device), _stream())
    return mean, invstd, scale, shift


def bn_bits_ok(c):
    """Channel counts for which ``bn_apply(..., want_bits=True)`` is available (the streaming form: C divides 2048)."""

    return 8 <= c <= 2048 and 2048 % c == 0


def bn_apply(y, scale, shift, residual=None, relu=False, want_bits=False):
    """z = relu?(y * scale + shift (+ residual)).  ``want_bits``: returns (z, bits) with the ReLU mask of z as one bit per
    element (uint8 [numel/8]; bit e of byte i: element 8*i + e is > 0) for ``conv2d_dgrad_bnstats(relu_mask_bits=...)``."""

    c = y.shape[-1]
    out = torch.empty_like(y)
    bits = torch.empty(y.numel() // 8, device=y.device, dtype=torch.uint8) if want_bits else None
    _call("rs_bn_apply_bits_dt", _dev(y, "y", y.dtype), _dev(scale, "scale"), _dev(shift, "shift"), _dev(residual, "residual", y.dtype),
          _dev(out, "out", y.dtype), _dev(bits, "bits", torch.uint8), _dt(y), y.numel() // c, c, int(relu), _stream())
    return (out, bits) if want_bits else out


def bn_bwd(dz, zmask, y, mean, invstd, gamma, want_masked=False, dgamma=None, dbeta=None):
    """Returns (dy, dgamma, dbeta[, dmasked])."""

    c = y.shape[-1]
    m = y.numel() // c
    dy = torch.empty_like(y)
    dmasked = torch.empty_like(y) if want_masked else None
    if dgamma is None:
        dgamma = torch.empty(c, device=y.device, dtype=torch.float32)
    if dbeta is None:
        dbeta = torch.empty(c, device=y.device, dtype=torch.float32)
    t = y.dtype
    _call("rs_bn_bwd_dt", _dev(dz, "dz", t), _dev(zmask, "zmask", t), _dev(y, "y", t), _dev(mean, "mean"), _dev(invstd, "invstd"),
          _dev(gamma, "gamma"), _dev(dy, "dy", t), _dev(dmasked, "dmasked", t), _dev(dgamma, "dgamma"), _dev(dbeta, "dbeta"), _dt(y), m, c,
          _bn_ws(m, c, y.device), _stream())
    return (dy, dgamma, dbeta, dmasked) if want_masked else (dy, dgamma, dbeta)


def scatter_add_stride2(t, out):
    """``out[:, ::2, ::2, :] += t`` in place (``rs_scatter_add_stride2_dt``): the data gradient of a 1x1 / stride-2 convolution is its
    transposed product on the low-resolution grid (``t``), landing on the even positions of the input grid."""

    n, hs, ws, c = t.shape
    assert out.shape[0] == n and out.shape[3] == c and out.dtype == t.dtype and out.is_contiguous()
    _call("rs_scatter_add_stride2_dt", _dev(t, "t", t.dtype), _dev(out, "out", t.dtype), _dt(t), n, hs, ws, out.shape[1], out.shape[2], c,
          _stream())
    return out


def maxpool2d_bwd(dy, argmax, in_shape, k, stride, pad, out=None, out_dtype=None):
    """Gradient wrt the pooling input [N,H,W,C]; ``out`` given => accumulate into it.  ``out_dtype`` fp32 on a bf16 dy
    is the precision boundary of the bf16 path (stem pool)."""

    n, h, w, c = in_shape
    ho, wo = dy.shape[1:3]
    acc = out is not None
    if out is None:
        out = torch.empty(in_shape, device=dy.device, dtype=out_dtype or dy.dtype)
    _call("rs_maxpool2d_bwd_dt", _dev(dy, "dy", dy.dtype), _dt(dy), _dev(argmax, "argmax", torch.uint8), _dev(out, "dx", out.dtype),
          _dt(out), n, h, w, c, k, stride, pad, ho, wo, int(acc), _stream())
    return out


def upsample2x_bwd(dup, c1, c2=0, mask1=None, mask2=None, out1=None):
    """dup [N,2H,2W,C1+C2] -> (d1 [N,H,W,C1], d2 [N,H,W,C2] or None); ``out1`` given => accumulate into it."""

    n, h2, w2, ct = dup.shape
    assert ct == c1 + c2 and h2 % 2 == 0 and w2 % 2 == 0
    h, w = h2 // 2, w2 // 2
    acc = out1 is not None
    t = dup.dtype
    d1 = out1 if acc else torch.empty((n, h, w, c1), device=dup.device, dtype=t)
    d2 = torch.empty((n, h, w, c2), device=dup.device, dtype=t) if c2 else None
    _call("rs_upsample2x_bwd_dt", _dev(dup, "dup", t), _dev(d1, "d1", t), _dev(d2, "d2", t), _dev(mask1, "mask1", t),
          _dev(mask2, "mask2", t), _dt(dup), n, h, w, c1, c2, int(acc), _stream())
    return d1, d2


def final_conv1x1_bwd(x, w, dlogits, relu_mask=True, dw=None, db=None):
    """x [N,H,W,Cin] NHWC, w [C,Cin], dlogits NCHW -> (dx NHWC, dw [C,Cin], db [C])."""

    n, h, wd, cin = x.shape
    c = w.shape[0]
    lib = _lib.lib()
    dx = torch.empty_like(x)
    if dw is None:
        dw = torch.empty((c, cin), device=x.device, dtype=torch.float32)
    if db is None:
        db = torch.empty(c, device=x.device, dtype=torch.float32)
    ws = _workspace(lib.rs_final_conv1x1_bwd_workspace_bytes(cin, c), x.device)
    _call("rs_final_conv1x1_bwd_dt", _dev(x, "x", x.dtype), _dev(w, "w"), _dev(dlogits, "dlogits"), _dev(dx, "dx", x.dtype), _dev(dw, "dw"),
          _dev(db, "db"), _dt(x), n, h, wd, cin, c, int(relu_mask), ws, _stream())
    return dx, dw, db


# ------------------------------------------------------------------------------------------------------------------
# losses / metrics (NCHW logits, int64 targets)
# ------------------------------------------------------------------------------------------------------------------

NLL_CROSS_ENTROPY, NLL_FOCAL = 0, 1


def _ignore_label(ignore, classes):
    """The ``ignore`` argument of the losses and counts below as the C ABI's int: ``None`` stays ``None`` (the entry points without
    ``_ig``), an integer must be no class of 0 .. ``classes`` - 1 and fit the label byte."""

    if ignore is None:
        return None
    if isinstance(ignore, bool) or int(ignore) != ignore or not classes <= int(ignore) <= 255:
        raise ValueError("robosat_amd: the ignore label is an integer in {}..255 for {} classes, got {!r}".format(classes, classes, ignore))
    return int(ignore)


BOUNDARY_MAX_REACH = 128
_BOUNDARY_TABLES = {}


def boundary_reach(w0, sigma):
    """R = ceil(3 * sigma), the reach in pixels of the boundary weight ``1 + w0 * exp(-d^2 / (2 sigma^2))`` (include/robosat_hip.h);
    raises ``ValueError`` unless both are finite numbers > 0 and 1 <= R <= 128."""

    import math

    for name, value in (("w0", w0), ("sigma", sigma)):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not value > 0:
            raise ValueError("robosat_amd: the boundary weight's {} is a finite number > 0, got {!r}".format(name, value))
    reach = int(math.ceil(3.0 * float(sigma)))
    if not 1 <= reach <= BOUNDARY_MAX_REACH:
        raise ValueError("robosat_amd: the boundary weight reaches ceil(3 * sigma) = {} pixels, more than {}".format(reach, BOUNDARY_MAX_REACH))
    return reach


def boundary_table(w0, sigma):
    """float32 numpy [R * R]: ``table[k] = float32(1 + w0 * exp(-k / (2 sigma^2)))``, made in float64 and rounded once."""

    import numpy as np

    reach = boundary_reach(w0, sigma)
    k = np.arange(reach * reach, dtype=np.float64)
    return (1.0 + float(w0) * np.exp(-k / (2.0 * float(sigma) * float(sigma)))).astype(np.float32)


def _boundary_table_on(w0, sigma, device):
    """The table on ``device``, cached per (w0, sigma, device): made and uploaded once, before any capture that uses it."""

    key = (float(w0), float(sigma), str(device))
    table = _BOUNDARY_TABLES.get(key)
    if table is None:
        table = torch.from_numpy(boundary_table(w0, sigma)).to(device)
        _BOUNDARY_TABLES[key] = table
    return table


def boundary_weight_plane(targets, w0, sigma, ignore=None, classes=None):
    """int64 [N, H, W] labels -> float32 [N, H, W]: the boundary weight plane of ``rs_boundary_weight_plane``
    (include/robosat_hip.h): ``table[d2]`` within ``ceil(3 sigma)`` pixels of a label boundary, exactly 1 beyond, exactly 0 at a pixel
    whose label is ``ignore``.  ``classes`` (the logits' class count) lets ``ignore`` be checked against it here; without it the
    loss call does that."""

    n, h, w = targets.shape
    reach = boundary_reach(w0, sigma)
    c = 1 if classes is None else int(classes)
    ignore = _ignore_label(ignore, c)
    tgt = _dev(targets, "targets", torch.int64)  # (a CPU tensor raises before anything is loaded or sized)
    lib = _lib.lib()
    table = _boundary_table_on(w0, sigma, targets.device)
    plane = torch.empty((n, h, w), device=targets.device, dtype=torch.float32)
    _call("rs_boundary_weight_plane", tgt, _dev(table, "table"), _dev(plane, "plane"), n, c, h, w, reach, -1 if ignore is None else ignore,
          _workspace(lib.rs_boundary_weight_plane_workspace_bytes(n, h, w), targets.device), _stream())
    return plane


SEPARATION_MAX_REACH = 32
_SEPARATION_TABLES = {}


def separation_reach(ws, sigma):
    """D = ceil(3 * sigma), the reach in pixels of the separation weight ``ws * exp(-(d1 + d2)^2 / (2 sigma^2))``
    (include/robosat_hip.h); raises ``ValueError`` unless both are finite numbers > 0 and 1 <= D <= 32."""

    import math

    for name, value in (("ws", ws), ("sigma", sigma)):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not value > 0:
            raise ValueError("robosat_amd: the separation weight's {} is a finite number > 0, got {!r}".format(name, value))
    reach = int(math.ceil(3.0 * float(sigma)))
    if not 1 <= reach <= SEPARATION_MAX_REACH:
        raise ValueError("robosat_amd: the separation weight reaches ceil(3 * sigma) = {} pixels, more than {}".format(
            reach, SEPARATION_MAX_REACH))
    return reach


def separation_table(ws, sigma):
    """float32 numpy [D * D]: ``table[k] = float32(ws * exp(-k / (2 sigma^2)))``, made in float64 and rounded once."""

    import numpy as np

    reach = separation_reach(ws, sigma)
    k = np.arange(reach * reach, dtype=np.float64)
    return (float(ws) * np.exp(-k / (2.0 * float(sigma) * float(sigma)))).astype(np.float32)


def _separation_table_on(ws, sigma, device):
    """The table on ``device``, cached per (ws, sigma, device): made and uploaded once, before any capture that uses it."""

    key = (float(ws), float(sigma), str(device))
    table = _SEPARATION_TABLES.get(key)
    if table is None:
        table = torch.from_numpy(separation_table(ws, sigma)).to(device)
        _SEPARATION_TABLES[key] = table
    return table


def separation_weight_plane(targets, ws, sigma, ignore=None, classes=None, base=None, check=False):
    """int64 [N, H, W] labels -> float32 [N, H, W]: ``base`` plus the separation term of ``rs_separation_weight_plane``
    (include/robosat_hip.h): ``table[s2]`` at a background pixel whose two nearest objects are within reach, s2 = a + b + isqrt(4ab)
    of their squared distances, nothing elsewhere.  Objects are the 4-connected components of the valid pixels of the classes
    1 .. ``classes`` - 1 (without ``classes``: of every valid non-zero label).  ``base`` float32 [N, H, W] on the labels' device (the
    boundary weight plane, say); without it the base is 1 at a valid pixel and 0 at an ignored one.  ``check`` reads the labelling's
    error word back after the call and raises if it is set: a host synchronisation, so never inside a captured step."""

    n, h, w = targets.shape
    reach = separation_reach(ws, sigma)
    if classes is None:
        ignore, c = _ignore_label(ignore, 1), 256
    else:
        c = int(classes)
        if not 1 <= c <= 256:
            raise ValueError("robosat_amd: the separation weight takes 1..256 classes, got {!r}".format(classes))
        ignore = _ignore_label(ignore, c)
    tgt = _dev(targets, "targets", torch.int64)  # (a CPU tensor raises before anything is loaded or sized)
    if base is not None:
        if not isinstance(base, torch.Tensor) or tuple(base.shape) != (n, h, w) or base.dtype != torch.float32 or base.device != targets.device:
            raise ValueError("robosat_amd: the separation weight's base is float32 [N, H, W] = {} on {}, got {}".format(
                (n, h, w), targets.device, "{} {} on {}".format(base.dtype, tuple(base.shape), base.device)
                if isinstance(base, torch.Tensor) else repr(base)))
    lib = _lib.lib()
    nbytes = lib.rs_separation_weight_plane_workspace_bytes(n, h, w)
    table = _separation_table_on(ws, sigma, targets.device)
    plane = torch.empty((n, h, w), device=targets.device, dtype=torch.float32)
    workspace = _workspace(nbytes, targets.device)
    _call("rs_separation_weight_plane", tgt, _dev(table, "table"), _dev(base, "base"), _dev(plane, "plane"), n, c, h, w, reach,
          -1 if ignore is None else ignore, workspace, _stream())
    if check:
        err = _WORKSPACE[(targets.device, torch.cuda.current_stream().cuda_stream)][:4].view(torch.int32)
        if int(err.item()):
            raise RuntimeError("rs_separation_weight_plane: a union-find loop of the labelling ran out of its H*W bound (code {})".format(
                int(err.item())))
    return plane


RELAX_MAX_RADIUS = 16


def relax_radius(radius):
    """The relaxation radius R of ``rs_label_set_plane`` as an int; raises ``ValueError`` unless it is an integer (no bool, no float)
    in 1..16."""

    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= RELAX_MAX_RADIUS:
        raise ValueError("robosat_amd: the relaxation radius is an integer in 1..{} pixels, got {!r}".format(RELAX_MAX_RADIUS, radius))
    return radius


def label_set_plane(targets, radius, ignore=None, classes=None):
    """int64 [N, H, W] labels -> uint8 [N, H, W]: the label set plane of ``rs_label_set_plane`` (include/robosat_hip.h): bit c of a
    valid pixel's byte says that class c occurs among the valid pixels of its image within ``radius`` pixels in x and in y; 0 at a
    pixel whose label is ``ignore``.  ``classes`` (the logits' class count) lets ``ignore`` be checked against it here; without it the
    loss call does that."""

    n, h, w = targets.shape
    radius = relax_radius(radius)
    c = 1 if classes is None else int(classes)
    ignore = _ignore_label(ignore, c)
    tgt = _dev(targets, "targets", torch.int64)  # (a CPU tensor raises before anything is loaded or sized)
    sets = torch.empty((n, h, w), device=targets.device, dtype=torch.uint8)
    _call("rs_label_set_plane", tgt, _dev(sets, "sets", torch.uint8), n, c, h, w, radius, -1 if ignore is None else ignore, _stream())
    return sets


HARD_NO_CAP = 0xFFFFFFFF


def hard_fraction(fraction):
    """``fraction`` of the hard-pixel selection as a float: a finite number in (0, 1], else ``ValueError``."""

    import math

    if isinstance(fraction, bool) or not isinstance(fraction, (int, float)) or not math.isfinite(fraction) or not 0 < fraction <= 1:
        raise ValueError("robosat_amd: the hard-pixel fraction is a finite number in (0, 1], got {!r}".format(fraction))
    return float(fraction)


def hard_cap(below):
    """The cap on the hard-pixel threshold for the probability bound ``below`` in (0, 1): the bits of ``float32(-ln below)``, made in
    float64 and rounded once (include/robosat_hip.h).  A pixel whose true class has a probability below ``below`` has a key above
    the cap and is always kept."""

    import math
    import struct

    if isinstance(below, bool) or not isinstance(below, (int, float)) or not 0 < below < 1:  # (NaN fails both comparisons)
        raise ValueError("robosat_amd: the hard-pixel probability bound is a number in (0, 1), got {!r}".format(below))
    return struct.unpack("<I", struct.pack("<f", -math.log(float(below))))[0]


def hard_fraction_bits(fraction):
    """The checked ``fraction`` as the C ABI takes it: the 64 bits of the double in an integer (``fraction_bits``)."""

    import struct

    return struct.unpack("<q", struct.pack("<d", hard_fraction(fraction)))[0]


def _hard_args(shape, fraction, below, ignore, classes, base, device):
    """What the two hard-pixel wrappers share: the checked scalars as the C ABI takes them and the outputs."""

    n, h, w = shape
    fraction = hard_fraction_bits(fraction)
    cap = HARD_NO_CAP if below is None else hard_cap(below)
    ignore = _ignore_label(ignore, classes)
    if base is not None:
        assert tuple(base.shape) == (n, h, w), "base is [N, H, W]"
    plane = torch.empty((n, h, w), device=device, dtype=torch.float32)
    info = torch.empty((n, 4), device=device, dtype=torch.int64)
    return fraction, cap, -1 if ignore is None else ignore, plane, info


def hard_pixel_plane(logits, targets, fraction, below=None, ignore=None, base=None, want_keys=False):
    """float32 [N, C, H, W] logits, int64 [N, H, W] labels -> ``(plane, info)`` of ``rs_hard_pixel_plane`` (include/robosat_hip.h):
    per image the valid pixels whose cross-entropy is among the ``ceil(fraction * V)`` largest (ties kept), or above ``-ln below``,
    get ``base`` (float32 [N, H, W]; 1.0 without one) in the float32 [N, H, W] ``plane``, every other pixel +0.0; ``info`` int64
    [N, 4] = (valid pixels, k, threshold key, kept pixels).  ``want_keys`` adds the key plane: int32 [N, H, W] that holds the
    uint32 bits."""

    n, c, h, w = logits.shape
    x, tgt = _dev(logits, "logits"), _dev(targets, "targets", torch.int64)  # (a CPU tensor raises before anything is loaded or sized)
    assert tuple(targets.shape) == (n, h, w), "targets is [N, H, W]"
    fraction, cap, ignore, plane, info = _hard_args((n, h, w), fraction, below, ignore, c, base, logits.device)
    keys = torch.empty((n, h, w), device=logits.device, dtype=torch.int32) if want_keys else None
    lib = _lib.lib()
    _call("rs_hard_pixel_plane", x, tgt, _dev(base, "base"), _dev(plane, "plane"), _dev(keys, "keys", torch.int32),
          _dev(info, "info", torch.int64), n, c, h, w, fraction, cap, ignore,
          _workspace(lib.rs_hard_pixel_workspace_bytes(n, h, w), logits.device), _stream())
    return (plane, info, keys) if want_keys else (plane, info)


def hard_pixel_select(keys, fraction, below=None, targets=None, ignore=None, base=None):
    """``rs_hard_pixel_select``: the selection of ``hard_pixel_plane`` on a key plane of the caller's, int32 [N, H, W] that holds
    any uint32 bits -> ``(plane, info)``.  ``targets`` is needed with ``ignore`` (any label byte here: there is no class count)."""

    n, h, w = keys.shape
    k = _dev(keys, "keys", torch.int32)
    if (ignore is None) != (targets is None):
        raise ValueError("robosat_amd: hard_pixel_select takes targets and ignore together")
    if targets is not None:
        assert tuple(targets.shape) == (n, h, w), "targets is [N, H, W]"
    fraction, cap, ignore, plane, info = _hard_args((n, h, w), fraction, below, ignore, 0, base, keys.device)
    lib = _lib.lib()
    _call("rs_hard_pixel_select", k, _dev(targets, "targets", torch.int64), _dev(base, "base"), _dev(plane, "plane"),
          _dev(info, "info", torch.int64), n, h, w, fraction, cap, ignore,
          _workspace(lib.rs_hard_pixel_workspace_bytes(n, h, w), keys.device), _stream())
    return plane, info


def nll_loss_fwd(logits, targets, weight, mode, gamma=2.0, ignore=None, pixel_weight=None, label_sets=None):
    """``ignore`` (here and in the four losses below): the label value whose pixels are left out of the loss
    (``rs_*_ig`` in include/robosat_hip.h); ``None`` calls the entry point without it.  ``pixel_weight`` float32 [N, H, W]
    (``rs_nll_loss_*_pw``): a non-negative weight per pixel on top of the class weight; ``None`` makes the calls made without it.
    ``label_sets`` uint8 [N, H, W] (``rs_nll_loss_*_rx``, the plane of ``label_set_plane``): the relaxed loss, the probability of a
    pixel's whole class set in place of its own class's; ``None`` makes the calls made without it."""

    n, c, h, w = logits.shape
    lib = _lib.lib()
    ignore = _ignore_label(ignore, c)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    stats = torch.empty(2, device=logits.device, dtype=torch.float32)
    if label_sets is not None:
        assert tuple(label_sets.shape) == (n, h, w), "label_sets is [N, H, W]"
        assert pixel_weight is None or tuple(pixel_weight.shape) == (n, h, w), "pixel_weight is [N, H, W]"
        _call("rs_nll_loss_fwd_rx", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"),
              _dev(loss, "loss"), _dev(stats, "stats"), n, c, h, w, mode, ctypes.c_float(gamma),
              _workspace(lib.rs_nll_loss_workspace_bytes(), logits.device), _stream(), _dev(pixel_weight, "pixel_weight"),
              -1 if ignore is None else ignore, _dev(label_sets, "label_sets", torch.uint8))
        return loss, stats
    if pixel_weight is not None:
        assert tuple(pixel_weight.shape) == (n, h, w), "pixel_weight is [N, H, W]"
        _call("rs_nll_loss_fwd_pw", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"),
              _dev(loss, "loss"), _dev(stats, "stats"), n, c, h, w, mode, ctypes.c_float(gamma),
              _workspace(lib.rs_nll_loss_workspace_bytes(), logits.device), _stream(), _dev(pixel_weight, "pixel_weight"),
              -1 if ignore is None else ignore)
        return loss, stats
    if ignore is not None:
        _call("rs_nll_loss_fwd_ig", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"),
              _dev(loss, "loss"), _dev(stats, "stats"), n, c, h, w, mode, ctypes.c_float(gamma),
              _workspace(lib.rs_nll_loss_workspace_bytes(), logits.device), _stream(), ignore)
        return loss, stats
    _call("rs_nll_loss_fwd", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"), _dev(loss, "loss"),
          _dev(stats, "stats"), n, c, h, w, mode, ctypes.c_float(gamma), _workspace(lib.rs_nll_loss_workspace_bytes(), logits.device),
          _stream())
    return loss, stats


def nll_loss_bwd(logits, targets, weight, stats, grad_out, mode, gamma=2.0, ignore=None, pixel_weight=None, label_sets=None):
    n, c, h, w = logits.shape
    ignore = _ignore_label(ignore, c)
    dlogits = torch.empty_like(logits)
    if label_sets is not None:
        assert tuple(label_sets.shape) == (n, h, w), "label_sets is [N, H, W]"
        assert pixel_weight is None or tuple(pixel_weight.shape) == (n, h, w), "pixel_weight is [N, H, W]"
        _call("rs_nll_loss_bwd_rx", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"),
              _dev(stats, "stats"), _dev(grad_out, "grad_out"), _dev(dlogits, "dlogits"), n, c, h, w, mode, ctypes.c_float(gamma),
              _stream(), _dev(pixel_weight, "pixel_weight"), -1 if ignore is None else ignore,
              _dev(label_sets, "label_sets", torch.uint8))
        return dlogits
    if pixel_weight is not None:
        assert tuple(pixel_weight.shape) == (n, h, w), "pixel_weight is [N, H, W]"
        _call("rs_nll_loss_bwd_pw", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"),
              _dev(stats, "stats"), _dev(grad_out, "grad_out"), _dev(dlogits, "dlogits"), n, c, h, w, mode, ctypes.c_float(gamma),
              _stream(), _dev(pixel_weight, "pixel_weight"), -1 if ignore is None else ignore)
        return dlogits
    if ignore is not None:
        _call("rs_nll_loss_bwd_ig", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"),
              _dev(stats, "stats"), _dev(grad_out, "grad_out"), _dev(dlogits, "dlogits"), n, c, h, w, mode, ctypes.c_float(gamma),
              _stream(), ignore)
        return dlogits
    _call("rs_nll_loss_bwd", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"), _dev(stats, "stats"),
          _dev(grad_out, "grad_out"), _dev(dlogits, "dlogits"), n, c, h, w, mode, ctypes.c_float(gamma), _stream())
    return dlogits


def miou_loss_fwd(logits, targets, weight, ignore=None):
    n, c, h, w = logits.shape
    lib = _lib.lib()
    ignore = _ignore_label(ignore, c)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    stats = torch.empty(5 + 2 * n * c, device=logits.device, dtype=torch.float32)
    if ignore is not None:
        _call("rs_miou_loss_fwd_ig", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"),
              _dev(loss, "loss"), _dev(stats, "stats"), n, c, h, w, _workspace(lib.rs_miou_loss_workspace_bytes(n, c), logits.device),
              _stream(), ignore)
        return loss, stats
    _call("rs_miou_loss_fwd", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"), _dev(loss, "loss"),
          _dev(stats, "stats"), n, c, h, w, _workspace(lib.rs_miou_loss_workspace_bytes(n, c), logits.device), _stream())
    return loss, stats


def miou_loss_bwd(logits, targets, weight, stats, grad_out, ignore=None):
    n, c, h, w = logits.shape
    ignore = _ignore_label(ignore, c)
    dlogits = torch.empty_like(logits)
    if ignore is not None:
        _call("rs_miou_loss_bwd_ig", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"),
              _dev(stats, "stats"), _dev(grad_out, "grad_out"), _dev(dlogits, "dlogits"), n, c, h, w, _stream(), ignore)
        return dlogits
    _call("rs_miou_loss_bwd", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"), _dev(stats, "stats"),
          _dev(grad_out, "grad_out"), _dev(dlogits, "dlogits"), n, c, h, w, _stream())
    return dlogits


def tversky_params(alpha, beta, gamma, smooth, ce):
    """``(alpha, beta, gamma, smooth, ce)`` of the Tversky family as floats; raises ``ValueError`` unless all are finite numbers with
    alpha, beta >= 0 and not both 0, gamma > 0, smooth >= 0, ce >= 0 (what ``rs_tversky_finalize`` takes)."""

    import math

    values = []
    for name, value in (("alpha", alpha), ("beta", beta), ("gamma", gamma), ("smooth", smooth), ("ce", ce)):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
            raise ValueError("tversky: {} must be a finite number, got {!r}".format(name, value))
        values.append(float(value))
    alpha, beta, gamma, smooth, ce = values
    if alpha < 0 or beta < 0 or (alpha == 0 and beta == 0):
        raise ValueError("tversky: alpha and beta must be >= 0 and not both 0, got {!r} and {!r}".format(alpha, beta))
    if not gamma > 0:
        raise ValueError("tversky: gamma must be > 0, got {!r}".format(gamma))
    if smooth < 0:
        raise ValueError("tversky: smooth must be >= 0, got {!r}".format(smooth))
    if ce < 0:
        raise ValueError("tversky: ce must be >= 0, got {!r}".format(ce))
    return alpha, beta, gamma, smooth, ce


def tversky_sums(logits, targets, weight=None, per_image=True, ignore=None):
    """``rs_tversky_sums``: the float64 sums of the Tversky family in one pass -- per image ``[N*C*3 + 2]`` = (TP, SP, cnt) of every
    (image, class), then the cross-entropy numerator and denominator; batch form ``[C*3 + 2]``.  ``weight`` weighs the cross-entropy
    sums only."""

    n, c, h, w = logits.shape
    lib = _lib.lib()
    ignore = _ignore_label(ignore, c)
    sums = torch.empty(3 * (n if per_image else 1) * c + 2, device=logits.device, dtype=torch.float64)
    _call("rs_tversky_sums", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"),
          _dev(sums, "sums", torch.float64), n, c, h, w, 1 if per_image else 0, -1 if ignore is None else ignore,
          _workspace(lib.rs_tversky_workspace_bytes(n, c), logits.device), _stream())
    return sums


def tversky_finalize(sums, n, c, alpha=0.5, beta=0.5, gamma=1.0, smooth=1.0, ce=0.0, classes="present", per_image=True, world=1):
    """``rs_tversky_finalize``: (loss, stats) from the sums of ``tversky_sums`` for logits of ``n`` images and ``c`` classes; ``world`` = the
    number of data-parallel ranks whose sums were added into ``sums`` (include/robosat_hip.h)."""

    if classes not in ("present", "all"):
        raise ValueError("classes must be \"present\" or \"all\" (got {!r})".format(classes))
    segments = (n if per_image else 1) * c
    assert sums.numel() == 3 * segments + 2, "sums does not belong to this shape and form"
    loss = torch.empty((), device=sums.device, dtype=torch.float32)
    stats = torch.empty(4 + 2 * segments, device=sums.device, dtype=torch.float32)
    _call("rs_tversky_finalize", _dev(sums, "sums", torch.float64), _dev(loss, "loss"), _dev(stats, "stats"), n, c,
          ctypes.c_float(alpha), ctypes.c_float(beta), ctypes.c_float(gamma), ctypes.c_float(smooth), ctypes.c_float(ce),
          1 if classes == "all" else 0, 1 if per_image else 0, int(world), _stream())
    return loss, stats


def tversky_bwd(logits, targets, weight, stats, grad_out, ce=0.0, per_image=True, ignore=None):
    """``rs_tversky_bwd``: d loss / d logits from the ``stats`` of ``tversky_finalize``; ``grad_out`` may be ``None`` (= 1)."""

    n, c, h, w = logits.shape
    ignore = _ignore_label(ignore, c)
    assert stats.numel() == 4 + 2 * (n if per_image else 1) * c, "stats does not belong to this shape and form"
    dlogits = torch.empty_like(logits)
    _call("rs_tversky_bwd", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(weight, "weight"), _dev(stats, "stats"),
          _dev(grad_out, "grad_out"), _dev(dlogits, "dlogits"), n, c, h, w, 1 if per_image else 0, ctypes.c_float(ce),
          -1 if ignore is None else ignore, _stream())
    return dlogits


SKELETON_MAX_ITERS = 64


def _skeleton_args(planes, iters):
    if planes.dim() != 3:
        raise ValueError("robosat_amd: the soft skeleton takes fp32 planes [M, H, W], got a shape of {}".format(tuple(planes.shape)))
    if isinstance(iters, bool) or int(iters) != iters or not 0 <= int(iters) <= SKELETON_MAX_ITERS:
        raise ValueError("robosat_amd: the soft skeleton takes 0..{} iterations, got {!r}".format(SKELETON_MAX_ITERS, iters))
    return tuple(planes.shape) + (int(iters),)


def soft_skeleton(planes, iters, save=True):
    """``rs_soft_skeleton_fwd``: float32 planes ``[M, H, W]`` with values in [0, 1] -> ``(skeleton [M, H, W], saved)``, the paper's
    ``soft_skel`` with ``iters`` iterations (include/robosat_hip.h).  ``saved`` is what ``soft_skeleton_bwd`` takes: the planes, the
    2 * iters + 1 planes of erosions and partial skeletons, and ``iters``.  ``save=False`` keeps nothing and returns ``None`` for it."""

    m, h, w, iters = _skeleton_args(planes, iters)
    lib = _lib.lib()
    skel = torch.empty_like(planes)
    nfloats = lib.rs_soft_skeleton_state_floats(m, h, w, iters, 1 if save else 0)
    if nfloats < 0:
        raise ValueError("robosat_amd: the soft skeleton does not take planes of {} (RS_EINVAL)".format((m, h, w)))
    if save:
        state = torch.empty(nfloats, device=planes.device, dtype=torch.float32)
        ptr = _dev(state, "state")
    else:
        state, ptr = None, _workspace(4 * nfloats, planes.device)
    _call("rs_soft_skeleton_fwd", _dev(planes, "planes"), _dev(skel, "skel"), ptr, m, h, w, iters, 1 if save else 0, _stream())
    return skel, ((planes, state, iters) if save else None)


def soft_skeleton_bwd(saved, grad):
    """``rs_soft_skeleton_bwd``: d loss / d planes from ``grad`` = d loss / d skeleton and the ``saved`` of ``soft_skeleton``."""

    planes, state, iters = saved
    m, h, w, iters = _skeleton_args(planes, iters)
    if tuple(grad.shape) != (m, h, w):
        raise ValueError("robosat_amd: the skeleton's gradient is [M, H, W] = {}, got {}".format((m, h, w), tuple(grad.shape)))
    lib = _lib.lib()
    dplanes = torch.empty_like(planes)
    _call("rs_soft_skeleton_bwd", _dev(planes, "planes"), _dev(state, "state"), _dev(grad, "grad"), _dev(dplanes, "dplanes"), m, h, w,
          iters, _workspace(lib.rs_soft_skeleton_bwd_workspace_bytes(m, h, w, iters), planes.device), _stream())
    return dplanes


def cldice_class_mask(classes, c):
    """The bit mask of ``rs_cldice_*`` for logits of ``c`` classes: ``None`` = every class 1 .. c - 1, else the listed indices."""

    if classes is None:
        picked = list(range(1, c))
    else:
        picked = sorted(set(int(k) for k in classes))
        if not picked or len(picked) != len(list(classes)) or picked[0] < 1 or picked[-1] >= c:
            raise ValueError("cldice: classes are distinct indices in 1..{} for logits of {} classes (0 is the background), got {!r}".format(
                c - 1, c, list(classes)))
    if not picked:
        raise ValueError("cldice: logits of {} class have no non-background class".format(c))
    mask = 0
    for k in picked:
        mask |= 1 << k
    return mask, len(picked)


def cldice_planes(logits, targets, classes=None, ignore=None):
    """``rs_cldice_planes``: ``(P, Y)``, each float32 ``[N * K, H, W]`` in the order [image][class ascending]: the softmax plane and the
    0/1 label plane of every selected class, both 0 at an ignored pixel."""

    n, c, h, w = logits.shape
    mask, k = cldice_class_mask(classes, c)
    ignore = _ignore_label(ignore, c)
    p = torch.empty((n * k, h, w), device=logits.device, dtype=torch.float32)
    y = torch.empty_like(p)
    _call("rs_cldice_planes", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(p, "P"), _dev(y, "Y"), n, c, h, w, mask,
          -1 if ignore is None else ignore, _stream())
    return p, y


def cldice_sums(p, y, sp, sy):
    """``rs_cldice_sums``: float64 ``[pairs, 4]`` = (sum S_P Y, sum S_P, sum S_Y P, sum S_Y) per plane, in a fixed order."""

    pairs, h, w = p.shape
    assert p.shape == y.shape == sp.shape == sy.shape
    lib = _lib.lib()
    sums = torch.empty((pairs, 4), device=p.device, dtype=torch.float64)
    _call("rs_cldice_sums", _dev(p, "P"), _dev(y, "Y"), _dev(sp, "SP"), _dev(sy, "SY"), _dev(sums, "sums", torch.float64), pairs, h, w,
          _workspace(lib.rs_cldice_workspace_bytes(pairs), p.device), _stream())
    return sums


def cldice_finalize(sums, smooth=1.0):
    """``rs_cldice_finalize``: ``(loss, coef [pairs, 3])`` from the sums; d loss / d S_P = coef[:, 0] Y + coef[:, 1] per pixel and
    d loss / d P through the sensitivity = coef[:, 2] S_Y."""

    pairs = sums.shape[0]
    loss = torch.empty((), device=sums.device, dtype=torch.float32)
    coef = torch.empty((pairs, 3), device=sums.device, dtype=torch.float32)
    _call("rs_cldice_finalize", _dev(sums, "sums", torch.float64), _dev(loss, "loss"), _dev(coef, "coef"), pairs, ctypes.c_float(smooth),
          _stream())
    return loss, coef


def cldice_skel_grad(y, coef):
    """``rs_cldice_skel_grad``: d loss / d S_P = alpha Y + beta, what ``soft_skeleton_bwd`` is given."""

    pairs, h, w = y.shape
    grad = torch.empty_like(y)
    _call("rs_cldice_skel_grad", _dev(y, "Y"), _dev(coef, "coef"), _dev(grad, "grad"), pairs, h, w, _stream())
    return grad


def cldice_bwd(logits, targets, dp, sy, coef, grad_out, classes=None, ignore=None):
    """``rs_cldice_bwd``: d loss / d logits from ``dp`` = the skeleton's backward and the direct term ``coef[:, 2] S_Y``, through the
    softmax Jacobian restricted to the selected planes; ``grad_out`` may be ``None`` (= 1)."""

    n, c, h, w = logits.shape
    mask, _ = cldice_class_mask(classes, c)
    ignore = _ignore_label(ignore, c)
    dlogits = torch.empty_like(logits)
    _call("rs_cldice_bwd", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(dp, "dP"), _dev(sy, "SY"), _dev(coef, "coef"),
          _dev(grad_out, "grad_out"), _dev(dlogits, "dlogits"), n, c, h, w, mask, -1 if ignore is None else ignore, _stream())
    return dlogits


def lovasz_fwd(logits, targets, want_grad=True, ignore=None):
    """Returns (loss, d loss / d logits for grad_out = 1 or None)."""

    n, c, h, w = logits.shape
    lib = _lib.lib()
    ignore = _ignore_label(ignore, c)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    grad = torch.empty_like(logits) if want_grad else None
    if ignore is not None:
        _call("rs_lovasz_fwd_ig", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(loss, "loss"), _dev(grad, "grad"),
              n, c, h, w, _workspace(lib.rs_lovasz_workspace_bytes(n, c, h, w), logits.device), _stream(), ignore)
        return loss, grad
    _call("rs_lovasz_fwd", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(loss, "loss"), _dev(grad, "grad"), n, c, h,
          w, _workspace(lib.rs_lovasz_workspace_bytes(n, c, h, w), logits.device), _stream())
    return loss, grad


def lovasz_softmax_fwd(logits, targets, per_image=True, classes="present", want_grad=True, want_probs=False, ignore=None):
    """Lovasz-Softmax (``rs_lovasz_softmax_fwd``): returns (loss, d loss / d logits for grad_out = 1 or None, fp32
    softmax probabilities NCHW or None)."""

    if classes not in ("present", "all"):
        raise ValueError("classes must be \"present\" or \"all\" (got {!r})".format(classes))
    n, c, h, w = logits.shape
    lib = _lib.lib()
    pi = 1 if per_image else 0
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    grad = torch.empty_like(logits) if want_grad else None
    probs = torch.empty_like(logits) if want_probs else None
    nbytes = lib.rs_lovasz_softmax_workspace_bytes(n, c, h, w, pi)
    ignore = _ignore_label(ignore, c)
    if ignore is not None:
        _call("rs_lovasz_softmax_fwd_ig", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(loss, "loss"),
              _dev(grad, "grad"), _dev(probs, "probs"), n, c, h, w, pi, 1 if classes == "all" else 0, _workspace(nbytes, logits.device),
              _stream(), ignore)
        return loss, grad, probs
    _call("rs_lovasz_softmax_fwd", _dev(logits, "logits"), _dev(targets, "targets", torch.int64), _dev(loss, "loss"), _dev(grad, "grad"),
          _dev(probs, "probs"), n, c, h, w, pi, 1 if classes == "all" else 0, _workspace(nbytes, logits.device), _stream())
    return loss, grad, probs


def scale_by_scalar(src, scalar):
    out = torch.empty_like(src)
    _call("rs_scale_by_scalar", _dev(src, "src"), _dev(scalar, "scalar"), _dev(out, "out"), src.numel(), _stream())
    return out


def confusion_counts(scores, targets, counts):
    """counts (uint64-as-int64 [4] device tensor) += (tn, fn, fp, tp) of the whole batch (reference naming)."""

    n, c, h, w = scores.shape
    _call("rs_confusion_counts", _dev(scores, "scores"), _dev(targets, "targets", torch.int64), _dev(counts, "counts", torch.int64), n, c,
          h, w, _stream())
    return counts


def confusion_matrix(scores, targets, counts):
    """counts (int64 [C*C] device tensor, row = actual, column = predicted) += the batch's confusion matrix."""

    n, c, h, w = scores.shape
    assert counts.numel() == c * c
    _call("rs_confusion_matrix", _dev(scores, "scores"), _dev(targets, "targets", torch.int64), _dev(counts, "counts", torch.int64), n, c,
          h, w, _stream())
    return counts


def label_histogram_u8(labels, counts256):
    """counts256 (int64 [256] device tensor) += np.bincount(labels) of a uint8 device tensor (tools/weights.py:41-47)."""

    _call("rs_label_histogram_u8", _dev(labels, "labels", torch.uint8), labels.numel(), _dev(counts256, "counts", torch.int64), _stream())
    return counts256


def softvote_masks(quantized, weights=None, threshold=None):
    """quantized uint8 [K, P] (binary models) or [K, P, C-1] -> uint8 [P] class indices: the weighted soft vote of
    tools/masks.py:42-84 over K models' probability bytes.  With ``threshold`` (binary models only, 0 < T <= 1) the mask is
    ``voted foreground >= T`` in place of the argmax (``rs_softvote_masks_threshold``)."""

    if quantized.dim() == 2:
        quantized = quantized.unsqueeze(-1)
    k, p, cq = quantized.shape
    out = torch.empty(p, device=quantized.device, dtype=torch.uint8)
    wt = None if weights is None else torch.as_tensor(list(weights), dtype=torch.float64).to(quantized.device)
    if threshold is not None:
        threshold = float(threshold)
        if cq != 1:
            raise ValueError("robosat_amd: a threshold cuts the one foreground probability of a binary model; these probabilities "
                             "are of {} classes".format(cq + 1))
        if not 0 < threshold <= 1:  # (false for nan too)
            raise ValueError("robosat_amd: the threshold is a probability, 0 < T <= 1, got {}".format(threshold))
        _call("rs_softvote_masks_threshold", _dev(quantized, "quantized", torch.uint8), _dev(wt, "weights", torch.float64),
              _dev(_anchors(quantized.device), "anchors", torch.float64), _dev(out, "out", torch.uint8), k, p, ctypes.byref(ctypes.c_double(threshold)), _stream())
        return out
    _call("rs_softvote_masks", _dev(quantized, "quantized", torch.uint8), _dev(wt, "weights", torch.float64),
          _dev(_anchors(quantized.device), "anchors", torch.float64), _dev(out, "out", torch.uint8), k, p, cq + 1, _stream())
    return out


def augment_tiles(images, masks, index, op, mean, std):
    """Batch from a decoded-tile cache: images uint8 [T,S,S,C], masks uint8 [T,S,S] or None, index / op int32 [N] device
    tensors -> (images fp32 NCHW [N,C,S,S], masks int64 [N,S,S] or None): flip / rot90 / ToTensor / Normalize in one pass."""

    t, s, s2, c = images.shape
    assert s == s2, "square tiles (a 90-degree rotation must keep the shape)"
    n = index.numel()
    out = torch.empty((n, c, s, s), device=images.device, dtype=torch.float32)
    om = torch.empty((n, s, s), device=images.device, dtype=torch.int64) if masks is not None else None
    fm, fs = (ctypes.c_float * c)(*mean), (ctypes.c_float * c)(*std)
    _call("rs_augment_tiles", _dev(images, "images", torch.uint8), _dev(masks, "masks", torch.uint8), _dev(index, "index", torch.int32),
          _dev(op, "op", torch.int32), fm, fs, _dev(out, "out"), _dev(om, "out_masks", torch.int64), n, s, c, _stream())
    return out, om


def tile_band_sums(images):
    """images uint8 [T,S,S,C] (C <= 4; any slice that is contiguous) -> int64 [T,C]: the sum of every band of every tile, in
    integers (the band means of the contrast stage of ``augment_tiles_jitter``)."""

    t, s, s2, c = images.shape
    assert s == s2, "square tiles"
    sums = torch.empty((t, c), device=images.device, dtype=torch.int64)
    _call("rs_tile_band_sums", _dev(images, "images", torch.uint8), _dev(sums, "sums", torch.int64), t, s, c, _stream())
    return sums


def augment_tiles_jitter(images, masks, index, op, geom, color, band_sums, mean, std, rgb):
    """``augment_tiles`` with a zoom-in window and colour factors per item (include/robosat_hip.h): ``geom`` int32 [N,3] =
    (w, x0, y0) and ``color`` float32 [N,4] = (brightness, contrast, saturation, gamma) are HOST values (tensors or nested
    lists), ``band_sums`` is ``tile_band_sums(images)`` (None is allowed when no item has a contrast factor), ``rgb`` says
    that bands 0..2 are R, G, B (saturation runs only then).  Identity parameters give ``augment_tiles`` bit for bit."""

    t, s, s2, c = images.shape
    assert s == s2, "square tiles (a 90-degree rotation must keep the shape)"
    n = index.numel()
    geom = torch.as_tensor(geom, dtype=torch.int32).contiguous()
    color = torch.as_tensor(color, dtype=torch.float32).contiguous()
    if geom.is_cuda or color.is_cuda:
        raise RuntimeError("robosat_amd: `geom` and `color` are host values (the launch checks them and carries them as arguments)")
    if tuple(geom.shape) != (n, 3) or tuple(color.shape) != (n, 4):
        raise ValueError("robosat_amd: `geom` must be [N,3] and `color` [N,4] for the N = {} items of `index`".format(n))
    if band_sums is not None and tuple(band_sums.shape) != (t, c):
        raise ValueError("robosat_amd: `band_sums` must be [T,C] = [{},{}], the sums of these `images`".format(t, c))
    out = torch.empty((n, c, s, s), device=images.device, dtype=torch.float32)
    om = torch.empty((n, s, s), device=images.device, dtype=torch.int64) if masks is not None else None
    fm, fs = (ctypes.c_float * c)(*mean), (ctypes.c_float * c)(*std)
    _call("rs_augment_tiles_jitter", _dev(images, "images", torch.uint8), _dev(masks, "masks", torch.uint8),
          _dev(index, "index", torch.int32), _dev(op, "op", torch.int32), ctypes.cast(geom.data_ptr(), ctypes.POINTER(ctypes.c_int32)),
          ctypes.cast(color.data_ptr(), ctypes.POINTER(ctypes.c_float)), _dev(band_sums, "band_sums", torch.int64), fm, fs,
          _dev(out, "out"), _dev(om, "out_masks", torch.int64), n, s, c, int(bool(rgb)), _stream())
    return out, om


def augment_tiles_rotate(images, masks, index, op, geom, rot, color, band_sums, mean, std, rgb):
    """``augment_tiles_jitter`` with the window turned about its centre (include/robosat_hip.h): ``rot`` int32 [N,2] = (c, s),
    the cosine and sine of each item's angle in units of 2**-16 (``robosat_amd.augment.rotation``), is a HOST value like ``geom``
    and ``color``.  Where the turned window leaves the tile it reads the tile mirrored about its edges, image and mask alike."""

    t, s, s2, c = images.shape
    assert s == s2, "square tiles (a 90-degree rotation must keep the shape)"
    n = index.numel()
    geom = torch.as_tensor(geom, dtype=torch.int32).contiguous()
    rot = torch.as_tensor(rot, dtype=torch.int32).contiguous()
    color = torch.as_tensor(color, dtype=torch.float32).contiguous()
    if geom.is_cuda or rot.is_cuda or color.is_cuda:
        raise RuntimeError("robosat_amd: `geom`, `rot` and `color` are host values (the launch checks them and carries them as arguments)")
    if tuple(geom.shape) != (n, 3) or tuple(rot.shape) != (n, 2) or tuple(color.shape) != (n, 4):
        raise ValueError("robosat_amd: `geom` must be [N,3], `rot` [N,2] and `color` [N,4] for the N = {} items of `index`".format(n))
    if band_sums is not None and tuple(band_sums.shape) != (t, c):
        raise ValueError("robosat_amd: `band_sums` must be [T,C] = [{},{}], the sums of these `images`".format(t, c))
    out = torch.empty((n, c, s, s), device=images.device, dtype=torch.float32)
    om = torch.empty((n, s, s), device=images.device, dtype=torch.int64) if masks is not None else None
    fm, fs = (ctypes.c_float * c)(*mean), (ctypes.c_float * c)(*std)
    _call("rs_augment_tiles_rotate", _dev(images, "images", torch.uint8), _dev(masks, "masks", torch.uint8),
          _dev(index, "index", torch.int32), _dev(op, "op", torch.int32), ctypes.cast(geom.data_ptr(), ctypes.POINTER(ctypes.c_int32)),
          ctypes.cast(rot.data_ptr(), ctypes.POINTER(ctypes.c_int32)), ctypes.cast(color.data_ptr(), ctypes.POINTER(ctypes.c_float)),
          _dev(band_sums, "band_sums", torch.int64), fm, fs, _dev(out, "out"), _dev(om, "out_masks", torch.int64), n, s, c,
          int(bool(rgb)), _stream())
    return out, om


# ---- rs features: raster stages (csrc/features.hip; definitions in include/robosat_hip.h) --------------------------------
CLEAN_AUTO, CLEAN_LDS, CLEAN_HBM = 0, 1, 2


def disc_rows(eps):
    """Per-row half-widths dx of ``disc(eps)`` (OpenCV's documented MORPH_ELLIPSE, eps x eps): r = c = eps // 2, row i has
    dy = i - r, dx = rint(c * sqrt((r*r - dy*dy) / (r*r))) and columns max(c - dx, 0) .. min(c + dx + 1, eps) - 1 set."""

    import math

    r = c = eps // 2
    rows = []
    for i in range(eps):
        dy = i - r
        rows.append(int(round(c * math.sqrt((r * r - dy * dy) / (r * r)))) if r else 0)  # (round: half to even, as rint)
    return rows


def disc(eps):
    """``disc(eps)`` as an eps x eps uint8 0/1 numpy matrix (what ``getStructuringElement(MORPH_ELLIPSE, (eps, eps))`` documents)."""

    import numpy as np

    k = np.zeros((eps, eps), dtype=np.uint8)
    c = eps // 2
    for i, dx in enumerate(disc_rows(eps)):
        k[i, max(c - dx, 0):min(c + dx + 1, eps)] = 1
    return k


def _disc_arg(eps):
    if eps < 0 or eps > 64:
        raise ValueError("robosat_amd: disc diameter must be in 0..64, got {}".format(eps))
    return (ctypes.c_int32 * max(eps, 1))(*(disc_rows(eps) or [0]))


def clean_form(h, w):
    """CLEAN_LDS where a tile's two bit-planes fit the 160 KB LDS, else CLEAN_HBM."""

    return _lib.lib().rs_features_clean_form(h, w)


def clean_masks(images_u8, index, eps_open, eps_close, form=CLEAN_AUTO):
    """uint8 [B, H, W] class-index masks -> uint8 0/1 [B, H, W]: close(open(images == index)) with discs of diameter
    eps_open (``--denoise``) and eps_close (``--grow``)."""

    b, h, w = images_u8.shape
    out = torch.empty_like(images_u8)
    lib = _lib.lib()
    ws = None
    if form != CLEAN_LDS:  # (CLEAN_AUTO is the HBM form: profiles/features)
        ws = torch.empty(lib.rs_features_clean_workspace_bytes(b, h, w), device=images_u8.device, dtype=torch.uint8)
    _call("rs_features_clean", _dev(images_u8, "images", torch.uint8), _dev(out, "out", torch.uint8), _dev(ws, "workspace", torch.uint8), b,
          h, w, index, eps_open, _disc_arg(eps_open), eps_close, _disc_arg(eps_close), form, _stream())
    return out


def label_components(masks):
    """uint8 [B, H, W] (non-zero = foreground) -> int32 [B, H, W]: 4-connected components, label = 1 + min(y * W + x) of the
    component, background 0."""

    b, h, w = masks.shape
    labels = torch.empty((b, h, w), device=masks.device, dtype=torch.int32)
    err = torch.zeros(1, device=masks.device, dtype=torch.int32)
    _call("rs_features_label", _dev(masks, "masks", torch.uint8), _dev(labels, "labels", torch.int32), _dev(err, "err", torch.int32), b, h,
          w, _stream())
    if int(err.item()):
        raise RuntimeError("rs_features_label: a union-find loop ran out of its H*W bound (code {})".format(int(err.item())))
    return labels


def component_table(labels, min_area=0):
    """int32 [B, H, W] canonical labels -> int32 [N, 7] rows (tile, label, area, x0, y0, x1, y1) of the components with
    area >= min_area, sorted by (tile, label)."""

    b, h, w = labels.shape
    dev = labels.device
    slotmap = torch.empty((b, h, w), device=dev, dtype=torch.int32)
    counters = torch.empty(2, device=dev, dtype=torch.int32)
    capacity = 1 << 16
    for _ in range(2):  # (the second pass has the exact capacity)
        raw = torch.empty((capacity, 6), device=dev, dtype=torch.int32)
        table = torch.empty((capacity, 7), device=dev, dtype=torch.int32)
        _call("rs_features_components", _dev(labels, "labels", torch.int32), _dev(slotmap, "slotmap", torch.int32),
              _dev(raw, "raw", torch.int32), _dev(table, "table", torch.int32), _dev(counters, "counters", torch.int32), capacity, b, h, w,
              int(min_area), _stream())
        found, kept = counters.tolist()
        if found <= capacity:
            break
        capacity = found
    else:
        raise RuntimeError("rs_features_components: {} components do not fit a table of {}".format(found, capacity))
    table = table[:kept]
    order = torch.argsort(table[:, 0].to(torch.int64) * (h * w + 1) + table[:, 1].to(torch.int64))
    return table[order].contiguous()


def boundary_edges(labels, table):
    """Directed unit boundary edges of the components in ``table``: int32 [E, 5] rows (tile, label, x, y, dir), in the
    order the device wrote them (sort on the host)."""

    b, h, w = labels.shape
    dev = labels.device
    keep = torch.empty(b * h * w, device=dev, dtype=torch.uint8)
    counter = torch.empty(1, device=dev, dtype=torch.int32)
    table = table.contiguous()

    def run(edges, capacity):
        _call("rs_features_edges", _dev(labels, "labels", torch.int32), _dev(table, "table", torch.int32) if len(table) else None,
              len(table), _dev(keep, "keep", torch.uint8), _dev(edges, "edges", torch.int32), capacity,
              _dev(counter, "counter", torch.int32), b, h, w, _stream())
        return int(counter.item())

    n = run(None, 0)
    edges = torch.empty((n, 5), device=dev, dtype=torch.int32)
    if n:
        got = run(edges, n)
        assert got == n, (got, n)
    return edges


# ---- rs features --stitch: the tiles of a call as one sparse raster (tables from robosat_amd.features.stitch_tables) ----------
def halo_apron(eps_open, eps_close):
    """Apron A of ``gather_halo`` for these discs: the reach of open followed by close (an eps of 0 or 1 is the identity)."""

    return (eps_open if eps_open > 1 else 0) + (eps_close if eps_close > 1 else 0)


def _halo(src, nbr, apron, fill, crop):
    t, hs, ws = src.shape
    h, w = (hs - 2 * apron, ws - 2 * apron) if crop else (hs, ws)
    if apron < 0 or h <= 0 or w <= 0 or apron > min(h, w):
        raise ValueError("robosat_amd: an apron of {} does not fit tiles of {}x{} (at most min(H, W))".format(apron, h, w))
    out = torch.empty((t, h, w) if crop else (t, h + 2 * apron, w + 2 * apron), device=src.device, dtype=torch.uint8)
    _call("rs_features_halo", _dev(src, "src", torch.uint8), _dev(out, "out", torch.uint8), _dev(nbr, "nbr", torch.int32), t, h, w, apron,
          fill, int(crop), _stream())
    return out


def gather_halo(images_u8, nbr, apron, fill=0):
    """uint8 [T, H, W] tiles + int32 [T, 8] neighbour slots -> uint8 [T, H + 2A, W + 2A]: every tile with an apron of A pixels
    from its 8 neighbours, ``fill`` where there is none."""

    assert nbr.shape == (images_u8.shape[0], 8), "nbr is [T, 8]"
    return _halo(images_u8, nbr, apron, fill, False)


def crop_halo(padded_u8, apron):
    """uint8 [T, H + 2A, W + 2A] -> the centres, uint8 [T, H, W]."""

    return _halo(padded_u8, None, apron, 0, True)


def clean_masks_stitched(images_u8, nbr, index, eps_open, eps_close):
    """``clean_masks`` of the one raster the tiles form: gather the apron, clean the padded tiles, crop."""

    apron = halo_apron(eps_open, eps_close)
    if apron == 0:
        return clean_masks(images_u8, index, eps_open, eps_close)
    padded = gather_halo(images_u8, nbr, apron, fill=255 if index == 0 else 0)  # (a byte that is not the class)
    return crop_halo(clean_masks(padded, index, eps_open, eps_close), apron)


def stitch_labels(labels, nbr, inplace=False):
    """Per-tile canonical labels int32 [T, H, W] (``label_components``) -> the labels of the whole raster (a new tensor unless
    ``inplace``): components joined across the seams of present 4-neighbour tiles, label = 1 + min(slot * H * W + y * W + x)."""

    t, h, w = labels.shape
    assert nbr.shape == (t, 8), "nbr is [T, 8]"
    out = labels if inplace else labels.clone()
    err = torch.zeros(1, device=labels.device, dtype=torch.int32)
    _call("rs_features_stitch_labels", _dev(out, "labels", torch.int32), _dev(nbr, "nbr", torch.int32), _dev(err, "err", torch.int32), t, h,
          w, _stream())
    if int(err.item()):
        raise RuntimeError("rs_features_stitch_labels: a union-find loop ran out of its T*H*W bound (code {})".format(int(err.item())))
    return out


def component_table_stitched(labels, origin, min_area=0):
    """Stitched labels int32 [T, H, W] + int32 [T, 2] tile origins -> int32 [N, 6] rows (label, area, X0, Y0, X1, Y1) in mosaic
    pixels of the components whose whole area is >= min_area, sorted by label."""

    t, h, w = labels.shape
    assert origin.shape == (t, 2), "origin is [T, 2]"
    dev = labels.device
    slotmap = torch.empty((t, h, w), device=dev, dtype=torch.int32)
    counters = torch.empty(2, device=dev, dtype=torch.int32)
    capacity = 1 << 16
    for _ in range(2):  # (the second pass has the exact capacity)
        raw = torch.empty((capacity, 6), device=dev, dtype=torch.int32)
        table = torch.empty((capacity, 6), device=dev, dtype=torch.int32)
        _call("rs_features_components_stitched", _dev(labels, "labels", torch.int32), _dev(origin, "origin", torch.int32),
              _dev(slotmap, "slotmap", torch.int32), _dev(raw, "raw", torch.int32), _dev(table, "table", torch.int32),
              _dev(counters, "counters", torch.int32), capacity, t, h, w, int(min_area), _stream())
        found, kept = counters.tolist()
        if found <= capacity:
            break
        capacity = found
    else:
        raise RuntimeError("rs_features_components_stitched: {} components do not fit a table of {}".format(found, capacity))
    table = table[:kept]
    return table[torch.argsort(table[:, 0])].contiguous()


def boundary_edges_stitched(labels, nbr, origin, table):
    """Directed unit boundary edges of the components in ``table`` (``component_table_stitched``): int32 [E, 4] rows
    (label, X, Y, dir) in mosaic pixels, in the order the device wrote them."""

    t, h, w = labels.shape
    assert nbr.shape == (t, 8) and origin.shape == (t, 2)
    dev = labels.device
    keep = torch.empty(t * h * w, device=dev, dtype=torch.uint8)
    counter = torch.empty(1, device=dev, dtype=torch.int32)
    table = table.contiguous()

    def run(edges, capacity):
        _call("rs_features_edges_stitched", _dev(labels, "labels", torch.int32), _dev(nbr, "nbr", torch.int32),
              _dev(origin, "origin", torch.int32), _dev(table, "table", torch.int32) if len(table) else None, len(table),
              _dev(keep, "keep", torch.uint8), _dev(edges, "edges", torch.int32), capacity, _dev(counter, "counter", torch.int32), t, h, w,
              _stream())
        return int(counter.item())

    n = run(None, 0)
    edges = torch.empty((n, 4), device=dev, dtype=torch.int32)
    if n:
        got = run(edges, n)
        assert got == n, (got, n)
    return edges


def stitched_features(images_u8, nbr, origin, index, eps_open, eps_close, min_area=0):
    """Every raster stage of ``rs features --stitch`` for one call: class-index tiles uint8 [T, H, W] with their neighbour and
    origin tables -> (table int32 [N, 6], edges int32 [E, 4]) of the whole raster."""

    labels = stitch_labels(label_components(clean_masks_stitched(images_u8, nbr, index, eps_open, eps_close)), nbr, inplace=True)
    table = component_table_stitched(labels, origin, min_area)
    return table, boundary_edges_stitched(labels, nbr, origin, table)


# ---- rs features --dedupe: the overlap table of two label rasters (definitions in include/robosat_hip.h) ------------------------
OVERLAP_CAPACITY = 1 << 16  # rows of the first call (a hash table of 2^17 slots, 1.5 MB)


def overlap_table(labels_a, labels_b, stitched=False, capacity=None):
    """Two int32 [B, H, W] label rasters (``label_components`` / ``stitch_labels``) -> int32 [N, 4] rows
    (raster, label_a, label_b, count): one row per pair of components that share a pixel, ``count`` the pixels they share,
    sorted lexicographically.  ``raster`` is the tile, or 0 throughout with ``stitched`` (labels of one raster of B tiles).
    ``capacity``: the rows of the first call (default ``OVERLAP_CAPACITY``); a call that does not fit is repeated with the
    number of rows it reported, or with 8 times the capacity where the hash table itself ran out."""

    if labels_a.shape != labels_b.shape or labels_a.dim() != 3:
        raise ValueError("robosat_amd: the label rasters are both [B, H, W], got {} and {}".format(tuple(labels_a.shape), tuple(labels_b.shape)))
    if labels_a.device != labels_b.device:
        raise ValueError("robosat_amd: the label rasters are on {} and {}".format(labels_a.device, labels_b.device))
    b, h, w = labels_a.shape
    pixels = b * h * w
    group = pixels if stitched else h * w
    a, bb = _dev(labels_a, "labels_a", torch.int32), _dev(labels_b, "labels_b", torch.int32)
    dev = labels_a.device
    capacity = OVERLAP_CAPACITY if capacity is None else int(capacity)
    if capacity < 1:
        raise ValueError("robosat_amd: capacity is at least 1, got {}".format(capacity))
    lib = _lib.lib()
    counters = torch.empty(2, device=dev, dtype=torch.int32)
    while True:  # (capacity grows with every pass and a table of `pixels` rows holds every pair there can be)
        capacity = min(capacity, max(pixels, 1))
        ws = torch.empty(lib.rs_features_overlaps_workspace_bytes(capacity) // 8, device=dev, dtype=torch.int64)
        rows = torch.empty((capacity, 4), device=dev, dtype=torch.int32)
        _call("rs_features_overlaps", a, bb, _dev(ws, "workspace", torch.int64), _dev(rows, "rows", torch.int32), capacity,
              _dev(counters, "counters", torch.int32), pixels, group, _stream())
        found, lost = counters.tolist()
        if not lost and found <= capacity:
            break
        if capacity >= pixels:
            raise RuntimeError("rs_features_overlaps: {} rows (table full: {}) do not fit a table of {}".format(found, bool(lost), capacity))
        capacity = capacity * 8 if lost else found
    rows = rows[:found]
    if found:
        key = (rows[:, 0].to(torch.int64) * (group + 1) + rows[:, 1].to(torch.int64)) * (pixels + 1) + rows[:, 2].to(torch.int64)
        rows = rows[torch.argsort(key)]
    return rows.contiguous()


# ---- rs features --score: per-component sums of probability bytes (definitions in include/robosat_hip.h) ------------------------
SCORE_MAX_MODELS = 8


def component_scores(labels, table, quantized, stitched=False):
    """int32 [B, H, W] labels (``label_components``, ``stitch_labels`` or ``split_labels``), the rows of ``component_table``
    (``component_table_stitched`` with ``stitched``) or any subset of them, and uint8 [K, B, H, W] quantised probabilities of the
    class (one plane per model, 1 <= K <= 8) -> int64 [N, K]: row i holds, for every model, the exact sum of its bytes over the pixels
    of the table's i-th component."""

    if labels.dim() != 3:
        raise ValueError("robosat_amd: the label raster is [B, H, W], got {}".format(tuple(labels.shape)))
    if quantized.dim() != 4 or tuple(quantized.shape[1:]) != tuple(labels.shape):
        raise ValueError("robosat_amd: the probabilities are [K, B, H, W] over the labels' {}, got {}".format(tuple(labels.shape),
                                                                                                            tuple(quantized.shape)))
    k = quantized.shape[0]
    if not 1 <= k <= SCORE_MAX_MODELS:
        raise ValueError("robosat_amd: 1 to {} models are summed in one call, got {}".format(SCORE_MAX_MODELS, k))
    if table.dim() != 2 or table.shape[1] != (6 if stitched else 7):
        raise ValueError("robosat_amd: the table is [N, {}], got {}".format(6 if stitched else 7, tuple(table.shape)))
    if labels.device != quantized.device or labels.device != table.device:
        raise ValueError("robosat_amd: labels, table and probabilities are on {}, {} and {}".format(labels.device, table.device,
                                                                                                   quantized.device))
    b, h, w = labels.shape
    pixels = b * h * w
    table = table.contiguous()
    rowmap = torch.empty(pixels, device=labels.device, dtype=torch.int32)
    sums = torch.empty((len(table), k), device=labels.device, dtype=torch.int64)
    _call("rs_features_scores", _dev(labels, "labels", torch.int32), _dev(quantized, "quantized", torch.uint8),
          _dev(table, "table", torch.int32) if len(table) else None, len(table), int(bool(stitched)), _dev(rowmap, "rowmap", torch.int32),
          _dev(sums, "sums", torch.int64) if len(table) else None, pixels, pixels if stitched else h * w, k, _stream())
    return sums


# ---- rs features --geometry centerline: skeleton and links (definitions in include/robosat_hip.h) --------------------------------
THIN_PAIRS = 16  # pairs of sub-iterations enqueued between two reads of the device's counter (profiles/features_centerline)


def thin_masks(masks_u8, nbr=None, pairs=None, want_pairs=False):
    """uint8 [B, H, W] (non-zero = set) -> uint8 0/1 [B, H, W]: the Guo-Hall skeleton of every tile, or with ``nbr`` int32 [B, 8]
    of the one sparse raster the tiles form.  ``pairs`` pairs of sub-iterations (default ``THIN_PAIRS``) are enqueued per read of
    the counter; the result does not depend on it.  ``want_pairs``: also the number of pairs that were run."""

    b, h, w = masks_u8.shape
    pairs = THIN_PAIRS if pairs is None else int(pairs)
    if pairs < 1:
        raise ValueError("robosat_amd: thinning enqueues at least one pair per chunk, got {}".format(pairs))
    if nbr is not None:
        assert nbr.shape == (b, 8), "nbr is [T, 8]"
    dev = masks_u8.device
    out = torch.empty_like(masks_u8)
    masks, outp = _dev(masks_u8, "masks", torch.uint8), _dev(out, "out", torch.uint8)  # (a CPU tensor raises before anything is sized)
    ws = torch.empty(max(_lib.lib().rs_features_clean_workspace_bytes(b, h, w), 1), device=dev, dtype=torch.uint8)
    counters = torch.empty(2, device=dev, dtype=torch.int32)
    done = 0
    while True:
        _call("rs_features_thin", masks, outp, _dev(ws, "workspace", torch.uint8), _dev(nbr, "nbr", torch.int32),
              _dev(counters, "counters", torch.int32), b, h, w, pairs, int(done > 0), _stream())
        done += pairs
        if counters[1].item() == 0:
            return (out, done) if want_pairs else out
        if done > b * h * w:  # (every pair but the last deletes a pixel)
            raise RuntimeError("rs_features_thin: no fixed point after {} pairs on {} pixels".format(done, b * h * w))


def skeleton_links(skeleton, labels, table, nbr=None, origin=None):
    """Links of the skeleton uint8 [B, H, W] under the labels and table of the mask it was thinned from: int32 [N, 5] rows
    (tile, label, x, y, dir) with ``component_table``'s rows, or with ``nbr`` and ``origin`` int32 [N, 4] rows (label, X, Y, dir)
    in mosaic pixels with ``component_table_stitched``'s.  dir 0 E, 1 SE, 2 S, 3 SW; -1 a pixel without links.  In the order the
    device wrote them."""

    b, h, w = labels.shape
    if (nbr is None) != (origin is None):
        raise ValueError("robosat_amd: nbr and origin come together")
    assert skeleton.shape == labels.shape, "skeleton and labels are both [B, H, W]"
    if nbr is not None:
        assert nbr.shape == (b, 8) and origin.shape == (b, 2)
    dev = labels.device
    keep = torch.empty(b * h * w, device=dev, dtype=torch.uint8)
    counter = torch.empty(1, device=dev, dtype=torch.int32)
    table = table.contiguous()
    width = 5 if nbr is None else 4
    assert table.shape[1:] == (width + 2,), "table rows do not match the form"

    def run(links, capacity):
        _call("rs_features_skeleton_links", _dev(skeleton, "skeleton", torch.uint8), _dev(labels, "labels", torch.int32),
              _dev(nbr, "nbr", torch.int32), _dev(origin, "origin", torch.int32), _dev(table, "table", torch.int32) if len(table) else None,
              len(table), _dev(keep, "keep", torch.uint8), _dev(links, "links", torch.int32), capacity,
              _dev(counter, "counter", torch.int32), b, h, w, _stream())
        return int(counter.item())

    n = run(None, 0)
    links = torch.empty((n, width), device=dev, dtype=torch.int32)
    if n:
        got = run(links, n)
        assert got == n, (got, n)
    return links


def stitched_centerlines(images_u8, nbr, origin, index, eps_open, eps_close, min_area=0, width_radius=None):
    """Every raster stage of ``rs features --geometry centerline --stitch`` for one call: class-index tiles uint8 [T, H, W] with
    their neighbour and origin tables -> (table int32 [N, 6], links int32 [L, 4]) of the whole raster.  ``width_radius`` (``--width``):
    also ``distance_transform`` of the same cleaned mask with that radius, as a third result int32 [T, H, W]."""

    cleaned = clean_masks_stitched(images_u8, nbr, index, eps_open, eps_close)
    labels = stitch_labels(label_components(cleaned), nbr, inplace=True)
    table = component_table_stitched(labels, origin, min_area)
    links = skeleton_links(thin_masks(cleaned, nbr), labels, table, nbr, origin)
    if width_radius is None:
        return table, links
    return table, links, distance_transform(cleaned, width_radius, nbr)


# ---- rs features --width: capped squared Euclidean distance transform (definitions in include/robosat_hip.h) ---------------------
EDT_MAX_RADIUS = 128


def distance_transform(masks_u8, radius, nbr=None):
    """uint8 [B, H, W] (non-zero = set) -> int32 [B, H, W]: 0 at an unset pixel, at a set pixel min(radius^2, the squared distance
    in pixels to the nearest unset pixel of its tile), or with ``nbr`` int32 [B, 8] of the one sparse raster the tiles form.  Outside
    the raster (and in absent tiles) nothing is known: no distance comes from there.  ``radius`` in 1..128, with ``nbr`` at most
    min(H, W); a pixel at ``radius^2`` has no unset pixel within reach."""

    b, h, w = masks_u8.shape
    radius = int(radius)
    if not 1 <= radius <= EDT_MAX_RADIUS:
        raise ValueError("robosat_amd: the distance transform's radius is in 1..{}, got {}".format(EDT_MAX_RADIUS, radius))
    if nbr is not None:
        assert nbr.shape == (b, 8), "nbr is [T, 8]"
        if radius > min(h, w):
            raise ValueError("robosat_amd: a radius of {} does not fit stitched tiles of {}x{} (at most min(H, W))".format(radius, h, w))
    masks = _dev(masks_u8, "masks", torch.uint8)  # (a CPU tensor raises before anything is sized)
    g = torch.empty_like(masks_u8)
    d2 = torch.empty((b, h, w), device=masks_u8.device, dtype=torch.int32)
    _call("rs_features_edt", masks, _dev(nbr, "nbr", torch.int32), _dev(g, "g", torch.uint8), _dev(d2, "d2", torch.int32), b, h, w, radius,
          _stream())
    return d2


def sample_pixels(raster_i32, coords_i32):
    """int32 [B, H, W] raster + int32 [N, 3] rows (slot, y, x) -> int32 [N]: the raster's values at those pixels, gathered on the
    device (plain indexing: this is glue, the list is a few thousand skeleton pixels)."""

    if not raster_i32.is_cuda or not coords_i32.is_cuda:
        raise RuntimeError("robosat_amd: `raster` is on {} and `coords` on {} -- both live on the MI355X".format(raster_i32.device, coords_i32.device))
    if raster_i32.dim() != 3 or raster_i32.dtype != torch.int32 or coords_i32.dim() != 2 or coords_i32.shape[1] != 3 or coords_i32.dtype != torch.int32:
        raise ValueError("robosat_amd: sample_pixels takes an int32 [B, H, W] raster and int32 [N, 3] rows (slot, y, x)")
    c = coords_i32.long()
    return raster_i32[c[:, 0], c[:, 1], c[:, 2]]


# ---- rs features --split: touching objects into instances (definitions in include/robosat_hip.h) ---------------------------------
SPLIT_MAX_RADIUS = 64
GROW_STEPS = 16  # growth steps enqueued between two reads of the device's counters (profiles/features_split)


def grow_config():
    """(rows, columns, fused steps) of ``rs_features_grow``: the block of pixels a workgroup owns and the steps a launch takes."""

    h, w, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _call("rs_features_grow_config", ctypes.byref(h), ctypes.byref(w), ctypes.byref(k))
    return h.value, w.value, k.value


def split_seeds(labels, seed_labels, stitched=False):
    """Labels of a mask and of its cores, both int32 [B, H, W] -> int32 [B, H, W], the start raster of the growth: a core's label
    on its pixels, -1 on the rest of a component that holds a core, the component's own label where it holds none, 0 on background.
    ``stitched``: the labels are of the one raster the B tiles form."""

    if labels.shape != seed_labels.shape or labels.dim() != 3:
        raise ValueError("robosat_amd: the label rasters are both [B, H, W], got {} and {}".format(tuple(labels.shape), tuple(seed_labels.shape)))
    b, h, w = labels.shape
    pixels = b * h * w
    lm, ls = _dev(labels, "labels", torch.int32), _dev(seed_labels, "seed_labels", torch.int32)
    has = torch.empty(pixels, device=labels.device, dtype=torch.uint8)
    out = torch.empty_like(labels)
    _call("rs_features_split_seeds", lm, ls, _dev(has, "has", torch.uint8), _dev(out, "out", torch.int32), pixels,
          pixels if stitched else h * w, _stream())
    return out


def grow_labels(labels, nbr=None, steps=None, want_steps=False):
    """int32 [B, H, W] as ``split_seeds`` left it -> the same tensor, grown in place until no pixel is -1: every -1 pixel takes the
    label of the first of its N, W, E, S neighbours that had one before the step.  With ``nbr`` int32 [B, 8] the tiles are one sparse
    raster.  ``steps`` steps (default ``GROW_STEPS``) are enqueued per read of the counters; the result does not depend on it.
    ``want_steps``: also the number of steps that were enqueued.  -1 pixels that no label can reach raise."""

    b, h, w = labels.shape
    steps = GROW_STEPS if steps is None else int(steps)
    if steps < 1:
        raise ValueError("robosat_amd: the growth enqueues at least one step per chunk, got {}".format(steps))
    if nbr is not None:
        assert nbr.shape == (b, 8), "nbr is [T, 8]"
    lab = _dev(labels, "labels", torch.int32)  # (a CPU tensor raises before anything is sized)
    ws = torch.empty(_lib.lib().rs_features_grow_workspace_bytes(b, h, w) // 4 + 1, device=labels.device, dtype=torch.int32)
    counters = torch.empty(2, device=labels.device, dtype=torch.int32)
    done = 0
    while True:
        _call("rs_features_grow", lab, _dev(ws, "workspace", torch.int32), _dev(nbr, "nbr", torch.int32),
              _dev(counters, "counters", torch.int32), b, h, w, steps, _stream())
        done += steps
        assigned, left = counters.tolist()
        if left == 0:
            return (labels, done) if want_steps else labels
        if assigned == 0:
            raise RuntimeError("rs_features_grow: {} unassigned pixels that no label reaches (after {} steps)".format(left, done))


def split_labels(cleaned, labels, radius, nbr=None, steps=None):
    """``rs features --split``: the cleaned mask uint8 [B, H, W] and its labels int32 [B, H, W] (``label_components``, or with ``nbr``
    ``stitch_labels``) -> int32 [B, H, W] labels of instances: the cores a disc of ``radius`` pixels fits into, labelled like the mask
    and grown back over it; a component without a core keeps its label.  ``radius`` in 1..64, with ``nbr`` at most min(H, W).
    The host reads back the growth's counters once per chunk and, through the existing helpers that label the cores
    (``label_components``, ``stitch_labels``), their one-word error flags; no raster comes back."""

    radius = int(radius)
    if not 1 <= radius <= SPLIT_MAX_RADIUS:
        raise ValueError("robosat_amd: the split radius is in 1..{}, got {}".format(SPLIT_MAX_RADIUS, radius))
    d2 = distance_transform(cleaned, radius, nbr)
    cores = torch.empty_like(cleaned)
    _call("rs_features_split_cores", _dev(d2, "d2", torch.int32), _dev(cores, "cores", torch.uint8), d2.numel(), radius, _stream())
    seed_labels = label_components(cores)
    if nbr is not None:
        seed_labels = stitch_labels(seed_labels, nbr, inplace=True)
    return grow_labels(split_seeds(labels, seed_labels, stitched=nbr is not None), nbr, steps)


# ---- rs evaluate: per-group counts over two rasters (csrc/evaluate.hip; definitions in include/robosat_hip.h) --------------------
EVAL_MAX_CLASSES = 8
EVAL_MAX_DISTANCE = EDT_MAX_RADIUS - 1  # the band's D: the transform behind it has the radius D + 1


def eval_config():
    """Pixels one workgroup of ``mask_confusion`` / ``boundary_counts`` covers (consecutive ones of the whole call)."""

    n = ctypes.c_int()
    _call("rs_eval_config", ctypes.byref(n))
    return n.value


def _eval_pair(a, b, names, dtype):
    """The shared argument checks of the two counting calls -> (pointer, pointer, pixels, H*W)."""

    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError("robosat_amd: {} and {} are both [B, H, W], got {} and {}".format(names[0], names[1], tuple(a.shape), tuple(b.shape)))
    if a.device != b.device:
        raise ValueError("robosat_amd: {} and {} are on {} and {}".format(names[0], names[1], a.device, b.device))
    if a.numel() == 0 or a.numel() >= 1 << 31:
        raise ValueError("robosat_amd: a call counts 1 to 2^31 - 1 pixels, got {}".format(a.numel()))
    return _dev(a, names[0], dtype), _dev(b, names[1], dtype), a.numel(), a.shape[1] * a.shape[2]


def mask_confusion(predicted_u8, actual_u8, classes, stitched=False, ignore=None):
    """Two uint8 [B, H, W] class-index rasters -> (int64 [G, C, C], int64 [G]): per tile (G = B), or with ``stitched`` for the one
    raster the B tiles form (G = 1), ``counts[g][a][p]`` = the pixels with actual == a and predicted == p, and the number of pixels
    where either value is no class of 0 .. ``classes`` - 1 (they are in no cell).  2 <= ``classes`` <= 8.

    With ``ignore`` (``rs_eval_confusion_ig``) a third tensor follows, int64 [G]: the pixels whose ACTUAL value is ``ignore`` over a
    predicted value that is a class.  They are in no cell and not among the bad ones."""

    classes = int(classes)
    if not 2 <= classes <= EVAL_MAX_CLASSES:
        raise ValueError("robosat_amd: 2 to {} classes are counted, got {}".format(EVAL_MAX_CLASSES, classes))
    ignore = _ignore_label(ignore, classes)
    p, a, pixels, hw = _eval_pair(predicted_u8, actual_u8, ("predicted", "actual"), torch.uint8)
    groups = 1 if stitched else predicted_u8.shape[0]
    if ignore is not None:
        cc = groups * classes * classes
        three = torch.empty(cc + 2 * groups, device=predicted_u8.device, dtype=torch.int64)
        counts, bad, ignored = three[:cc].view(groups, classes, classes), three[cc:cc + groups], three[cc + groups:]
        _call("rs_eval_confusion_ig", p, a, _dev(counts, "counts", torch.int64), _dev(bad, "bad", torch.int64),
              _dev(ignored, "ignored", torch.int64), pixels, pixels if stitched else hw, classes, _stream(), ignore)
        return counts, bad, ignored
    # (one buffer, `bad` behind `counts`: the library then zeroes both with one fill)
    both = torch.empty(groups * (classes * classes + 1), device=predicted_u8.device, dtype=torch.int64)
    counts, bad = both[:groups * classes * classes].view(groups, classes, classes), both[groups * classes * classes:]
    _call("rs_eval_confusion", p, a, _dev(counts, "counts", torch.int64), _dev(bad, "bad", torch.int64), pixels,
          pixels if stitched else hw, classes, _stream())
    return counts, bad


def prob_histogram(prob_u8, actual_u8, classes, cls, stitched=False, ignore=None):
    """The probability bytes of class ``cls`` (what ``rs predict`` stores: byte q stands for q / 255) and the labels, both uint8
    [B, H, W] -> (hist int64 [G, 2, 256], bad int64 [G], ignored int64 [G]): per tile (G = B), or with ``stitched`` for the one
    raster the B tiles form (G = 1), ``hist[g][pos][q]`` = the pixels with byte q and (label == cls) == pos among the pixels whose
    label is a class of 0 .. ``classes`` - 1; ``bad``: the pixels whose label is no class and not ``ignore``; ``ignored``: those
    whose label is ``ignore`` (all zero without one).  Neither kind is in a cell.  2 <= ``classes`` <= 8, 1 <= ``cls`` < ``classes``
    (``rs_eval_prob_hist``)."""

    classes = int(classes)
    if not 2 <= classes <= EVAL_MAX_CLASSES:
        raise ValueError("robosat_amd: 2 to {} classes are counted, got {}".format(EVAL_MAX_CLASSES, classes))
    if isinstance(cls, bool) or int(cls) != cls or not 1 <= int(cls) < classes:
        raise ValueError("robosat_amd: the class of the probabilities is a non-background one, 1..{}, got {!r}".format(classes - 1, cls))
    ignore = _ignore_label(ignore, classes)
    q, a, pixels, hw = _eval_pair(prob_u8, actual_u8, ("prob", "actual"), torch.uint8)
    groups = 1 if stitched else prob_u8.shape[0]
    # (one buffer, `skipped` behind `hist`: the library then zeroes both with one fill)
    both = torch.empty(groups * 514, device=prob_u8.device, dtype=torch.int64)
    hist, skipped = both[:groups * 512].view(groups, 2, 256), both[groups * 512:].view(groups, 2)
    _call("rs_eval_prob_hist", q, a, _dev(hist, "hist", torch.int64), _dev(skipped, "skipped", torch.int64), pixels,
          pixels if stitched else hw, classes, int(cls), -1 if ignore is None else ignore, _stream())
    return hist, skipped[:, 0], skipped[:, 1]


def boundary_counts(d2_a, d2_b, d, stitched=False, coded=None):
    """Two int32 [B, H, W] rasters of ``distance_transform(mask, d + 1)`` (with ``nbr`` for ``stitched``) -> int64 [G, 3]: per tile,
    or with ``stitched`` for the one raster the B tiles form, the pixels in the first mask's band, in the second's and in both.  A
    mask's band is its pixels with 1 <= d2 <= d*d: those within ``d`` pixels of an unset pixel of the raster; the raster's edge is
    no boundary.  1 <= ``d`` <= 127.

    With ``coded`` (uint8 [B, H, W], a coded plane of ``select_known``, the transforms being those of the two coded planes) a pixel
    whose byte is 2 is unknown and in neither band (``rs_eval_boundary_coded``)."""

    d = int(d)
    if not 1 <= d <= EVAL_MAX_DISTANCE:
        raise ValueError("robosat_amd: the boundary band's distance is in 1..{}, got {}".format(EVAL_MAX_DISTANCE, d))
    a, b, pixels, hw = _eval_pair(d2_a, d2_b, ("d2_a", "d2_b"), torch.int32)
    if coded is not None and (coded.shape != d2_a.shape or coded.device != d2_a.device):
        raise ValueError("robosat_amd: coded is [B, H, W] like the transforms and on their device, got {} on {}".format(tuple(coded.shape), coded.device))
    counts = torch.empty((1 if stitched else d2_a.shape[0], 3), device=d2_a.device, dtype=torch.int64)
    if coded is None:
        _call("rs_eval_boundary", a, b, _dev(counts, "counts", torch.int64), pixels, pixels if stitched else hw, d, _stream())
    else:
        _call("rs_eval_boundary_coded", a, b, _dev(coded, "coded", torch.uint8), _dev(counts, "counts", torch.int64), pixels,
              pixels if stitched else hw, d, _stream())
    return counts


def select_known(predicted_u8, actual_u8, index, ignore, classes):
    """``rs evaluate --type --ignored unknown``: two uint8 [B, H, W] class-index rasters, the class ``index`` (1 .. ``classes`` - 1)
    and the ``ignore`` label (``classes`` .. 255) -> (coded_p, coded_g, mask_p, mask_g), uint8 [B, H, W] each.  With U = (actual ==
    ignore): coded_p is 2 on U, 1 where predicted == index outside U, 0 elsewhere; coded_g the same with actual == index; mask_p =
    (coded_p == 1), mask_g = (coded_g == 1) as 0/1 bytes.  One launch (``rs_eval_select``) in place of two ``clean_masks``."""

    classes = int(classes)
    if not 2 <= classes <= EVAL_MAX_CLASSES:
        raise ValueError("robosat_amd: 2 to {} classes are counted, got {}".format(EVAL_MAX_CLASSES, classes))
    if isinstance(index, bool) or int(index) != index or not 1 <= int(index) < classes:
        raise ValueError("robosat_amd: the class to select is a non-background one, 1..{}, got {!r}".format(classes - 1, index))
    ignore = _ignore_label(ignore, classes)
    if ignore is None:
        raise ValueError("robosat_amd: select_known codes the pixels of an ignore label; without one the masks are clean_masks'")
    p, a, pixels, _ = _eval_pair(predicted_u8, actual_u8, ("predicted", "actual"), torch.uint8)
    coded_p, coded_g, mask_p, mask_g = (torch.empty_like(predicted_u8, memory_format=torch.contiguous_format) for _ in range(4))
    _call("rs_eval_select", p, a, _dev(coded_p, "coded_p", torch.uint8), _dev(coded_g, "coded_g", torch.uint8),
          _dev(mask_p, "mask_p", torch.uint8), _dev(mask_g, "mask_g", torch.uint8), pixels, classes, int(index), ignore, _stream())
    return coded_p, coded_g, mask_p, mask_g


# ---- rs evaluate --centerline: the buffer method on two skeletons (rs_eval_centerline; definitions in include/robosat_hip.h) -------
EVAL_MAX_RHO = EDT_MAX_RADIUS - 1  # the tolerance rho: the transforms behind it have the radius rho + 1


def centerline_counts(skel_p, skel_g, rho, nbr=None):
    """Two uint8 [B, H, W] skeletons (``thin_masks`` of the predicted and the actual mask; non-zero = set) -> int64 [G, 8]: per tile
    (G = B), or with ``nbr`` int32 [B, 8] for the one sparse raster the tiles form (G = 1), the links of either skeleton by
    ``skeleton_links``' rule and those whose two end pixels both lie within ``rho`` pixels of the other skeleton:
    (p_straight, p_diag, p_straight_matched, p_diag_matched, g_straight, g_diag, g_straight_matched, g_diag_matched).  "Within
    ``rho``" is ``distance_transform(complement of the skeleton, rho + 1, nbr) <= rho^2``, so nothing beyond the raster's edge or in
    an absent tile is near.  1 <= ``rho`` <= 127; with ``nbr`` ``rho + 1`` fits min(H, W) (the transform says so)."""

    rho = int(rho)
    if not 1 <= rho <= EVAL_MAX_RHO:
        raise ValueError("robosat_amd: the centerline tolerance is in 1..{}, got {}".format(EVAL_MAX_RHO, rho))
    p, g, _, _ = _eval_pair(skel_p, skel_g, ("skel_p", "skel_g"), torch.uint8)
    b, h, w = skel_p.shape
    if nbr is not None and (nbr.shape != (b, 8) or nbr.device != skel_p.device):
        raise ValueError("robosat_amd: nbr is [T, 8] on the skeletons' device, got {} on {}".format(tuple(nbr.shape), nbr.device))
    # (the complement is glue: a skeleton is 0/1 bytes, and a byte compare keeps "non-zero = set" for any other)
    d2_to_p = distance_transform((skel_p == 0).to(torch.uint8), rho + 1, nbr)
    d2_to_g = distance_transform((skel_g == 0).to(torch.uint8), rho + 1, nbr)
    counts = torch.empty((b if nbr is None else 1, 8), device=skel_p.device, dtype=torch.int64)
    _call("rs_eval_centerline", p, g, _dev(d2_to_g, "d2_to_g", torch.int32), _dev(d2_to_p, "d2_to_p", torch.int32),
          _dev(nbr, "nbr", torch.int32), _dev(counts, "counts", torch.int64), b, h, w, rho, _stream())
    return counts


# ---- the optimiser step of rs train (csrc/optim.hip; definitions in include/robosat_hip.h, the optimizer in robosat_amd/optim.py) ----
class _OptimItem(ctypes.Structure):  # rs_optim_item (include/robosat_hip.h)
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("s", ctypes.c_void_p),
                ("numel", ctypes.c_long), ("decay", ctypes.c_int), ("reserved", ctypes.c_int)]


OPTIM_CTL_BYTES = 32  # int64 step @ 0, double sumsq @ 8, float coef @ 16


def optim_limits():
    """``(RS_OPTIM_CHUNK, RS_OPTIM_ITEMS)``: the elements one block walks per item chunk, the items one launch carries."""

    chunk, items = ctypes.c_int(0), ctypes.c_int(0)
    _call("rs_optim_limits", ctypes.byref(chunk), ctypes.byref(items))
    return chunk.value, items.value


def _storage_order(t):
    """The (size, stride) pairs of ``t`` from the outermost to the innermost dimension in memory, after checking that ``t`` covers
    its storage range densely: what makes an element-wise pass over raw pointers legal (a KRSC weight and its gradient, a vector)."""

    dims = sorted(((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1), reverse=True)
    want = 1
    for st, sz in reversed(dims):
        if st != want:
            raise ValueError("robosat_amd: an optimizer tensor must be dense in memory, got shape {} strides {}".format(
                tuple(t.shape), t.stride()))
        want *= sz
    return tuple(dims)


def optim_items(entries):
    """The host array of ``rs_optim_item`` for ``entries`` = ``(p, g, m, v, s | None, decay)`` tensors per parameter: fp32, on one
    device, dense and in one memory order per entry (a channels-last weight with its KRSC gradient is; nothing is copied).
    Returns ``(items, total_chunks)``; the array holds raw addresses, so the tensors must outlive its use."""

    chunk, _ = optim_limits()
    items = (_OptimItem * len(entries))()
    chunks = 0
    for i, (p, g, m, v, s, decay) in enumerate(entries):
        order = _storage_order(p)
        for name, t in (("p", p), ("g", g), ("m", m), ("v", v), ("s", s)):
            if t is None and name == "s":
                continue
            if not t.is_cuda or t.device != p.device:
                raise RuntimeError("robosat_amd: optimizer `{}` is on {} -- the step only runs on the MI355X".format(name, t.device))
            if t.dtype != torch.float32:
                raise TypeError("robosat_amd: optimizer `{}` must be torch.float32, got {}".format(name, t.dtype))
            if t.numel() != p.numel() or _storage_order(t) != order:
                raise ValueError("robosat_amd: optimizer `{}` {} / {} is not laid out like its parameter {} / {}".format(
                    name, tuple(t.shape), t.stride(), tuple(p.shape), p.stride()))
        items[i] = _OptimItem(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None if s is None else s.data_ptr(),
                              p.numel(), int(bool(decay)), 0)
        chunks += (p.numel() + chunk - 1) // chunk
    return items, chunks


def optim_workspace_bytes(total_chunks):
    nbytes = _lib.lib().rs_optim_workspace_bytes(int(total_chunks))
    if nbytes <= 0:
        raise ValueError("rs_optim_workspace_bytes: invalid arguments")
    return nbytes


def optim_grad_norm(items, clip, ctl, workspace):
    """``ctl.sumsq`` = the float64 sum of squares of every item's gradient, ``ctl.coef`` = min(1, clip / (norm + 1e-6)); ``workspace``:
    uint8, at least ``optim_workspace_bytes(total chunks of the items)``."""

    _call("rs_optim_grad_norm", items, len(items), ctypes.c_float(clip), _dev(ctl, "ctl", torch.uint8),
          _dev(workspace, "workspace", torch.uint8), _stream())


def optim_step(items, table, ctl, beta1, beta2, eps, use_coef):
    """One AdamW step of every item with row ``ctl.step`` of ``table`` (fp32 [T, 4]); then ``ctl.step`` += 1."""

    if table.dim() != 2 or table.shape[1] != 4:
        raise ValueError("robosat_amd: the schedule table is [T, 4], got {}".format(tuple(table.shape)))
    _call("rs_optim_step", items, len(items), _dev(table, "table"), table.shape[0], _dev(ctl, "ctl", torch.uint8),
          ctypes.c_float(beta1), ctypes.c_float(beta2), ctypes.c_float(eps), int(bool(use_coef)), _stream())
