"""sha256 of the outputs of the fp32 direct-form EPI_EVAL launches of the implicit GEMM (conv_igemm_dma_kernel.h) on Gaussian operands:
the shapes of tests/test_gpu_igemm_eval_tile.py (M = 81 and 429, Cin 32 / 64 / 96, Cout 32 .. 160, the four fp32 tiles at both row sizes,
plain 1x1 and the launches that keep the gather table, every epilogue kind) and the 15 distinct launch shapes of the predict pass at bs 2
with the epilogue each runs with, on the dispatcher's own choice.  The library is whatever ROBOSAT_HIP_LIB names, else the tree's: run from
the repository root once per library and diff the two listings (profiles/igemm_eval_tile/hashes.txt)."""
import hashlib
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "scripts")
from robosat_amd import ops  # noqa: E402
from igemm_eval_ab_kernels import SHAPES, operands  # noqa: E402

DEV = "cuda:0"


def h(name, t):
    torch.cuda.synchronize()
    print(name, hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:24], tuple(t.shape))


def kinds(n, ho, wo, cout, g):
    sc, sh = torch.rand(cout, device=DEV, generator=g) + 0.5, torch.randn(cout, device=DEV, generator=g)
    res, mask = torch.randn(n, ho, wo, cout, device=DEV, generator=g), torch.randn(n, ho, wo, cout, device=DEV, generator=g)
    return (("none", {}), ("affine", dict(scale=sc, shift=sh)), ("relu", dict(scale=sc, shift=sh, relu=True)),
            ("res+relu", dict(scale=sc, shift=sh, residual=res, relu=True)), ("res", dict(residual=res)), ("mask", dict(relu_mask=mask)),
            ("res+mask", dict(residual=res, relu_mask=mask)))


# (kernel size, stride, pad, two sources)
FORMS = ((1, 1, 0, False), (1, 2, 0, False), (3, 1, 1, False), (3, 2, 1, False), (1, 1, 0, True))
for tile in ("128x128", "128x64", "128x32", "64x64"):
    for rowb in (64, 128):
        for n, hh, ww in ((1, 9, 9), (3, 11, 13)):
            for cin in (32, 64, 96):
                for cout in (32, 96, 160, 64, 128):
                    for k, stride, pad, two in FORMS:
                        if (k, stride, two) != (1, 1, False) and (n == 1 or cin != 64 or cout in (32, 128)):
                            continue  # (the table forms: the larger M, one Cin, three Couts)
                        g = torch.Generator(device=DEV).manual_seed(1)
                        x = torch.randn(n, hh, ww, cin, device=DEV, generator=g)
                        w = torch.randn(cout, k, k, cin, device=DEV, generator=g) * (2.0 / (k * k * cin)) ** 0.5
                        src = dict(src1=x[..., :32].contiguous(), src2=x[..., 32:].contiguous()) if two and cin > 32 else dict(src1=x)
                        ho, wo = (hh + 2 * pad - k) // stride + 1, (ww + 2 * pad - k) // stride + 1
                        with ops.tuning(tile=tile, rowb=rowb):
                            for kind, opts in kinds(n, ho, wo, cout, g):
                                tag = "{} r{} {}x{}x{} {}>{} k{}s{}{} {}".format(tile, rowb, n, hh, ww, cin, cout, k, stride, " cat" if two else "", kind)
                                h(tag, ops.conv2d(weight=w, stride=stride, pad=pad, **src, **opts))
for cin, cout, k, stride, ho, kind, _ in SHAPES:
    x, w, kw = operands(2, cin, cout, k, stride, ho, kind, seed=2)
    h("bench bs2 {}>{} k{}s{}@{} {}".format(cin, cout, k, stride, ho, kind), ops.conv2d(x, w, **kw))
