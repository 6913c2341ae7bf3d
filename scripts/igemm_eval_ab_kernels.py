"""Per-launch times (us) of the fp32 direct-form implicit-GEMM launches of the predict pass (conv_igemm_dma_kernel.h, EPI_EVAL) alone on
the chip, at bs 16 of the 512^2 benchmark: the 15 distinct shapes of the encoder's layer2 .. layer4 with the epilogue each runs with
(conv1 / conv2: scale + shift + ReLU; conv3: + residual; downsample: scale + shift) and how often the pass launches it -- HIP events
around 20 launches, median [min-max] of 9 rounds; the last column weights the medians by those counts.  The library is whatever
ROBOSAT_HIP_LIB names, else the tree's: run from the repository root once per library, alternately (profiles/igemm_eval_tile/ab_steps.txt)."""
import os
import sys

import torch

sys.path.insert(0, ".")
from robosat_amd import ops  # noqa: E402

DEV = "cuda:0"
# (cin, cout, k, stride, output size, kind, launches per pass)
SHAPES = (
    (256, 128, 1, 1, 128, "relu", 1), (128, 128, 3, 2, 64, "relu", 1), (256, 512, 1, 2, 64, "affine", 1), (128, 512, 1, 1, 64, "res", 4),
    (512, 128, 1, 1, 64, "relu", 3), (512, 256, 1, 1, 64, "relu", 1), (256, 256, 3, 2, 32, "relu", 1), (512, 1024, 1, 2, 32, "affine", 1),
    (256, 1024, 1, 1, 32, "res", 6), (1024, 256, 1, 1, 32, "relu", 5), (1024, 512, 1, 1, 32, "relu", 1), (512, 512, 3, 2, 16, "relu", 1),
    (1024, 2048, 1, 2, 16, "affine", 1), (512, 2048, 1, 1, 16, "res", 3), (2048, 512, 1, 1, 16, "relu", 2),
)


def operands(n, cin, cout, k, stride, ho, kind, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    hs = ho * stride
    x = torch.randn(n, hs, hs, cin, device=DEV, generator=g)
    w = torch.randn(cout, k, k, cin, device=DEV, generator=g) * (2.0 / (k * k * cin)) ** 0.5
    sc, sh = torch.rand(cout, device=DEV, generator=g) + 0.5, torch.randn(cout, device=DEV, generator=g)
    kw = dict(stride=stride, pad=k // 2, scale=sc, shift=sh, relu=kind != "affine")
    if kind == "res":
        kw["residual"] = torch.randn(n, ho, ho, cout, device=DEV, generator=g)
    return x, w, kw


def timed(fn, reps=20, rounds=9):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps * 1000.0)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


if __name__ == "__main__":
    tag = os.environ.get("ROBOSAT_HIP_LIB", "tree").split("/")[-2:]
    out, total = [], 0.0
    for cin, cout, k, stride, ho, kind, count in SHAPES:
        x, w, kw = operands(16, cin, cout, k, stride, ho, kind)
        o = torch.empty(16, ho, ho, cout, device=DEV)
        med, lo, hi = timed(lambda: ops.conv2d(x, w, out=o, **kw))
        total += count * med
        out.append("{}>{}k{}s{}@{}{} {:.1f} [{:.1f}-{:.1f}]".format(cin, cout, k, stride, ho, "+res" if kind == "res" else "", med, lo, hi))
        del x, w, kw, o
    print("/".join(tag), " ".join(out), "| {} launches of the pass {:.1f} us".format(sum(s[-1] for s in SHAPES), total))
