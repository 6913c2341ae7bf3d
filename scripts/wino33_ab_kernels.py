"""Per-launch times (us) of the benchmark's conv_wino33_f32 launches at bs 16 -- the Bottleneck conv2 shapes of layer1 .. layer4 and dec5 +
final + softmax -- alone on the chip: HIP events around 20 launches, median [min-max] of 9 rounds.  The library is whatever
ROBOSAT_HIP_LIB names, else the tree's: run from the repository root once per library, alternately (profiles/wino33_items/ab_steps.txt)."""
import os
import sys

import torch

sys.path.insert(0, ".")
from robosat_amd import ops  # noqa: E402

DEV = "cuda:0"
g = torch.Generator(device=DEV).manual_seed(0)


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


tag = os.path.basename(os.environ.get("ROBOSAT_HIP_LIB", "tree"))
out = []
for name, n, h, c, launches in (("layer1", 16, 128, 64, 3), ("layer2", 16, 64, 128, 3), ("layer3", 16, 32, 256, 5), ("layer4", 16, 16, 512, 2)):
    x = torch.randn(n, h, h, c, device=DEV, generator=g)
    u = ops.pack_wino33_weight(torch.randn(c, 3, 3, c, device=DEV, generator=g) * 0.05)
    sc, sh = torch.rand(c, device=DEV, generator=g), torch.randn(c, device=DEV, generator=g)
    med, lo, hi = timed(lambda: ops.conv2d_wino33(x, u, scale=sc, shift=sh, relu=True))
    out.append((name, med, lo, hi, launches))
x = torch.randn(16, 512, 512, 32, device=DEV, generator=g)
u = ops.pack_wino33_weight(torch.randn(32, 3, 3, 32, device=DEV, generator=g) * 0.05)
fw, fb = torch.randn(2, 32, device=DEV, generator=g), torch.randn(2, device=DEV, generator=g)
med, lo, hi = timed(lambda: ops.conv2d_wino33_head(x, u, fw, fb, "softmax"))
out.append(("dec5+final", med, lo, hi, 1))
tot13 = sum(m * k for nm, m, _, _, k in out[:4])
print(tag, " ".join("{} {:.1f} [{:.1f}-{:.1f}]".format(nm, m, lo, hi) for nm, m, lo, hi, _ in out), "| 13 conv2 launches {:.1f} us, head {:.1f} us".format(tot13, out[4][1]))
