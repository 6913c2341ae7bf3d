"""Per-launch times (us) of the fp32 Winograd DecoderBlock launches (conv_wino_f32.hip) alone on the chip: the five decoder shapes of the
predict pass at bs 16 and the data gradients the fp32 train step runs in this form at bs 8 -- HIP events around 20 launches, median
[min-max] of 9 rounds.  The library is whatever ROBOSAT_HIP_LIB names, else the tree's: run from the repository root once per library,
alternately (profiles/wino_items/ab_steps.txt)."""
import os
import sys

import torch

sys.path.insert(0, ".")
from robosat_amd import ops  # noqa: E402

DEV = "cuda:0"
g = torch.Generator(device=DEV).manual_seed(0)
LAYERS = (("dec0", 2048, 256, 256, 16), ("dec1", 1024, 256, 256, 32), ("dec2", 512, 256, 64, 64), ("dec3", 256, 64, 128, 128), ("dec4", 128, 0, 32, 256))


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
for name, c1, c2, cout, hs in LAYERS:
    a = torch.randn(16, hs, hs, c1, device=DEV, generator=g)
    b = torch.randn(16, hs, hs, c2, device=DEV, generator=g) if c2 else None
    u = ops.pack_wino_phase_weight(ops.pack_phase_weight(torch.randn(cout, 3, 3, c1 + c2, device=DEV, generator=g) * 0.02))
    out.append((name,) + timed(lambda: ops.conv2d_phase_wino(a, u, src2=b, relu=True, upsampled=True)))
    del a, b, u
fwd = sum(o[1] for o in out)
ndg = 0
for name, c1, c2, cout, hs in LAYERS:
    if not ops.wino_dgrad_ok(8, hs, hs, c1, c2, cout):
        continue
    dz = torch.randn(8, 2 * hs, 2 * hs, cout, device=DEV, generator=g)
    u = ops.pack_wino_dgrad_weight(ops.pack_dgrad_phase_weight(torch.randn(cout, 3, 3, c1 + c2, device=DEV, generator=g) * 0.02))
    mask = torch.randn(8, hs, hs, c1 + c2, device=DEV, generator=g)
    out.append(("dg." + name,) + timed(lambda: ops.conv2d_dgrad_phase_wino(dz, u, c1, c2, mask1=mask)))
    ndg += 1
    del dz, u, mask
print(tag, " ".join("{} {:.1f} [{:.1f}-{:.1f}]".format(*o) for o in out),
      "| 5 decoder launches {:.1f} us, {} dgrads {:.1f} us".format(fwd, ndg, sum(o[1] for o in out[5:])))
