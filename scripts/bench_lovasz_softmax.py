"""Lovasz-Softmax (rs_lovasz_softmax_fwd) against the reference's Lovasz hinge (rs_lovasz_fwd): ms per forward + gradient,
device events around 20 calls after 3 warm-up calls, each form in turn.
usage: python scripts/bench_lovasz_softmax.py  (measurement tool; run it under rocprofv3 --kernel-trace --stats for the
per-kernel split)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from robosat_amd import ops

dev = torch.device("cuda:0")
REPS = 20


def timed(fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


for n, c, hw in ((32, 2, 512), (32, 4, 512)):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(n, c, hw, hw, generator=g) * 0.7).to(dev)
    t = torch.randint(0, c, (n, hw, hw), generator=g).to(dev)
    keys = n * c * hw * hw
    rows = [("lovasz (hinge, reference variant)", lambda: ops.lovasz_fwd(x, t)),
            ("lovasz_softmax per image", lambda: ops.lovasz_softmax_fwd(x, t, per_image=True)),
            ("lovasz_softmax flattened", lambda: ops.lovasz_softmax_fwd(x, t, per_image=False)),
            ("lovasz_softmax per image, loss only", lambda: ops.lovasz_softmax_fwd(x, t, per_image=True, want_grad=False))]
    for name, fn in rows:
        print("N {} C {} {}x{} ({:.1f} M keys)  {:<36s} {:.3f} ms".format(n, c, hw, hw, keys / 1e6, name, timed(fn)), flush=True)
