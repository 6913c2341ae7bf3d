"""Loss forward + backward at the train leg's shape (N = 32, C = 2, 512 x 512) with and without boundary label relaxation
(profiles/relax/README.md).  Through the C ABI by ctypes, binding only what a variant calls, so that the parent commit's library runs
from the same script (``--lib``).  Times are device events around ``--steps`` passes after ``--warmup``; kernel times come from
running this script under ``rocprofv3 --kernel-trace --stats``, a process of its own per variant.

    python scripts/bench_relax.py --variant plain                      # rs_nll_loss_fwd + rs_nll_loss_bwd
    python scripts/bench_relax.py --variant plain --lib parent/librobosat_hip.so
    python scripts/bench_relax.py --variant relax --radius 2           # rs_label_set_plane + rs_nll_loss_*_rx
    python scripts/bench_relax.py --variant relax --radius 16
    python scripts/bench_relax.py --variant planes --radius 2          # rs_label_set_plane beside rs_boundary_weight_plane, same labels:
                                                                       # under the kernel trace, label_set_kernel beside boundary_mask_kernel
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def labels(n, h, w, seed=0):
    """int64 [n, h, w]: one to three rectangles per tile, as the synthetic training tiles have them (tests/synth.py, and
    scripts/bench_boundary_weight.py)."""

    rng = np.random.default_rng(seed)
    t = np.zeros((n, h, w), dtype=np.int64)
    for i in range(n):
        for _ in range(int(rng.integers(1, 4))):
            bw, bh = rng.integers(w // 8, w // 2), rng.integers(h // 8, h // 2)
            x0, y0 = rng.integers(0, w - bw), rng.integers(0, h - bh)
            t[i, y0:y0 + bh, x0:x0 + bw] = 1
    return torch.from_numpy(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["plain", "relax", "planes"], required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "robosat_amd", "librobosat_hip.so"))
    ap.add_argument("--mode", type=int, default=0, help="0 CrossEntropy, 1 Focal")
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--c", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_relax: needs the MI355X (no CPU path)")

    lib = ctypes.CDLL(args.lib, mode=ctypes.RTLD_GLOBAL)
    dev = torch.device("cuda", 0)
    n, c, h, w = args.n, args.c, args.size, args.size
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(n, c, h, w, generator=g) * 2).to(dev)
    t = labels(n, h, w).to(dev)
    weight = torch.tensor([1.0, 2.5] + [1.0] * (c - 2))[:c].to(dev)
    loss, stats = torch.zeros((), device=dev), torch.zeros(2, device=dev)
    dx = torch.empty_like(x)
    sets = torch.zeros(n, h, w, dtype=torch.uint8, device=dev)
    plane = torch.ones(n, h, w, device=dev)
    btable = torch.ones(9 * 9, device=dev)  # (reach 9, the boundary weight's default sigma of 3; the values do not matter to the time)
    ws = torch.empty(max(1 << 20, 6 * n * h * w), dtype=torch.uint8, device=dev)
    lws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gamma = ctypes.c_float(2.0)

    def check(rc):
        if rc:
            sys.exit("bench_relax: status {}".format(rc))

    def set_plane():
        check(lib.rs_label_set_plane(p(t), p(sets), n, c, h, w, args.radius, -1, stream))

    def boundary_plane():
        check(lib.rs_boundary_weight_plane(p(t), p(btable), p(plane), n, c, h, w, 9, -1, p(ws), stream))

    def step():
        if args.variant == "plain":
            check(lib.rs_nll_loss_fwd(p(x), p(t), p(weight), p(loss), p(stats), n, c, h, w, args.mode, gamma, p(lws), stream))
            check(lib.rs_nll_loss_bwd(p(x), p(t), p(weight), p(stats), None, p(dx), n, c, h, w, args.mode, gamma, stream))
            return
        set_plane()
        check(lib.rs_nll_loss_fwd_rx(p(x), p(t), p(weight), p(loss), p(stats), n, c, h, w, args.mode, gamma, p(lws), stream, None, -1, p(sets)))
        check(lib.rs_nll_loss_bwd_rx(p(x), p(t), p(weight), p(stats), None, p(dx), n, c, h, w, args.mode, gamma, stream, None, -1, p(sets)))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.steps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return round(start.elapsed_time(stop) * 1000.0 / args.steps, 2)

    out = {"variant": args.variant, "lib": os.path.relpath(args.lib, ROOT), "mode": args.mode, "shape": [n, c, h, w]}
    if args.variant == "planes":
        out.update({"radius": args.radius, "set_plane_us": timed(set_plane), "boundary_plane_us": timed(boundary_plane)})
    else:
        out["us_per_pass"] = timed(step)
        out["loss"] = float(loss)
        if args.variant == "relax":
            out.update({"radius": args.radius, "pixels_with_two_classes": round(float((sets == 3).float().mean()), 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
