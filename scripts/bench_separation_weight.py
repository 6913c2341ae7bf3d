"""Loss forward + backward at the train leg's shape (N = 32, C = 2, 512 x 512) with and without the separation weight
(profiles/separation_weight/README.md).  Through the C ABI by ctypes, binding only what a variant calls, so that the parent commit's
library runs from the same script (``--lib``).  Times are device events around ``--steps`` passes after ``--warmup``; kernel times
come from running this script under ``rocprofv3 --kernel-trace --stats``, a process of its own per variant.

    python scripts/bench_separation_weight.py --variant plain                      # rs_nll_loss_fwd + rs_nll_loss_bwd
    python scripts/bench_separation_weight.py --variant plain --lib parent/librobosat_hip.so
    python scripts/bench_separation_weight.py --variant boundary                   # rs_boundary_weight_plane + rs_nll_loss_*_pw (the yardstick)
    python scripts/bench_separation_weight.py --variant separation                 # rs_separation_weight_plane + rs_nll_loss_*_pw
    python scripts/bench_separation_weight.py --variant both                       # boundary plane, separation onto it, rs_nll_loss_*_pw
    python scripts/bench_separation_weight.py --variant separation --labels blocks # rows of houses three pixels apart instead of rectangles
"""

import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def labels(n, h, w, kind, seed=0):
    """int64 [n, h, w].  ``rectangles``: one to three rectangles per tile, as the synthetic training tiles have them (tests/synth.py,
    and scripts/bench_boundary_weight.py).  ``blocks``: houses of 20 x 28 pixels in rows, three pixels apart within a row and twelve
    between rows, every tile shifted by an offset of its own: every house has a neighbour in reach."""

    rng = np.random.default_rng(seed)
    t = np.zeros((n, h, w), dtype=np.int64)
    for i in range(n):
        if kind == "rectangles":
            for _ in range(int(rng.integers(1, 4))):
                bw, bh = rng.integers(w // 8, w // 2), rng.integers(h // 8, h // 2)
                x0, y0 = rng.integers(0, w - bw), rng.integers(0, h - bh)
                t[i, y0:y0 + bh, x0:x0 + bw] = 1
        else:
            oy, ox = int(rng.integers(0, 32)), int(rng.integers(0, 31))
            for y0 in range(oy, h - 20, 32):
                for x0 in range(ox, w - 28, 31):
                    t[i, y0:y0 + 20, x0:x0 + 28] = 1
    return torch.from_numpy(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["plain", "boundary", "separation", "both"], required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "robosat_amd", "librobosat_hip.so"))
    ap.add_argument("--labels", choices=["rectangles", "blocks"], default="rectangles")
    ap.add_argument("--mode", type=int, default=0, help="0 CrossEntropy, 1 Focal")
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--c", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--w0", type=float, default=4.0)
    ap.add_argument("--boundary-sigma", type=float, default=3.0)
    ap.add_argument("--ws", type=float, default=10.0)
    ap.add_argument("--sigma", type=float, default=5.0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_separation_weight: needs the MI355X (no CPU path)")

    lib = ctypes.CDLL(args.lib, mode=ctypes.RTLD_GLOBAL)
    dev = torch.device("cuda", 0)
    n, c, h, w = args.n, args.c, args.size, args.size
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(n, c, h, w, generator=g) * 2).to(dev)
    t = labels(n, h, w, args.labels).to(dev)
    weight = torch.tensor([1.0, 2.5] + [1.0] * (c - 2))[:c].to(dev)
    loss, stats = torch.zeros((), device=dev), torch.zeros(2, device=dev)
    dx = torch.empty_like(x)
    r = int(math.ceil(3 * args.boundary_sigma))
    k = np.arange(r * r, dtype=np.float64)
    btable = torch.from_numpy((1.0 + args.w0 * np.exp(-k / (2.0 * args.boundary_sigma ** 2))).astype(np.float32)).to(dev)
    d = int(math.ceil(3 * args.sigma))
    k = np.arange(d * d, dtype=np.float64)
    stable = torch.from_numpy((args.ws * np.exp(-k / (2.0 * args.sigma ** 2))).astype(np.float32)).to(dev)
    base, plane = torch.ones(n, h, w, device=dev), torch.ones(n, h, w, device=dev)
    ws = torch.empty(max(1 << 20, 16 + 14 * n * h * w), dtype=torch.uint8, device=dev)
    lws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)  # (the loss's own: the labelling's err word stays readable in `ws`)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gamma = ctypes.c_float(2.0)

    def check(rc):
        if rc:
            sys.exit("bench_separation_weight: status {}".format(rc))

    def step():
        if args.variant == "plain":
            check(lib.rs_nll_loss_fwd(p(x), p(t), p(weight), p(loss), p(stats), n, c, h, w, args.mode, gamma, p(lws), stream))
            check(lib.rs_nll_loss_bwd(p(x), p(t), p(weight), p(stats), None, p(dx), n, c, h, w, args.mode, gamma, stream))
            return
        if args.variant == "boundary":
            check(lib.rs_boundary_weight_plane(p(t), p(btable), p(plane), n, c, h, w, r, -1, p(ws), stream))
        elif args.variant == "separation":
            check(lib.rs_separation_weight_plane(p(t), p(stable), None, p(plane), n, c, h, w, d, -1, p(ws), stream))
        else:
            check(lib.rs_boundary_weight_plane(p(t), p(btable), p(base), n, c, h, w, r, -1, p(ws), stream))
            check(lib.rs_separation_weight_plane(p(t), p(stable), p(base), p(plane), n, c, h, w, d, -1, p(ws), stream))
        check(lib.rs_nll_loss_fwd_pw(p(x), p(t), p(weight), p(loss), p(stats), n, c, h, w, args.mode, gamma, p(lws), stream, p(plane), -1))
        check(lib.rs_nll_loss_bwd_pw(p(x), p(t), p(weight), p(stats), None, p(dx), n, c, h, w, args.mode, gamma, stream, p(plane), -1))

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.steps):
        step()
    stop.record()
    torch.cuda.synchronize()
    lit = float((plane > (base if args.variant == "both" else 1)).float().mean()) if args.variant in ("separation", "both") else 0.0
    err = int(ws[:4].view(torch.int32).item()) if args.variant in ("separation", "both") else 0
    print(json.dumps({"variant": args.variant, "labels": args.labels, "lib": os.path.relpath(args.lib, ROOT), "mode": args.mode,
                      "shape": [n, c, h, w], "us_per_pass": round(start.elapsed_time(stop) * 1000.0 / args.steps, 2), "loss": float(loss),
                      "object_pixels": round(float((t > 0).float().mean()), 4), "pixels_with_a_term": round(lit, 4), "label_err": err}))


if __name__ == "__main__":
    main()
