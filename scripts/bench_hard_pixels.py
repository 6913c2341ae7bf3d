"""Loss forward + backward at the train leg's shape (N = 32, C = 2, 512 x 512) with and without hard-pixel mining
(profiles/hard_pixels/README.md).  Through the C ABI by ctypes, binding only what a variant calls, so that the parent commit's
library runs from the same script (``--lib``).  Times are device events around ``--steps`` passes after ``--warmup``; kernel times
come from running this script under ``rocprofv3 --kernel-trace --stats``, a process of its own per variant.

    python scripts/bench_hard_pixels.py --variant plain                       # rs_nll_loss_fwd + rs_nll_loss_bwd
    python scripts/bench_hard_pixels.py --variant plain --lib parent/librobosat_hip.so
    python scripts/bench_hard_pixels.py --variant hard --data uniform         # rs_hard_pixel_plane + rs_nll_loss_*_pw, random logits
    python scripts/bench_hard_pixels.py --variant hard --data skewed          # ... 99 % of the pixels confidently right
    python scripts/bench_hard_pixels.py --variant select --data skewed        # rs_hard_pixel_plane alone
"""

import argparse
import ctypes
import json
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def logits(n, c, h, w, targets, data, seed=0):
    """uniform: randn * 2.  skewed: 99 % of the pixels predict their label with margin 12 + |randn| * 4 (a cross-entropy between 0 --
    exactly 0 in float32 beyond a margin of about 17 -- and 1e-5), the others are random."""

    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g) * 2
    if data == "skewed":
        sure = torch.rand(n, h, w, generator=g) < 0.99
        margin = 12 + torch.randn(n, h, w, generator=g).abs() * 4
        hot = torch.zeros(n, c, h, w).scatter_(1, targets.unsqueeze(1), 1.0)
        x = torch.where(sure.unsqueeze(1), x * 0.1 + hot * margin.unsqueeze(1), x)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["plain", "hard", "select"], required=True)
    ap.add_argument("--data", choices=["uniform", "skewed"], default="uniform")
    ap.add_argument("--lib", default=os.path.join(ROOT, "robosat_amd", "librobosat_hip.so"))
    ap.add_argument("--mode", type=int, default=0, help="0 CrossEntropy, 1 Focal")
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--c", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--fraction", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hard_pixels: needs the MI355X (no CPU path)")

    lib = ctypes.CDLL(args.lib, mode=ctypes.RTLD_GLOBAL)
    dev = torch.device("cuda", 0)
    n, c, h, w = args.n, args.c, args.size, args.size
    g = torch.Generator().manual_seed(1)
    t_host = torch.randint(0, c, (n, h // 8, w // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    x = logits(n, c, h, w, t_host, args.data).to(dev)
    t = t_host.to(dev)
    weight = torch.tensor([1.0, 2.5] + [1.0] * (c - 2))[:c].to(dev)
    loss, stats = torch.zeros((), device=dev), torch.zeros(2, device=dev)
    dx = torch.empty_like(x)
    plane = torch.ones(n, h, w, device=dev)
    info = torch.zeros(n, 4, dtype=torch.int64, device=dev)
    nbytes = 1 << 20
    if args.variant != "plain":
        lib.rs_hard_pixel_workspace_bytes.restype = ctypes.c_long
        nbytes = max(nbytes, lib.rs_hard_pixel_workspace_bytes(n, h, w))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gamma = ctypes.c_float(2.0)
    fraction_bits = ctypes.c_long(struct.unpack("<q", struct.pack("<d", args.fraction))[0])  # the double's 64 bits

    def check(rc):
        if rc:
            sys.exit("bench_hard_pixels: status {}".format(rc))

    def step():
        if args.variant == "plain":
            check(lib.rs_nll_loss_fwd(p(x), p(t), p(weight), p(loss), p(stats), n, c, h, w, args.mode, gamma, p(ws), stream))
            check(lib.rs_nll_loss_bwd(p(x), p(t), p(weight), p(stats), None, p(dx), n, c, h, w, args.mode, gamma, stream))
            return
        check(lib.rs_hard_pixel_plane(p(x), p(t), None, p(plane), None, p(info), n, c, h, w, fraction_bits,
                                      ctypes.c_long(0xFFFFFFFF), -1, p(ws), stream))
        if args.variant == "select":
            return
        check(lib.rs_nll_loss_fwd_pw(p(x), p(t), p(weight), p(loss), p(stats), n, c, h, w, args.mode, gamma, p(ws), stream, p(plane), -1))
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
    out = {"variant": args.variant, "data": args.data, "lib": os.path.relpath(args.lib, ROOT), "mode": args.mode, "shape": [n, c, h, w],
           "us_per_pass": round(start.elapsed_time(stop) * 1000.0 / args.steps, 2), "loss": float(loss)}
    if args.variant != "plain":
        out.update({"fraction": args.fraction, "info_image0": info[0].tolist(), "kept_share": round(float(plane.mean()), 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
