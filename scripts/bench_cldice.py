"""Loss forward + backward at the train leg's shape (N = 32, C = 2, 512 x 512, fp32) with and without the clDice term
(profiles/cldice/README.md).  Times are device events around ``--steps`` passes after ``--warmup``; kernel times come from running the
``native`` variant under ``rocprofv3 --kernel-trace --stats``, a process of its own.

    python scripts/bench_cldice.py --variant ce                       # rs_nll_loss_fwd + rs_nll_loss_bwd through the C ABI
    python scripts/bench_cldice.py --variant ce --lib parent/librobosat_hip.so
    python scripts/bench_cldice.py --variant native --iters 10        # ClDiceLoss2d(CrossEntropyLoss2d): the kernels of csrc/cldice.hip
    python scripts/bench_cldice.py --variant torch --iters 10         # the same loss with the term composed from torch's GPU ops + autograd
    python scripts/bench_cldice.py --variant compare --iters 10       # native and torch alternating, --rounds times each, in one process
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def road_labels(n, h, w, seed=0):
    """int64 [n, h, w]: four to eight straight roads per tile, 5 to 13 pixels wide, at any angle."""

    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    t = np.zeros((n, h, w), dtype=np.int64)
    for i in range(n):
        for _ in range(int(rng.integers(4, 9))):
            angle, half = rng.uniform(0, np.pi), rng.uniform(2.5, 6.5)
            x0, y0 = rng.uniform(0, w), rng.uniform(0, h)
            dist = np.abs((xx - x0) * np.sin(angle) - (yy - y0) * np.cos(angle))
            t[i][dist <= half] = 1
    return torch.from_numpy(t)


def logits_for(t, c, seed=0):
    """Logits of a half-trained network: the labels blurred and scaled, plus smooth noise."""

    g = torch.Generator().manual_seed(seed)
    n, h, w = t.shape
    onehot = F.one_hot(t, c).permute(0, 3, 1, 2).float()
    noise = F.avg_pool2d(torch.randn(n, c, h, w, generator=g), 5, 1, 2) * 4
    return (F.avg_pool2d(onehot, 5, 1, 2) * 4 + noise).contiguous()


def torch_cldice(x, t, iters, smooth=1.0):
    """The clDice term of include/robosat_hip.h from torch's own GPU ops, for autograd."""

    n, c, h, w = x.shape
    p = torch.softmax(x, 1)[:, 1:].reshape(n * (c - 1), h, w)
    y = torch.stack([(t == k).float() for k in range(1, c)], 1).reshape(n * (c - 1), h, w)

    def erode(a):
        return torch.minimum(-F.max_pool2d(-a, (3, 1), (1, 1), (1, 0)), -F.max_pool2d(-a, (1, 3), (1, 1), (0, 1)))

    def skel(a):
        s = None
        for _ in range(iters + 1):
            nxt = erode(a)
            d = F.relu(a - F.max_pool2d(nxt, 3, 1, 1))
            s = d if s is None else s + F.relu(d - s * d)
            a = nxt
        return s

    sp = skel(p)
    with torch.no_grad():
        sy = skel(y)
    tprec = ((sp * y).sum((1, 2)) + smooth) / (sp.sum((1, 2)) + smooth)
    tsens = ((sy * p).sum((1, 2)) + smooth) / (sy.sum((1, 2)) + smooth)
    return (1 - 2 * tprec * tsens / (tprec + tsens)).mean()


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        step()
    stop.record()
    torch.cuda.synchronize()
    return round(start.elapsed_time(stop) * 1000.0 / steps, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["ce", "native", "torch", "compare"], required=True)
    ap.add_argument("--lib", default=os.path.join(ROOT, "robosat_amd", "librobosat_hip.so"))
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--c", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--a", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cldice: needs the MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    n, c, h, w = args.n, args.c, args.size, args.size
    t_cpu = road_labels(n, h, w)
    t = t_cpu.to(dev)
    x = logits_for(t_cpu, c).to(dev)
    out = {"variant": args.variant, "shape": [n, c, h, w], "iters": args.iters, "a": args.a,
           "road_pixels": round(float((t > 0).float().mean()), 4)}

    if args.variant == "ce":
        lib = ctypes.CDLL(args.lib, mode=ctypes.RTLD_GLOBAL)
        p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        weight = torch.ones(c, device=dev)
        loss, stats, dx = torch.zeros((), device=dev), torch.zeros(2, device=dev), torch.empty_like(x)
        lws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        gamma = ctypes.c_float(2.0)

        def step():
            for rc in (lib.rs_nll_loss_fwd(p(x), p(t), p(weight), p(loss), p(stats), n, c, h, w, 0, gamma, p(lws), stream),
                       lib.rs_nll_loss_bwd(p(x), p(t), p(weight), p(stats), None, p(dx), n, c, h, w, 0, gamma, stream)):
                if rc:
                    sys.exit("bench_cldice: status {}".format(rc))

        out.update({"lib": os.path.relpath(args.lib, ROOT), "us_per_pass": timed(step, args.steps, args.warmup), "loss": float(loss)})
        print(json.dumps(out))
        return

    from robosat_amd.losses import ClDiceLoss2d, CrossEntropyLoss2d

    base = CrossEntropyLoss2d().to(dev)
    crit = ClDiceLoss2d(base, args.a, iters=args.iters).to(dev)
    xg = x.clone().requires_grad_(True)
    last = {}

    def native():
        xg.grad = None
        loss = crit(xg, t)
        loss.backward()
        last["native"] = loss

    def composed():
        xg.grad = None
        loss = (1.0 - args.a) * base(xg, t) + args.a * torch_cldice(xg, t, args.iters)
        loss.backward()
        last["torch"] = loss

    if args.variant == "native":
        out["us_per_pass"] = timed(native, args.steps, args.warmup)
    elif args.variant == "torch":
        out["us_per_pass"] = timed(composed, args.steps, args.warmup)
    else:
        rounds = {"native": [], "torch": []}
        for _ in range(args.rounds):
            rounds["native"].append(timed(native, args.steps, args.warmup))
            rounds["torch"].append(timed(composed, args.steps, args.warmup))
        native()
        g_native = xg.grad.clone()
        composed()
        out.update({"us_per_pass": rounds, "max_abs_grad_difference": float((xg.grad - g_native).abs().max()),
                    "max_abs_grad": float(g_native.abs().max())})
    out["loss"] = {k: float(v) for k, v in last.items()}
    out["peak_memory_MB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
