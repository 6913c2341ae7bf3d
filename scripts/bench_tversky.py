"""Loss forward + backward of the Tversky family beside the losses it is measured against (profiles/tversky/README.md), at
N = 32, 512 x 512 fp32 with C = 2 and C = 4, in ONE process with the variants alternating inside every round:

    tversky0   rs_tversky_sums + rs_tversky_finalize + rs_tversky_bwd, lambda = 0 (Dice, per image, classes present)
    miou       rs_miou_loss_fwd + rs_miou_loss_bwd                      -- the same passes over the same bytes as tversky0
    tversky1   the same three calls with lambda = 1                     -- the fused "Dice + cross-entropy"
    ce         rs_nll_loss_fwd + rs_nll_loss_bwd (CrossEntropy)         -- tversky0 + ce is the unfused alternative to tversky1

Through the C ABI by ctypes, binding only what a variant calls, so that the parent commit's library runs from the same script
(``--lib``: it has no rs_tversky_* and times ``miou`` and ``ce`` only).  ``--module`` adds the same four through the Python modules
and autograd (this tree's library only).  Times are device events around ``--steps`` passes after ``--warmup``, the median of
``--rounds`` rounds; kernel times come from running this script under ``rocprofv3 --kernel-trace --stats``, a process of its own.

    python scripts/bench_tversky.py --out profiles/tversky
    python scripts/bench_tversky.py --lib parent/librobosat_hip.so --out profiles/tversky --name parent
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def inputs(n, c, size, dev, seed=1):
    """Labels in 8 x 8 blocks, logits = randn * 0.5 + 3 * onehot(label): a confident network, which puts mIoULoss2d on its soft-IoU
    branch (the branch whose passes are the Tversky passes)."""

    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, c, (n, size // 8, size // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    x = torch.randn(n, c, size, size, generator=g) * 0.5
    x.scatter_add_(1, t.unsqueeze(1), torch.full((n, 1, size, size), 3.0))
    weight = torch.tensor([1.0, 2.5] + [1.0] * (c - 2))[:c]
    return x.to(dev), t.to(dev), weight.to(dev)


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
    return start.elapsed_time(stop) * 1000.0 / steps


def abi_variants(lib, x, t, weight, have_tversky):
    """name -> (step, result) on the C ABI; result() returns what the variant computed, for the record."""

    n, c, h, w = x.shape
    dev = x.device
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    loss = {k: torch.zeros((), device=dev) for k in ("tversky0", "miou", "tversky1", "ce")}
    dx = torch.empty_like(x)
    lib.rs_miou_loss_workspace_bytes.restype = ctypes.c_long
    nbytes = max(1 << 20, lib.rs_miou_loss_workspace_bytes(n, c))
    if have_tversky:
        lib.rs_tversky_workspace_bytes.restype = ctypes.c_long
        nbytes = max(nbytes, lib.rs_tversky_workspace_bytes(n, c))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nll_stats = torch.zeros(2, device=dev)
    miou_stats = torch.zeros(5 + 2 * n * c, device=dev)
    tv_sums = torch.zeros(3 * n * c + 2, dtype=torch.float64, device=dev)
    tv_stats = torch.zeros(4 + 2 * n * c, device=dev)
    f = ctypes.c_float

    def check(rc):
        if rc:
            sys.exit("bench_tversky: status {}".format(rc))

    def ce():
        check(lib.rs_nll_loss_fwd(p(x), p(t), p(weight), p(loss["ce"]), p(nll_stats), n, c, h, w, 0, f(0.0), p(ws), stream))
        check(lib.rs_nll_loss_bwd(p(x), p(t), p(weight), p(nll_stats), None, p(dx), n, c, h, w, 0, f(0.0), stream))

    def miou():
        check(lib.rs_miou_loss_fwd(p(x), p(t), p(weight), p(loss["miou"]), p(miou_stats), n, c, h, w, p(ws), stream))
        check(lib.rs_miou_loss_bwd(p(x), p(t), p(weight), p(miou_stats), None, p(dx), n, c, h, w, stream))

    def tversky(name, lam):
        def step():
            check(lib.rs_tversky_sums(p(x), p(t), p(weight), p(tv_sums), n, c, h, w, 1, -1, p(ws), stream))
            check(lib.rs_tversky_finalize(p(tv_sums), p(loss[name]), p(tv_stats), n, c, f(0.5), f(0.5), f(1.0), f(1.0), f(lam), 0, 1, 1,
                                          stream))
            check(lib.rs_tversky_bwd(p(x), p(t), p(weight), p(tv_stats), None, p(dx), n, c, h, w, 1, f(lam), -1, stream))
        return step

    out = {"miou": miou, "ce": ce}
    if have_tversky:
        out.update({"tversky0": tversky("tversky0", 0.0), "tversky1": tversky("tversky1", 1.0)})
    return out, loss, miou_stats


def module_variants(x, t, weight):
    from robosat_amd import losses

    crits = {"tversky0": losses.TverskyLoss2d(weight=weight), "miou": losses.mIoULoss2d(weight=weight),
             "tversky1": losses.TverskyLoss2d(ce=1.0, weight=weight), "ce": losses.CrossEntropyLoss2d(weight=weight)}
    leaf = x.detach().requires_grad_(True)

    def make(crit):
        crit = crit.to(x.device)

        def step():
            leaf.grad = None
            crit(leaf, t).backward()
        return step

    return {k: make(v) for k, v in crits.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "robosat_amd", "librobosat_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tversky"))
    ap.add_argument("--name", default="bench", help="the JSON file's stem")
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--module", action="store_true", help="also time the Python modules under autograd")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tversky: needs the MI355X (no CPU path)")

    lib = ctypes.CDLL(args.lib, mode=ctypes.RTLD_GLOBAL)
    have_tversky = hasattr(lib, "rs_tversky_sums")
    dev = torch.device("cuda", 0)
    order = ["tversky0", "miou", "tversky1", "ce"]
    record = {"lib": os.path.relpath(os.path.abspath(args.lib), ROOT), "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
              "shapes": []}
    for c in args.classes:
        x, t, weight = inputs(args.n, c, args.size, dev)
        steps, loss, miou_stats = abi_variants(lib, x, t, weight, have_tversky)
        levels = {"abi": steps}
        if args.module and have_tversky:
            levels["module"] = module_variants(x, t, weight)
        entry = {"shape": [args.n, c, args.size, args.size]}
        for level, variants in levels.items():
            names = [k for k in order if k in variants]
            rounds = {k: [] for k in names}
            for _ in range(args.rounds):
                for k in names:  # the variants alternate inside a round: a drift of the machine hits all of them
                    rounds[k].append(timed(variants[k], args.steps, args.warmup))
            us = {k: round(statistics.median(v), 2) for k, v in rounds.items()}
            entry[level] = {"us_per_pass": us, "rounds": {k: [round(v, 2) for v in vs] for k, vs in rounds.items()}}
            if "tversky0" in us:
                entry[level]["a_tversky0_over_miou"] = round(us["tversky0"] / us["miou"], 4)
                entry[level]["b_tversky1_over_tversky0_plus_ce"] = round(us["tversky1"] / (us["tversky0"] + us["ce"]), 4)
        entry["loss"] = {k: float(v) for k, v in loss.items() if k in levels["abi"]}
        entry["miou_branch"] = "nll" if float(miou_stats[2]) > 0.5 else "miou"
        record["shapes"].append(entry)
        print(json.dumps(entry))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.name + ".json"), "w") as fp:
        json.dump(record, fp, indent=1)
        fp.write("\n")


if __name__ == "__main__":
    main()
