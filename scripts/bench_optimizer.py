"""The optimiser step alone: the real parameter set of ``UNet(2)`` (the tensors that receive a gradient, in their own memory order)
stepped with random gradients, no network pass (profiles/optimizer/README.md).  Variants, alternating inside every round:

    adam_torch     torch.optim.Adam(fused=True), ``rs train``'s step without the new keys            7 * 4 * N bytes
    native_plain   robosat_amd.optim.AdamW with no extras (constant rate, wd = 0)                    7 * 4 * N bytes
    torch_full     torch AdamW(fused=True) + clip_grad_norm_ + _foreach_lerp_ (the EMA)              the composition native_full replaces
    native_full    robosat_amd.optim.AdamW with decay + poly schedule + clip_norm + ema              (9 * 4 + 4) * N bytes

N = the number of stepped elements.  Bytes are what the algorithm must move: p, m, v read and written and g read (7 floats per
element), the shadow read and written (+ 2) and the norm's extra read of g (+ 1).  Times are device events around ``--steps`` steps
after ``--warmup``, the median of ``--rounds`` rounds with the spread (max - min) / median beside it; bytes/s = bytes / time.  Kernel
times come from running this script under ``rocprofv3 --kernel-trace --stats``, in a process of its own (``--only`` picks a variant).

    python scripts/bench_optimizer.py --out profiles/optimizer
"""

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parameter_set(dev, seed=0):
    """Clones of the U-Net's stepped parameters (resnet.fc never gets a gradient) and one fixed gradient per tensor, laid out like it."""

    from robosat_amd.unet import UNet

    torch.manual_seed(seed)
    net = UNet(2, pretrained=False).to(dev)
    shapes = [p.detach() for n, p in net.named_parameters() if not n.startswith("resnet.fc.")]
    g = torch.Generator(device=dev).manual_seed(seed + 1)

    def fresh():
        params = [torch.nn.Parameter(p.clone(memory_format=torch.preserve_format)) for p in shapes]
        for q in params:
            q.grad = torch.empty_like(q, memory_format=torch.preserve_format).normal_(0.0, 1e-2, generator=g)
        return params

    return fresh, sum(p.numel() for p in shapes), len(shapes)


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


def variants(fresh, total_steps):
    from robosat_amd.optim import AdamW

    lr, wd, clip, ema = 1e-4, 0.01, 1.0, 0.999
    out = {}

    params = fresh()
    adam = torch.optim.Adam(params, lr=lr, fused=True)
    out["adam_torch"] = adam.step

    params = fresh()
    plain = AdamW(params, lr=lr)
    out["native_plain"] = plain.step

    params_t = fresh()
    decay = [q for q in params_t if q.dim() > 1]
    rest = [q for q in params_t if q.dim() <= 1]
    adamw = torch.optim.AdamW([{"params": decay, "weight_decay": wd}, {"params": rest, "weight_decay": 0.0}], lr=lr, fused=True)
    shadows = [q.detach().clone(memory_format=torch.preserve_format) for q in params_t]
    kept = [q.grad.clone(memory_format=torch.preserve_format) for q in params_t]

    def torch_full():
        # (clip_grad_norm_ scales the gradients in place: give it the same gradients every step, the copy left out of no variant's
        # bytes but inside this one's time would flatter the native step, so the scaling is undone by restoring g outside the window
        # only when it has drifted to denormals: with clip = 1 and |g| ~ 60 the coefficient is ~0.016 per step)
        torch.nn.utils.clip_grad_norm_(params_t, clip)
        adamw.step()
        with torch.no_grad():
            torch._foreach_lerp_(shadows, [q.detach() for q in params_t], 1.0 - ema)

    def torch_full_reset():
        with torch.no_grad():
            for q, k in zip(params_t, kept):
                q.grad.copy_(k)

    out["torch_full"] = torch_full
    out["torch_full.reset"] = torch_full_reset

    params = fresh()
    full = AdamW(params, lr=lr, weight_decay=wd, clip_norm=clip, ema=ema,
                 schedule={"kind": "poly", "total_steps": total_steps, "warmup_steps": 10})
    out["native_full"] = full.step
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer"))
    ap.add_argument("--name", default="bench_optimizer", help="the JSON file's stem")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default=None, help="one variant (for a kernel trace of its own)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optimizer: needs the MI355X (no CPU path)")
    from robosat_amd import ops

    dev = torch.device("cuda", 0)
    fresh, n, tensors = parameter_set(dev)
    steps = variants(fresh, args.rounds * (args.steps + args.warmup))
    order = [k for k in ("adam_torch", "native_plain", "torch_full", "native_full") if args.only in (None, k)]
    nbytes = {"adam_torch": 28 * n, "native_plain": 28 * n, "torch_full": 40 * n, "native_full": 40 * n}
    rounds = {k: [] for k in order}
    for _ in range(args.rounds):
        for k in order:  # the variants alternate inside a round: a drift of the machine hits all of them
            if k + ".reset" in steps:
                steps[k + ".reset"]()
            rounds[k].append(timed(steps[k], args.steps, args.warmup))
    chunk, items = ops.optim_limits()
    record = {"elements": n, "tensors": tensors, "chunk": chunk, "items_per_launch": items, "steps": args.steps, "warmup": args.warmup,
              "rounds": args.rounds, "variants": {}}
    for k in order:
        med = statistics.median(rounds[k])
        record["variants"][k] = {"us_per_step": round(med, 2), "spread": round((max(rounds[k]) - min(rounds[k])) / med, 4),
                                 "bytes": nbytes[k], "TB_per_s": round(nbytes[k] / med / 1e6, 3),
                                 "rounds_us": [round(v, 2) for v in rounds[k]]}
    v = record["variants"]
    if "adam_torch" in v and "native_plain" in v:
        record["native_plain_over_adam_torch"] = round(v["native_plain"]["us_per_step"] / v["adam_torch"]["us_per_step"], 4)
    if "torch_full" in v and "native_full" in v:
        record["native_full_over_torch_full"] = round(v["native_full"]["us_per_step"] / v["torch_full"]["us_per_step"], 4)
    print(json.dumps(record))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, args.name + ".json"), "w") as fp:
        json.dump(record, fp, indent=1)
        fp.write("\n")


if __name__ == "__main__":
    main()
