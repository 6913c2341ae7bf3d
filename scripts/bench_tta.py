"""Dihedral test-time augmentation of ``rs predict``: ``UNet.predict_quantized(tta=...)`` at 576^2 (512 + 2 * 32 overlap), fp32 and
bf16.  Every mode at N = 16 tiles per call, and d4 at N = 2 (the same 16-tile network batch as "none" at N = 16).  Device events
around 10 calls after 3 warm-up calls; ms per call, ms per network tile, and the fan-out + merge share (the two kernels timed
alone on the same operands).
usage: python scripts/bench_tta.py [MODE ...]  (default: every mode; "none" always runs, as the baseline; measurement tool; run it under rocprofv3 --kernel-trace --stats for the per-kernel split)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from oracle import robosat_ref as R, seeded
from robosat_amd import ops
from robosat_amd.unet import UNet

dev = torch.device("cuda:0")
REPS = 10
SIZE, OVERLAP = 576, 32
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


os.environ.setdefault("ROBOSAT_GRAPHS", "0")  # (eager, as `rs predict` runs batches of this size)
sd = seeded.seeded_state_dict(R.UNetRef(2).state_dict(), 0)
for dt in (torch.float32, torch.bfloat16):
    net = UNet(2, pretrained=False, compute_dtype=dt)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    base = None
    for mode, n in (("none", 16), ("hflip", 16), ("flips", 16), ("d4", 16), ("d4", 2)):
        if mode != "none" and sys.argv[1:] and mode not in sys.argv[1:]:
            continue
        g = torch.Generator().manual_seed(1)
        u8 = torch.randint(0, 256, (n, SIZE, SIZE, 3), generator=g, dtype=torch.uint8).to(dev)
        op_list = ops.tta_ops(mode, SIZE, SIZE)
        v = len(op_list)
        ms = timed(lambda: net.predict_quantized(u8, overlap=OVERLAP, tta=mode))
        per_tile = ms / (n * v)
        if mode == "none":
            base = per_tile
        extra = ""
        if mode != "none":
            x4 = ops.tta_fan_out_u8(u8, MEAN, STD, op_list, dt)
            probs = torch.rand((n * v, 2, SIZE, SIZE), device=dev)
            fan = timed(lambda: ops.tta_fan_out_u8(u8, MEAN, STD, op_list, dt))
            merge = timed(lambda: ops.tta_merge(probs, op_list, "quantize", OVERLAP))
            fan_bytes = u8.numel() + x4.numel() * x4.element_size()
            s_out = SIZE - 2 * OVERLAP
            merge_bytes = probs.numel() * 4 * (s_out * s_out) / (SIZE * SIZE) + n * s_out * s_out  # (border blocks are skipped)
            extra = "  fan-out {:.3f} ms ({:.2f} TB/s)  merge {:.3f} ms ({:.2f} TB/s)  share {:.2f} %".format(
                fan, fan_bytes / fan / 1e9, merge, merge_bytes / merge / 1e9, 100.0 * (fan + merge) / ms)
            del x4, probs
        print("{:<4s} N {:2d} V {} ({:3d} network tiles)  {:8.2f} ms per call  {:.3f} ms per network tile ({:+.1f} % vs none){}".format(
            "fp32" if dt == torch.float32 else "bf16", n, v, n * v, ms, per_tile, 100.0 * (per_tile / base - 1.0), extra), flush=True)
    del net
    torch.cuda.empty_cache()
