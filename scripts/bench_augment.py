"""The training feed's augmentation kernels at the flagship batch (N = 32 tiles of 512 x 512, C = 3 and C = 4): ``rs_augment_tiles``,
``rs_augment_tiles_jitter`` at identity and with every stage on (ops, windows and factors as ``rs train`` draws them from the README's
table), and ``rs_tile_band_sums`` over a 1 024-tile cache.  The launches under comparison alternate in one process; one pair of device
events per launch after warm-up, REPS launches each; median and 10th / 90th percentile, and GB/s from the bytes the shapes give (input
bytes touched once + output bytes; the jitter's four taps per pixel are not counted again).
usage: python scripts/bench_augment.py [--reps 200] [--out FILE.json]   (measurement tool; run it under rocprofv3 --kernel-trace --stats
for the per-kernel times)"""
import argparse
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from robosat_amd import ops
from robosat_amd.augment import Jitter, draw_jitter
from robosat_amd.datasets import draw_flip_rotations

dev = torch.device("cuda:0")
N, S, CACHE = 32, 512, 1024
MEAN, STD = [0.485, 0.456, 0.406, 0.449], [0.229, 0.224, 0.225, 0.226]
TABLE = Jitter(1.5, (0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (0.8, 1.25), True)


def alternate(variants, reps, warmup=10):
    """``{name: sorted ms per launch}``: the variants take turns, launch by launch."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            events[name].append((e0, e1))
    torch.cuda.synchronize()
    return {name: sorted(a.elapsed_time(b) for a, b in ev) for name, ev in events.items()}


def row(name, ms, nbytes):
    med, lo, hi = ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]
    print("{:<34s} {:8.1f} us  (p10 {:.1f}, p90 {:.1f})  {:7.1f} MB  {:6.0f} GB/s".format(name, med * 1e3, lo * 1e3, hi * 1e3, nbytes / 1e6,
                                                                                       nbytes / med / 1e6), flush=True)
    return {"name": name, "us_median": med * 1e3, "us_p10": lo * 1e3, "us_p90": hi * 1e3, "bytes": nbytes, "GBps": nbytes / med / 1e6,
            "launches": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for c in (3, 4):
        g = torch.Generator().manual_seed(c)
        images = torch.randint(0, 256, (N, S, S, c), generator=g, dtype=torch.uint8).to(dev)
        masks = torch.randint(0, 2, (N, S, S), generator=g, dtype=torch.uint8).to(dev)
        sums = ops.tile_band_sums(images)
        random.seed(7)
        index = torch.tensor(random.sample(range(N), N), dtype=torch.int32, device=dev)
        codes, geom, color = [], [], []
        for _ in range(N):
            codes.append(draw_flip_rotations())
            w, f = draw_jitter(TABLE, S)
            geom.append(w)
            color.append(f)
        op = torch.tensor(codes, dtype=torch.int32, device=dev)
        geom, color = torch.tensor(geom, dtype=torch.int32), torch.tensor(color, dtype=torch.float32)
        ident_g, ident_c = torch.tensor([[S, 0, 0]] * N, dtype=torch.int32), torch.ones((N, 4), dtype=torch.float32)
        mean, std = MEAN[:c], STD[:c]
        variants = {
            "augment_tiles C={}".format(c): lambda: ops.augment_tiles(images, masks, index, op, mean, std),
            "jitter, identity C={}".format(c): lambda: ops.augment_tiles_jitter(images, masks, index, op, ident_g, ident_c, sums, mean, std, True),
            "jitter, zoom only C={}".format(c): lambda: ops.augment_tiles_jitter(images, masks, index, op, geom, ident_c, sums, mean, std, True),
            "jitter, colour only C={}".format(c): lambda: ops.augment_tiles_jitter(images, masks, index, op, ident_g, color, sums, mean, std, True),
            "jitter, every stage C={}".format(c): lambda: ops.augment_tiles_jitter(images, masks, index, op, geom, color, sums, mean, std, True),
            "tile_band_sums of the batch C={}".format(c): lambda: ops.tile_band_sums(images),
        }
        times = alternate(variants, args.reps)
        moved = N * S * S * (c + 1) + N * S * S * (4 * c + 8)  # tile + mask bytes in, fp32 planes + int64 labels out
        for name, ms in times.items():
            rows.append(row(name, ms, N * S * S * c + N * c * 8 if name.startswith("tile_band_sums") else moved))
        del images, masks
        cache = torch.randint(0, 256, (CACHE, S, S, c), generator=g, dtype=torch.uint8).to(dev)
        times = alternate({"tile_band_sums, {} tiles C={}".format(CACHE, c): lambda: ops.tile_band_sums(cache)}, max(20, args.reps // 4))
        for name, ms in times.items():
            rows.append(row(name, ms, cache.numel() + CACHE * c * 8))
        want = cache.view(CACHE, -1, c).sum(dim=1, dtype=torch.int64)
        assert torch.equal(ops.tile_band_sums(cache), want), "band sums differ from torch's"
        del cache, want
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump({"N": N, "S": S, "rows": rows}, fp, indent=1)


if __name__ == "__main__":
    main()
