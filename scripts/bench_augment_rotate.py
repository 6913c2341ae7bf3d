"""What ``[augment] rotate`` costs at the flagship batch (N = 32 tiles of 3 x 512 x 512): ``rs_augment_tiles_jitter`` with the README's
full table (what ``rs train`` launches without the key) against ``rs_augment_tiles_rotate`` at rotate = 180 on the same tiles, ops,
windows and factors, plus the rotate kernel at 0 degrees (its fixed cost over the zoom, no gather) and at 45 degrees for every item
(the most scattered rows).  The launches alternate in one process; one pair of device events per launch after warm-up, REPS launches
each; median and 10th / 90th percentile, and GB/s from the bytes the shapes give (input bytes once + output bytes; the four taps per
pixel are not counted again).
usage: python scripts/bench_augment_rotate.py [--reps 200] [--out FILE.json]   (measurement tool; run it under rocprofv3 --kernel-trace
--stats for the per-kernel times)"""
import argparse
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_augment import MEAN, STD, alternate, row
from robosat_amd import ops
from robosat_amd.augment import Jitter, draw_jitter, draw_rotation, rotation
from robosat_amd.datasets import draw_flip_rotations

dev = torch.device("cuda:0")
N, S, C = 32, 512, 3
TABLE = Jitter(1.5, (0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (0.8, 1.25), True, 180.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator().manual_seed(C)
    images = torch.randint(0, 256, (N, S, S, C), generator=g, dtype=torch.uint8).to(dev)
    masks = torch.randint(0, 2, (N, S, S), generator=g, dtype=torch.uint8).to(dev)
    sums = ops.tile_band_sums(images)
    random.seed(7)
    index = torch.tensor(random.sample(range(N), N), dtype=torch.int32, device=dev)
    codes, geom, color, rot = [], [], [], []
    for _ in range(N):  # the draws of one training batch, in the loaders' order
        codes.append(draw_flip_rotations())
        w, f = draw_jitter(TABLE, S)
        geom.append(w)
        color.append(f)
        rot.append(draw_rotation(TABLE))
    op = torch.tensor(codes, dtype=torch.int32, device=dev)
    geom, color = torch.tensor(geom, dtype=torch.int32), torch.tensor(color, dtype=torch.float32)
    rot = torch.tensor(rot, dtype=torch.int32)
    still, diagonal = torch.tensor([rotation(0.0, 0.5)] * N, dtype=torch.int32), torch.tensor([rotation(45.0, 1.0)] * N, dtype=torch.int32)
    mean, std = MEAN[:C], STD[:C]
    variants = {
        "jitter, every stage (no rotate key)": lambda: ops.augment_tiles_jitter(images, masks, index, op, geom, color, sums, mean, std, True),
        "rotate, angles as drawn (A = 180)": lambda: ops.augment_tiles_rotate(images, masks, index, op, geom, rot, color, sums, mean, std, True),
        "rotate, every item at 0 degrees": lambda: ops.augment_tiles_rotate(images, masks, index, op, geom, still, color, sums, mean, std, True),
        "rotate, every item at 45 degrees": lambda: ops.augment_tiles_rotate(images, masks, index, op, geom, diagonal, color, sums, mean, std, True),
    }
    times = alternate(variants, args.reps)
    moved = N * S * S * (C + 1) + N * S * S * (4 * C + 8)  # tile + mask bytes in, fp32 planes + int64 labels out
    rows = [row(name, ms, moved) for name, ms in times.items()]
    base, turned = rows[0]["us_median"], rows[1]["us_median"]
    print("rotate over jitter: {:.2f} x, {:+.1f} us per batch".format(turned / base, turned - base))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump({"N": N, "S": S, "C": C, "rows": rows, "rotate_over_jitter": turned / base}, fp, indent=1)


if __name__ == "__main__":
    main()
