"""`rs evaluate --centerline`: where the time goes, on 16 tiles of 512 x 512 cut from one 2048 x 2048 road raster
(`bench_features.road_raster`), the prediction being the labels moved by (3, 5) pixels.

  (default)             the stages of one batch, host clock around a synchronize, median of --repeat after a warm-up, per tile and
                        stitched -> profiles/evaluate_centerline/bench_evaluate_centerline.json
  --stage-loop N        only `ops.boundary_counts` (D = RHO) and `ops.centerline_counts` N times each on the same tiles, for
                        `rocprofv3 --kernel-trace --stats -- python scripts/bench_evaluate_centerline.py --stage-loop 20`
  --phases TRACE.csv    no device: that run's *_kernel_trace.csv -> median us per launch of the two counting kernels and of the
                        stages behind `ops.centerline_counts`
  --cli                 no device in this process: writes the tiles as PNGs and runs `rs evaluate --type road` with and without
                        `--centerline RHO` in turn, --repeat times each, wall clock of the whole process"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_features import road_raster  # noqa: E402

SIDE, TILE = 2048, 512
KERNELS = ("eval_centerline_kernel", "eval_boundary_kernel", "edt_", "thin_pass_kernel")


def tiles():
    """(predicted, actual) class-index tiles uint8 [16, 512, 512] in slot order (x, then y), and their tile coordinates."""

    labels = road_raster(SIDE, 5)
    masks = np.roll(labels, (3, 5), axis=(0, 1))
    n = SIDE // TILE
    coords = [(x, y) for x in range(n) for y in range(n)]

    def cut(image):
        return np.stack([image[y * TILE:(y + 1) * TILE, x * TILE:(x + 1) * TILE] for x, y in coords])

    return cut(masks), cut(labels), coords


def median_ms(fn, repeat, warmup=3):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4)


def phases(path, loop):
    import csv

    with open(path) as fp:
        rows = list(csv.DictReader(fp))
    result = {"loop": loop, "us_per_launch_median": {}, "launches": {}}
    for name in KERNELS:
        times = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if times:
            result["us_per_launch_median"][name] = round(statistics.median(times), 2)
            result["launches"][name] = len(times)
    print(json.dumps(result, indent=1, sort_keys=True))


def cli(args):
    from robosat_amd import png
    from robosat_amd.colors import make_palette

    predicted, actual, coords = tiles()
    palette = make_palette("denim", "orange")
    with tempfile.TemporaryDirectory() as tmp:
        dataset = os.path.join(tmp, "dataset.toml")
        with open(dataset, "w") as fp:
            fp.write('[common]\nclasses = ["background", "road"]\ncolors = ["denim", "orange"]\n')
        for name, stack in (("masks", predicted), ("labels", actual)):
            for (x, y), image in zip(coords, stack):
                os.makedirs(os.path.join(tmp, name, "18", str(1000 + x)), exist_ok=True)
                png.write_png(os.path.join(tmp, name, "18", str(1000 + x), str(2000 + y) + ".png"), image, "P", palette)
        base = [sys.executable, "-m", "robosat_amd.tools", "evaluate", os.path.join(tmp, "masks"), os.path.join(tmp, "labels"), "--dataset",
                dataset, os.path.join(tmp, "report.json"), "--type", "road"]
        variants = {"without": [], "centerline": ["--centerline", str(args.rho)], "centerline_stitch": ["--centerline", str(args.rho), "--stitch"],
                    "without_stitch": ["--stitch"]}
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        seconds = {name: [] for name in variants}
        for _ in range(args.repeat + 1):  # (the first round warms the file cache and is dropped)
            for name, extra in variants.items():
                t0 = time.perf_counter()
                subprocess.run(base + extra, env=env, cwd=ROOT, check=True, capture_output=True, timeout=300)
                seconds[name].append(round(time.perf_counter() - t0, 3))
        with open(os.path.join(tmp, "report.json")) as fp:
            report = json.load(fp)
    print(json.dumps({"rho": args.rho, "wall_seconds": {k: v[1:] for k, v in seconds.items()},
                      "wall_seconds_median": {k: statistics.median(v[1:]) for k, v in seconds.items()},
                      "last_report_objects": {k: report["objects"][k] for k in ("predicted", "actual", "matched")}}, indent=1, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rho", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--stage-loop", type=int, default=0)
    ap.add_argument("--phases", type=str, default=None)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "evaluate_centerline", "bench_evaluate_centerline.json"))
    args = ap.parse_args()
    if args.phases:
        return phases(args.phases, args.stage_loop)
    if args.cli:
        return cli(args)

    import torch

    from robosat_amd import ops
    from robosat_amd.evaluate import centerline_report
    from robosat_amd.features import stitch_tables
    from robosat_amd.tiles import Tile

    if not torch.cuda.is_available():
        raise SystemExit("this measures on the MI355X only")
    rho, r = args.rho, args.repeat
    predicted, actual, coords = tiles()
    predicted, actual = torch.from_numpy(predicted).to("cuda:0"), torch.from_numpy(actual).to("cuda:0")
    nbr = torch.from_numpy(stitch_tables([Tile(x, y, 18) for x, y in coords], (TILE, TILE))[0]).to("cuda:0")
    mask_p, mask_g = ops.clean_masks(predicted, 1, 0, 0), ops.clean_masks(actual, 1, 0, 0)
    skel_p, skel_g = ops.thin_masks(mask_p), ops.thin_masks(mask_g)
    d2_p, d2_g = ops.distance_transform(mask_p, rho + 1), ops.distance_transform(mask_g, rho + 1)

    if args.stage_loop:
        for _ in range(args.stage_loop):
            ops.boundary_counts(d2_p, d2_g, rho)
        for _ in range(args.stage_loop):
            ops.centerline_counts(skel_p, skel_g, rho)
        torch.cuda.synchronize()
        return

    def transforms(a, b, table=None):
        return (ops.distance_transform((a == 0).to(torch.uint8), rho + 1, table), ops.distance_transform((b == 0).to(torch.uint8), rho + 1, table))

    stitched_p, stitched_g = ops.thin_masks(mask_p, nbr), ops.thin_masks(mask_g, nbr)
    counts = ops.centerline_counts(skel_p, skel_g, rho).sum(dim=0).tolist()
    counts_stitched = ops.centerline_counts(stitched_p, stitched_g, rho, nbr)[0].tolist()
    pixels = predicted.numel()
    ends = 2 * (counts[0] + counts[1] + counts[4] + counts[5])  # link ends: the int32 loads of the transforms (an upper bound: shared ends)
    result = {
        "batch": len(coords), "size": TILE, "rho": rho, "repeat": r, "road_share": round(float(mask_g.float().mean()), 4),
        "skeleton_share": round(float(skel_g.float().mean()), 5),
        "counts_per_tile_summed": counts, "counts_stitched": counts_stitched,
        "report_per_tile": centerline_report(rho, counts), "report_stitched": centerline_report(rho, counts_stitched),
        "bytes": {"eval_boundary_kernel": 8 * pixels, "eval_centerline_kernel_skeletons": 2 * pixels, "eval_centerline_kernel_link_ends": 4 * ends},
        "ms_per_batch_median": {
            "select_both": median_ms(lambda: (ops.clean_masks(predicted, 1, 0, 0), ops.clean_masks(actual, 1, 0, 0)), r),
            "thin_both": median_ms(lambda: (ops.thin_masks(mask_p), ops.thin_masks(mask_g)), r),
            "thin_both_stitched": median_ms(lambda: (ops.thin_masks(mask_p, nbr), ops.thin_masks(mask_g, nbr)), r),
            "complement_and_transform_both": median_ms(lambda: transforms(skel_p, skel_g), r),
            "complement_and_transform_both_stitched": median_ms(lambda: transforms(stitched_p, stitched_g, nbr), r),
            "centerline_counts": median_ms(lambda: ops.centerline_counts(skel_p, skel_g, rho), r),
            "centerline_counts_and_copy": median_ms(lambda: ops.centerline_counts(skel_p, skel_g, rho).tolist(), r),
            "centerline_counts_stitched": median_ms(lambda: ops.centerline_counts(stitched_p, stitched_g, rho, nbr), r),
            "boundary_counts_alone": median_ms(lambda: ops.boundary_counts(d2_p, d2_g, rho), r),
            "boundary_view": median_ms(lambda: ops.boundary_counts(ops.distance_transform(mask_p, rho + 1), ops.distance_transform(mask_g, rho + 1),
                                                                   rho).tolist(), r),
            "centerline_view": median_ms(lambda: ops.centerline_counts(ops.thin_masks(mask_p), ops.thin_masks(mask_g), rho).tolist(), r),
            "centerline_view_stitched": median_ms(lambda: ops.centerline_counts(ops.thin_masks(mask_p, nbr), ops.thin_masks(mask_g, nbr), rho,
                                                                                nbr).tolist(), r),
        },
        "thin_pairs": [ops.thin_masks(mask_p, want_pairs=True)[1], ops.thin_masks(mask_g, want_pairs=True)[1]],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
