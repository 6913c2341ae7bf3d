"""`rs evaluate --type --ignored unknown`: what the flag costs, on 16 tiles of 512 x 512 with two classes
(`bench_features.blob_masks`), the prediction being the labels moved by (3, 5) pixels, the labels with about 5 % ignored pixels in
three rectangles per tile.

  (default)             the stages of one batch, host clock around a synchronize, median of --repeat after a warm-up: the flagged
                        stages beside the ones they stand in for -> profiles/evaluate_ignore/bench_evaluate_ignore.json
  --unflagged           only the `--type --boundary D` stages without the flag, on labels free of ignored pixels: calls that every
                        build since `rs evaluate` has.  Prints one JSON line
  --ab PARENT.so        no device in this process: runs `--unflagged` in child processes, in turn on the library at PARENT.so (a
                        build of the parent commit) and on this tree's, --rounds times each -> the medians and their spread
  --stage-loop N        the counting and selecting calls N times each on the same tiles, for
                        `rocprofv3 --kernel-trace --stats -- python scripts/bench_evaluate_ignore.py --stage-loop 20`
  --phases TRACE.csv    no device: that run's *_kernel_trace.csv -> median us per launch of the kernels"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_features import blob_masks  # noqa: E402

BATCH, TILE, IGNORE = 16, 512, 255
KERNELS = ("eval_select_kernel", "eval_boundary_kernel<true>", "eval_boundary_kernel<false>", "eval_confusion_kernel", "eval_confusion_ig_kernel",
           "clean_select_kernel", "clean_pass_kernel", "clean_unpack_kernel", "clean_lds_kernel", "edt_row_kernel", "edt_col_kernel")
NEW_SYMBOLS = ("rs_eval_select", "rs_eval_boundary_coded")


def tiles():
    """(predicted, labels without ignored pixels, labels with them) uint8 [16, 512, 512]."""

    known = blob_masks(BATCH, TILE, 11)
    predicted = np.roll(known, (3, 5), axis=(1, 2))
    actual = known.copy()
    rng = np.random.RandomState(12)
    for b in range(BATCH):
        for _ in range(3):  # 3 x 66 x 66 = 13068 of 262144 pixels: 5 % where they do not overlap
            y, x = rng.randint(0, TILE - 66, 2)
            actual[b, y:y + 66, x:x + 66] = IGNORE
    return predicted, known, actual


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


def ab(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    command = [sys.executable, os.path.abspath(__file__), "--unflagged", "--repeat", str(args.repeat), "--boundary", str(args.boundary)]
    runs = {"parent": [], "here": []}
    for _ in range(args.rounds):
        for name in ("parent", "here"):
            child = dict(env)
            if name == "parent":
                child["ROBOSAT_HIP_LIB"] = os.path.abspath(args.ab)
            else:
                child.pop("ROBOSAT_HIP_LIB", None)
            done = subprocess.run(command, env=child, cwd=ROOT, check=True, capture_output=True, text=True, timeout=300)
            runs[name].append(json.loads(done.stdout.strip().splitlines()[-1]))
    stages = list(runs["here"][0]["ms_per_batch_median"])
    summary = {name: {s: {"median": statistics.median(r["ms_per_batch_median"][s] for r in rs),
                          "min": min(r["ms_per_batch_median"][s] for r in rs), "max": max(r["ms_per_batch_median"][s] for r in rs)}
                      for s in stages} for name, rs in runs.items()}
    same = all(r["counts"] == runs["here"][0]["counts"] for rs in runs.values() for r in rs)
    print(json.dumps({"rounds": args.rounds, "repeat": args.repeat, "boundary": args.boundary, "same_counts": same, "runs": runs, "summary": summary},
                     indent=1, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boundary", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--unflagged", action="store_true")
    ap.add_argument("--ab", type=str, default=None)
    ap.add_argument("--stage-loop", type=int, default=0)
    ap.add_argument("--phases", type=str, default=None)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "evaluate_ignore", "bench_evaluate_ignore.json"))
    args = ap.parse_args()
    if args.phases:
        return phases(args.phases, args.stage_loop)
    if args.ab:
        return ab(args)

    import torch

    from robosat_amd import _lib, ops

    if not torch.cuda.is_available():
        raise SystemExit("this measures on the MI355X only")
    if args.unflagged:  # (a parent build has neither symbol, and this leg calls neither)
        for name in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(name, None)
    d, r = args.boundary, args.repeat
    predicted, known, actual = (torch.from_numpy(a).to("cuda:0") for a in tiles())

    def plain_stages(labels):
        mask_p, mask_g = ops.clean_masks(predicted, 1, 0, 0), ops.clean_masks(labels, 1, 0, 0)
        return ops.boundary_counts(ops.distance_transform(mask_p, d + 1), ops.distance_transform(mask_g, d + 1), d).tolist()

    if args.unflagged:
        mask_p, mask_g = ops.clean_masks(predicted, 1, 0, 0), ops.clean_masks(known, 1, 0, 0)
        d2_p, d2_g = ops.distance_transform(mask_p, d + 1), ops.distance_transform(mask_g, d + 1)
        print(json.dumps({"lib": _lib.LIB_PATH, "counts": np.array(plain_stages(known)).sum(axis=0).tolist(), "ms_per_batch_median": {
            "clean_masks_both": median_ms(lambda: (ops.clean_masks(predicted, 1, 0, 0), ops.clean_masks(known, 1, 0, 0)), r),
            "transform_both": median_ms(lambda: (ops.distance_transform(mask_p, d + 1), ops.distance_transform(mask_g, d + 1)), r),
            "boundary_counts": median_ms(lambda: ops.boundary_counts(d2_p, d2_g, d), r),
            "stages_and_copy": median_ms(lambda: plain_stages(known), r),
        }}, sort_keys=True))
        return

    def flagged_stages(labels):
        coded_p, coded_g, _, _ = ops.select_known(predicted, labels, 1, IGNORE, 2)
        return ops.boundary_counts(ops.distance_transform(coded_p, d + 1), ops.distance_transform(coded_g, d + 1), d, coded=coded_g).tolist()

    coded_p, coded_g, mask_p, mask_g = ops.select_known(predicted, actual, 1, IGNORE, 2)
    d2_p, d2_g = ops.distance_transform(coded_p, d + 1), ops.distance_transform(coded_g, d + 1)

    if args.stage_loop:
        for _ in range(args.stage_loop):
            ops.select_known(predicted, actual, 1, IGNORE, 2)
        for _ in range(args.stage_loop):
            ops.clean_masks(predicted, 1, 0, 0), ops.clean_masks(actual, 1, 0, 0)
        for _ in range(args.stage_loop):
            ops.mask_confusion(predicted, known, 2)
        for _ in range(args.stage_loop):
            ops.mask_confusion(predicted, actual, 2, ignore=IGNORE)
        for _ in range(args.stage_loop):
            ops.boundary_counts(d2_p, d2_g, d)
        for _ in range(args.stage_loop):
            ops.boundary_counts(d2_p, d2_g, d, coded=coded_g)
        torch.cuda.synchronize()
        return

    pixels = predicted.numel()
    result = {
        "batch": BATCH, "size": TILE, "boundary": d, "repeat": r,
        "class_share": round(float((known == 1).float().mean()), 4), "ignored_share": round(float((actual == IGNORE).float().mean()), 4),
        "counts_flagged": np.array(flagged_stages(actual)).sum(axis=0).tolist(),
        "counts_flagged_without_ignored_pixels": np.array(flagged_stages(known)).sum(axis=0).tolist(),
        "counts_unflagged_without_ignored_pixels": np.array(plain_stages(known)).sum(axis=0).tolist(),
        "bytes": {"eval_select_kernel": 6 * pixels, "clean_masks_both": 4 * pixels, "eval_confusion_kernel": 2 * pixels,
                  "eval_boundary_kernel": 8 * pixels, "eval_boundary_kernel_coded": 9 * pixels},
        "ms_per_batch_median": {
            "select_known": median_ms(lambda: ops.select_known(predicted, actual, 1, IGNORE, 2), r),
            "clean_masks_both": median_ms(lambda: (ops.clean_masks(predicted, 1, 0, 0), ops.clean_masks(actual, 1, 0, 0)), r),
            "mask_confusion": median_ms(lambda: ops.mask_confusion(predicted, known, 2), r),
            "mask_confusion_ignore": median_ms(lambda: ops.mask_confusion(predicted, actual, 2, ignore=IGNORE), r),
            "transform_both_coded": median_ms(lambda: (ops.distance_transform(coded_p, d + 1), ops.distance_transform(coded_g, d + 1)), r),
            "boundary_counts": median_ms(lambda: ops.boundary_counts(d2_p, d2_g, d), r),
            "boundary_counts_coded": median_ms(lambda: ops.boundary_counts(d2_p, d2_g, d, coded=coded_g), r),
            "flagged_stages_and_copy": median_ms(lambda: flagged_stages(actual), r),
            "flagged_stages_and_copy_without_ignored_pixels": median_ms(lambda: flagged_stages(known), r),
            "unflagged_stages_and_copy_without_ignored_pixels": median_ms(lambda: plain_stages(known), r),
        },
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
