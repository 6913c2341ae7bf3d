#!/usr/bin/env python
"""Measures the `rs features` stages on the MI355X and writes profiles/features/bench_features.json:

  device   upload of the mask bytes -> clean -> label -> table -> edges back on the host; tiles/s at 512 x 512, batch 16,
           discs 20 / 20, on blob masks (about 10 % foreground) and on 50 % noise (which the opening empties: it times
           the morphology, not the labeller)
  labeller label_components alone on the shapes that are hard for it: 50 % noise unopened, a checkerboard, a one-pixel spiral
  cpu      the same stages through scipy.ndimage in a pool of at most 16 processes, for scale
  forms    the morphology kernel's LDS-resident form against its through-HBM form
  cli      `./rs features` from PNGs on disk, with the host share (PNG decode, ring linking, JSON)

  --stitch-leg   `rs features --stitch` against the per-tile path on one dataset, a dense 8 x 8 block of 512 x 512 tiles cut from one
           blob raster (objects cross the seams): per stage and whole, written to profiles/features_stitch/bench_stitch.json
           (`--stitch-leg --stage-loop N` only runs the stitched stages N times, for rocprofv3)

  --centerline-leg   `rs features --geometry centerline`: thinning and links on a synthetic road network (roads 21-24 pixels wide, so
           the 20-pixel opening keeps them), 512 x 512, batch 16, and on the stitched 8 x 8 block cut from one such raster; the pair
           count, the time at each candidate chunk size K, and the polygon path on the same masks, written to
           profiles/features_centerline/bench_centerline.json (`--centerline-leg --stage-loop N`: the stages N times, for rocprofv3)

  --dedupe-leg   `rs features --dedupe`: the polygon stages without and with the reference (its labelling, its table, the overlap
           table, the host's rule) on the blob batch, the overlap table on the shapes that bound it (one pair per tile, one pair
           per pixel) beside the labeller on the same tiles, and `./rs features` from disk without and with the flag, written to
           profiles/features_dedupe/bench_dedupe.json (`--dedupe-leg --stage-loop N`: the stages N times, for rocprofv3)

  --width-leg   `rs features --geometry centerline --width`: the distance transform beside the thinning it sits next to, the centerline
           raster stages per batch without and with it, and scipy.ndimage.distance_transform_edt on the host for the same cleaned
           masks; 16 tiles of 512 x 512 of tests/thin_ref.roads (22 pixels wide, so the 20-pixel opening keeps them) and a stitched
           4 x 4 call cut from one such raster, written to profiles/features_width/bench_width.json (`--width-leg --stage-loop N`:
           the stages N times, for rocprofv3; `--width-leg --without-only`: only the stages without the transform, which also runs
           on a tree from before it, for the comparison with the parent commit)

  --split-leg   `rs features --split`: the seed step and the regrowth on 16 tiles of 512 x 512 of tests/split_ref.touching_blobs
           (discs of about 14 pixels that touch), R = 8: the growth at every candidate number of fused steps K (the knob grow_fused;
           K = 1 is the baseline, the same kernel) and chunk size, the stages of `ops.split_labels`, the polygon stages per batch
           without and with the split, and a stitched 4 x 4 call, written to profiles/features_split/bench_split.json
           (`--split-leg --stage-loop N --fused K`: the growth alone N times at that K, for rocprofv3)

  --score-leg   `rs features --score`: the polygon stages per batch without and with the scoring stage (K = 1 and K = 3 models) on the
           blob batch, and `ops.component_scores` alone on the shapes that bound it (one component per tile, one per pixel) beside
           `ops.component_table` on the same tiles, written to profiles/features_score/bench_score.json
           (`--score-leg --stage-loop N`: the two calls on the blob batch and on the bounds N times, for rocprofv3;
           `--score-leg --stage-loop N --phases TRACE.csv`: no device, that run's kernel trace -> median us per launch and phase)

  --evaluate-leg   `rs evaluate`: per batch the counting pass alone (`ops.mask_confusion` and the copy of its counts to the host), with
           `--boundary 3` and with the object stages, on the blob batch against a copy of it moved by (3, 5) pixels, beside clean ->
           label -> table -> edges of `rs features` on the same tiles; and the counting call at its bounds (blobs, all one cell,
           random cells of 8 classes) beside `ops.label_histogram_u8` over the same two rasters, written to
           profiles/evaluate/bench_evaluate.json (`--evaluate-leg --stage-loop N`: the calls at the three bounds N times, for
           rocprofv3; `--evaluate-leg --stage-loop N --phases TRACE.csv`: no device, that run's kernel trace -> median us per launch)

  --evaluate-probs-leg   `rs evaluate --probs`: `ops.prob_histogram` beside `ops.mask_confusion` on the same two rasters and
           `ops.label_histogram_u8` over both, per call, on the blob batch as labels with three probability rasters (blob-like:
           bytes 1 and 254 with a soft edge; all one byte; uniformly random bytes) and on one tile cut into 8 x 8 tiles, written to
           profiles/evaluate_probs/bench_evaluate_probs.json (`--stage-loop N` and `--phases TRACE.csv` as for --evaluate-leg)

Compare `device.blobs` with the predict leg of `python bench.py` measured in the same session.  `--stage-loop N` only runs
the device stage N times (for `rocprofv3 --kernel-trace --stats -- python scripts/bench_features.py --stage-loop 20`)."""

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "features", "bench_features.json")


def blob_masks(batch, size, seed):
    """Class-index tiles with a handful of ellipses of class 1, about a tenth of the tile, and a little salt and pepper."""

    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:size, :size]
    out = np.zeros((batch, size, size), dtype=np.uint8)
    for b in range(batch):
        for _ in range(6):
            cy, cx = rng.randint(0, size, 2)
            ry, rx = rng.randint(size // 16, size // 8, 2)
            out[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = 1
        out[b] ^= (rng.rand(size, size) < 0.01).astype(np.uint8)
    return out


def noise_masks(batch, size, seed):
    return (np.random.RandomState(seed).rand(batch, size, size) < 0.5).astype(np.uint8)


def spiral_mask(n):
    """A one-pixel-wide square spiral filling n x n: one component, one chain of about n*n/2 pixels."""

    m = np.zeros((n, n), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):  # go on, or turn once; the cell after next must be free too (arms stay one pixel apart)
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m


def block_tiles(n, size, seed):
    """One (n * size)^2 class-index raster of ellipses of class 1 (about a tenth of it, the size of `blob_masks`' so many
    cross a seam) with a little salt and pepper, cut into n x n tiles in slot order (x, then y)."""

    rng = np.random.RandomState(seed)
    side = n * size
    image = np.zeros((side, side), dtype=np.uint8)
    for _ in range(6 * n * n):
        cy, cx = rng.randint(0, side, 2)
        ry, rx = rng.randint(size // 16, size // 8, 2)
        y0, y1, x0, x1 = max(cy - ry, 0), min(cy + ry + 1, side), max(cx - rx, 0), min(cx + rx + 1, side)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        image[y0:y1, x0:x1][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = 1
    image ^= (rng.rand(side, side) < 0.01).astype(np.uint8)
    return np.stack([image[y * size:(y + 1) * size, x * size:(x + 1) * size] for x in range(n) for y in range(n)])


def stitch_leg(args):
    """The stitched path against the per-tile path on the same n x n block, stage by stage (device time by host clock around a
    synchronize, as the other legs)."""

    import torch

    from robosat_amd import ops
    from robosat_amd.features import stitch_tables
    from robosat_amd.tiles import Tile

    n, size, eps = args.block, args.size, args.eps
    tiles = block_tiles(n, size, 0)
    nbr, origin, _ = stitch_tables([Tile(x, y, 18) for x in range(n) for y in range(n)], (size, size))
    dev, nbr, origin = torch.from_numpy(tiles).to("cuda:0"), torch.from_numpy(nbr).to("cuda:0"), torch.from_numpy(origin).to("cuda:0")
    apron = ops.halo_apron(eps, eps)

    def stitched():
        table, edges = ops.stitched_features(dev, nbr, origin, 1, eps, eps, 0)
        return table, edges.cpu()

    def per_tile():
        out = []
        for start in range(0, len(tiles), args.batch):
            labels = ops.label_components(ops.clean_masks(dev[start:start + args.batch], 1, eps, eps))
            table = ops.component_table(labels, 0)
            out.append((table, ops.boundary_edges(labels, table).cpu()))
        return out

    if args.stage_loop:
        for _ in range(args.stage_loop):
            stitched()
        return

    table, edges = stitched()
    parts = per_tile()
    padded = ops.gather_halo(dev, nbr, apron)
    cleaned_padded = ops.clean_masks(padded, 1, eps, eps)
    cleaned = ops.crop_halo(cleaned_padded, apron)
    local = ops.label_components(cleaned)
    labels = ops.stitch_labels(local, nbr)
    alone = ops.clean_masks(dev, 1, eps, eps)
    alone_labels = ops.label_components(alone)
    alone_table = ops.component_table(alone_labels, 0)
    r = args.repeat
    result = {
        "block": n, "size": size, "eps": eps, "apron": apron, "batch_per_tile": args.batch, "tiles": len(tiles),
        "foreground": float((tiles == 1).mean()),
        "stitched": {"components": int(len(table)), "edges": int(len(edges)), "ms": timed(stitched, r) * 1e3, "ms_split": {
            "gather": timed(lambda: ops.gather_halo(dev, nbr, apron), r) * 1e3,
            "clean_padded": timed(lambda: ops.clean_masks(padded, 1, eps, eps), r) * 1e3,
            "crop": timed(lambda: ops.crop_halo(cleaned_padded, apron), r) * 1e3,
            "label": timed(lambda: ops.label_components(cleaned), r) * 1e3,
            "seam_union_flatten": timed(lambda: ops.stitch_labels(local, nbr), r) * 1e3,
            "table": timed(lambda: ops.component_table_stitched(labels, origin, 0), r) * 1e3,
            "edges": timed(lambda: ops.boundary_edges_stitched(labels, nbr, origin, table).cpu(), r) * 1e3}},
        "per_tile": {"components": int(sum(len(t) for t, _ in parts)), "edges": int(sum(len(e) for _, e in parts)),
                     "ms": timed(per_tile, r) * 1e3, "ms_split_one_call_of_all_tiles": {
            "clean": timed(lambda: ops.clean_masks(dev, 1, eps, eps), r) * 1e3,
            "label": timed(lambda: ops.label_components(alone), r) * 1e3,
            "table": timed(lambda: ops.component_table(alone_labels, 0), r) * 1e3,
            "edges": timed(lambda: ops.boundary_edges(alone_labels, alone_table).cpu(), r) * 1e3}},
    }
    split = result["stitched"]["ms_split"]
    result["clean_ratio"] = {"measured": (split["gather"] + split["clean_padded"] + split["crop"])
                             / result["per_tile"]["ms_split_one_call_of_all_tiles"]["clean"],
                             "measured_clean_padded_alone": split["clean_padded"] / result["per_tile"]["ms_split_one_call_of_all_tiles"]["clean"],
                             "model": ((size + 2 * apron) / size) ** 2}
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "features_stitch", "bench_stitch.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


def road_raster(side, seed):
    """One side x side class-index raster of straight roads of class 1, 21 to 24 pixels wide, at random places and angles: six
    per 512 pixels of side (every road crosses the whole raster, so that keeps about a quarter of it road at any side)."""

    rng = np.random.RandomState(seed)
    image = np.zeros((side, side), dtype=np.uint8)
    at = np.arange(side, dtype=np.float32)
    for _ in range(max(2, 6 * side // 512)):
        cy, cx, angle, width = rng.uniform(0, side), rng.uniform(0, side), rng.uniform(0, np.pi), rng.uniform(21, 24)
        image[np.abs(((at - cx) * np.sin(angle))[None, :] - ((at - cy) * np.cos(angle))[:, None]) <= width / 2] = 1
    return image


def centerline_leg(args):
    """Thinning and links beside the polygon path on the same road masks: one batch of tiles, and the stitched n x n block."""

    import torch

    from robosat_amd import ops
    from robosat_amd.features import stitch_tables
    from robosat_amd.tiles import Tile

    n, size, eps, r = args.block, args.size, args.eps, args.repeat
    batch = np.stack([road_raster(size, seed) for seed in range(args.batch)])
    block = road_raster(n * size, 100)
    tiles = np.stack([block[y * size:(y + 1) * size, x * size:(x + 1) * size] for x in range(n) for y in range(n)])
    nbr, origin, _ = stitch_tables([Tile(x, y, 18) for x in range(n) for y in range(n)], (size, size))
    dev, dev_tiles = torch.from_numpy(batch).to("cuda:0"), torch.from_numpy(tiles).to("cuda:0")
    nbr, origin = torch.from_numpy(nbr).to("cuda:0"), torch.from_numpy(origin).to("cuda:0")

    def per_tile():
        cleaned = ops.clean_masks(dev, 1, eps, eps)
        labels = ops.label_components(cleaned)
        table = ops.component_table(labels, 0)
        return table, ops.skeleton_links(ops.thin_masks(cleaned), labels, table).cpu()

    def stitched():
        table, links = ops.stitched_centerlines(dev_tiles, nbr, origin, 1, eps, eps, 0)
        return table, links.cpu()

    if args.stage_loop:
        for _ in range(args.stage_loop):
            per_tile()
            stitched()
        return

    result = {"batch": args.batch, "size": size, "eps": eps, "block": n, "default_pairs_per_chunk": ops.THIN_PAIRS}
    cleaned = ops.clean_masks(dev, 1, eps, eps)
    labels = ops.label_components(cleaned)
    table = ops.component_table(labels, 0)
    skeleton, pairs = ops.thin_masks(cleaned, pairs=1, want_pairs=True)
    links = ops.skeleton_links(skeleton, labels, table)
    sec = timed(per_tile, r)
    polygon = timed(lambda: device_stage(batch, eps), r)
    result["per_tile"] = {
        "foreground_cleaned": float(cleaned.float().mean()), "components": int(len(table)), "skeleton_pixels": int(skeleton.sum()),
        "links": int(len(links)), "pairs": pairs, "ms_per_batch": sec * 1e3, "tiles_per_s": args.batch / sec,
        "polygon_path_ms_per_batch": polygon * 1e3, "polygon_path_tiles_per_s": args.batch / polygon,
        "ms_split": {"clean": timed(lambda: ops.clean_masks(dev, 1, eps, eps), r) * 1e3,
                     "label": timed(lambda: ops.label_components(cleaned), r) * 1e3,
                     "table": timed(lambda: ops.component_table(labels, 0), r) * 1e3,
                     "thin": timed(lambda: ops.thin_masks(cleaned), r) * 1e3,
                     "links": timed(lambda: ops.skeleton_links(skeleton, labels, table).cpu(), r) * 1e3},
        "thin_ms_by_pairs_per_chunk": {str(k): timed(lambda: ops.thin_masks(cleaned, pairs=k), r) * 1e3 for k in (1, 2, 4, 8, 16, 32, 64)},
    }
    full = torch.ones((args.batch, size, size), dtype=torch.uint8, device="cuda:0")
    _, full_pairs = ops.thin_masks(full, pairs=1, want_pairs=True)
    result["full_tiles"] = {"pairs": full_pairs, "thin_ms_by_pairs_per_chunk": {
        str(k): timed(lambda: ops.thin_masks(full, pairs=k), max(2, r // 4)) * 1e3 for k in (1, 4, 16, 64)}}

    cleaned = ops.clean_masks_stitched(dev_tiles, nbr, 1, eps, eps)
    labels = ops.stitch_labels(ops.label_components(cleaned), nbr)
    table = ops.component_table_stitched(labels, origin, 0)
    skeleton, pairs = ops.thin_masks(cleaned, nbr, pairs=1, want_pairs=True)
    links = ops.skeleton_links(skeleton, labels, table, nbr, origin)
    sec = timed(stitched, r)

    def polygons():
        table, edges = ops.stitched_features(dev_tiles, nbr, origin, 1, eps, eps, 0)
        return edges.cpu()

    polygon = timed(polygons, r)
    result["stitched"] = {
        "tiles": len(tiles), "components": int(len(table)), "skeleton_pixels": int(skeleton.sum()), "links": int(len(links)), "pairs": pairs,
        "ms": sec * 1e3, "tiles_per_s": len(tiles) / sec, "polygon_path_ms": polygon * 1e3, "polygon_path_tiles_per_s": len(tiles) / polygon,
        "ms_split": {"thin": timed(lambda: ops.thin_masks(cleaned, nbr), r) * 1e3,
                     "thin_ignoring_seams": timed(lambda: ops.thin_masks(cleaned), r) * 1e3,
                     "links": timed(lambda: ops.skeleton_links(skeleton, labels, table, nbr, origin).cpu(), r) * 1e3},
        "thin_ms_by_pairs_per_chunk": {str(k): timed(lambda: ops.thin_masks(cleaned, nbr, pairs=k), r) * 1e3 for k in (1, 2, 4, 8, 16, 32, 64)},
    }
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "features_centerline", "bench_centerline.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


def dedupe_leg(args):
    """The polygon path with the reference between the table and the edges, beside the path without it."""

    import torch

    from robosat_amd import ops, png
    from robosat_amd.colors import make_palette
    from robosat_amd.features import dedupe_keep

    size, eps, r, threshold = args.size, args.eps, args.repeat, 0.5
    masks = blob_masks(args.batch, size, 0)
    reference = np.roll(masks, (5, 7), axis=(1, 2))  # the same objects a little off ...
    reference[1::2] = blob_masks(args.batch, size, 2)[1::2]  # ... and, in every other tile, others
    dev, ref = torch.from_numpy(masks).to("cuda:0"), torch.from_numpy(reference).to("cuda:0")

    def plain():
        labels = ops.label_components(ops.clean_masks(dev, 1, eps, eps))
        table = ops.component_table(labels, 0)
        return table, ops.boundary_edges(labels, table).cpu()

    def deduped():
        labels = ops.label_components(ops.clean_masks(dev, 1, eps, eps))
        table = ops.component_table(labels, 0)
        ref_labels = ops.label_components(ops.clean_masks(ref, 1, 0, 0))
        pairs = ops.overlap_table(labels, ref_labels)
        keep, _ = dedupe_keep(table.cpu().numpy(), ops.component_table(ref_labels, 0).cpu().numpy(), pairs.cpu().numpy(), threshold)
        table = table[torch.from_numpy(keep).to(table.device)].contiguous()
        return table, ops.boundary_edges(labels, table).cpu(), pairs

    full = torch.ones((args.batch, size, size), dtype=torch.uint8, device="cuda:0")
    yy, xx = np.mgrid[:size, :size]
    board = torch.from_numpy(np.repeat(((yy + xx) % 2 == 0)[None], args.batch, 0).astype(np.uint8)).to("cuda:0")
    if args.stage_loop:
        for masks_u8 in (full, board):
            labels = ops.label_components(masks_u8)
            for _ in range(args.stage_loop):
                ops.overlap_table(labels, labels, capacity=1 << 23)
        for _ in range(args.stage_loop):
            deduped()
        return

    labels = ops.label_components(ops.clean_masks(dev, 1, eps, eps))
    table = ops.component_table(labels, 0)
    ref_labels = ops.label_components(ops.clean_masks(ref, 1, 0, 0))
    ref_table = ops.component_table(ref_labels, 0)
    kept, _, pairs = deduped()
    t_np, r_np, p_np = table.cpu().numpy(), ref_table.cpu().numpy(), pairs.cpu().numpy()
    t0 = time.perf_counter()
    for _ in range(r):
        dedupe_keep(t_np, r_np, p_np, threshold)
    host = (time.perf_counter() - t0) / r
    sec_plain, sec_dedupe = timed(plain, r), timed(deduped, r)
    result = {"batch": args.batch, "size": size, "eps": eps, "threshold": threshold,
              "components": int(len(table)), "reference_components": int(len(ref_table)), "pairs": int(len(pairs)), "kept": int(len(kept)),
              "ms_per_batch": {"without": sec_plain * 1e3, "with": sec_dedupe * 1e3},
              "ms_split": {"reference_select_and_label": timed(lambda: ops.label_components(ops.clean_masks(ref, 1, 0, 0)), r) * 1e3,
                           "reference_table": timed(lambda: ops.component_table(ref_labels, 0), r) * 1e3,
                           "overlap_table": timed(lambda: ops.overlap_table(labels, ref_labels), r) * 1e3,
                           "dedupe_keep_host": host * 1e3},
              "overlap_table_bounds": {}}
    for name, masks_u8 in (("all_ones", full), ("checkerboard", board)):
        hard = ops.label_components(masks_u8)
        rows = ops.overlap_table(hard, hard, capacity=1 << 23)
        result["overlap_table_bounds"][name] = {
            "rows": int(len(rows)),
            "overlap_table_ms_capacity_2p23": timed(lambda: ops.overlap_table(hard, hard, capacity=1 << 23), r) * 1e3,
            "overlap_table_ms_default_capacity": timed(lambda: ops.overlap_table(hard, hard), r) * 1e3,
            "label_components_ms": timed(lambda: ops.label_components(masks_u8), r) * 1e3}

    with tempfile.TemporaryDirectory() as tmp:
        count = 4 * args.batch
        tiles = blob_masks(count, size, 1)
        mapped = np.roll(tiles, (5, 7), axis=(1, 2))
        mapped[1::2] = blob_masks(count, size, 3)[1::2]
        for root, stack in (("masks", tiles), ("labels", mapped)):
            for i, image in enumerate(stack):
                os.makedirs(os.path.join(tmp, root, "18", str(69000 + i // 8)), exist_ok=True)
                png.write_png(os.path.join(tmp, root, "18", str(69000 + i // 8), str(104000 + i % 8) + ".png"), image, "P",
                              make_palette("denim", "orange"))
        with open(os.path.join(tmp, "dataset.toml"), "w") as fp:
            fp.write('[common]\nclasses = ["background", "parking"]\ncolors = ["denim", "orange"]\n')
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        cmd = [sys.executable, "-m", "robosat_amd.tools", "features", os.path.join(tmp, "masks"), "--type", "parking", "--dataset",
               os.path.join(tmp, "dataset.toml"), os.path.join(tmp, "out.geojson"), "--batch_size", str(args.batch)]
        result["cli"] = {"tiles": count, "note": "seconds includes interpreter start, torch import and library load"}
        for name, extra in (("without", []), ("with", ["--dedupe", os.path.join(tmp, "labels"), "--dedupe_threshold", str(threshold)])):
            subprocess.run(cmd + extra, env=env, cwd=ROOT, check=True, capture_output=True)  # (warm file cache)
            t0 = time.perf_counter()
            done = subprocess.run(cmd + extra, env=env, cwd=ROOT, check=True, capture_output=True, text=True)
            result["cli"][name] = {"seconds": time.perf_counter() - t0}
            with open(os.path.join(tmp, "out.geojson")) as fp:
                result["cli"][name]["features"] = len(json.load(fp)["features"])
            if extra:
                result["cli"][name]["stderr_last_line"] = done.stderr.strip().splitlines()[-1]

    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "features_dedupe", "bench_dedupe.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


SCORE_PHASES = ["blobs_k1", "blobs_k3", "all_ones_k1", "all_ones_k3", "checkerboard_k1", "checkerboard_k3"]  # (the stage loop's order)


def score_phases(path, loop):
    """The kernel trace of `--score-leg --stage-loop N` (rocprofv3's *_kernel_trace.csv) -> median us per launch of the table's and the
    scores' kernels in each of the loop's phases.  An iteration ends with its `score_sum_kernel`; of the kernels a table launched twice
    (a second pass with the exact capacity) the last launch counts."""

    import csv
    import statistics

    names = ("score_sum_kernel", "score_rows_kernel", "comp_stats_kernel", "comp_roots_kernel", "comp_filter_kernel")
    with open(path) as fp:
        rows = sorted(csv.DictReader(fp), key=lambda r: int(r["Start_Timestamp"]))
    iterations, current = [], {}
    for row in rows:
        name = next((n for n in names if n in row["Kernel_Name"]), None)
        if name is None:
            continue
        current[name] = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
        if name == "score_sum_kernel":
            iterations.append(current)
            current = {}
    if len(iterations) != loop * len(SCORE_PHASES):
        raise SystemExit("{} iterations in {}, {} x {} expected".format(len(iterations), path, len(SCORE_PHASES), loop))
    result = {"loop": loop, "us_per_launch_median": {}}
    for i, phase in enumerate(SCORE_PHASES):
        chunk = iterations[i * loop:(i + 1) * loop]
        result["us_per_launch_median"][phase] = {n: round(statistics.median(c[n] for c in chunk), 2) for n in names}
    print(json.dumps(result, indent=1, sort_keys=True))


def score_leg(args):
    """The polygon path with the scoring stage between the table and the edges, beside the path without it."""

    if args.phases:
        return score_phases(args.phases, args.stage_loop)

    import torch

    from robosat_amd import ops
    from robosat_amd.features import scores_from_sums

    size, eps, r = args.size, args.eps, args.repeat
    dev = torch.from_numpy(blob_masks(args.batch, size, 0)).to("cuda:0")
    rng = np.random.RandomState(5)
    q3 = torch.from_numpy(rng.randint(0, 256, size=(3, args.batch, size, size)).astype(np.uint8)).to("cuda:0")
    quantized = {1: q3[:1].contiguous(), 3: q3}

    def plain():
        labels = ops.label_components(ops.clean_masks(dev, 1, eps, eps))
        table = ops.component_table(labels, 0)
        return table, ops.boundary_edges(labels, table).cpu()

    def scored(k):
        labels = ops.label_components(ops.clean_masks(dev, 1, eps, eps))
        table = ops.component_table(labels, 0)
        scores = scores_from_sums(ops.component_scores(labels, table, quantized[k]).cpu().numpy(), table[:, 2].cpu().numpy())
        return table, ops.boundary_edges(labels, table).cpu(), scores

    full = torch.ones((args.batch, size, size), dtype=torch.uint8, device="cuda:0")
    yy, xx = np.mgrid[:size, :size]
    board = torch.from_numpy(np.repeat(((yy + xx) % 2 == 0)[None], args.batch, 0).astype(np.uint8)).to("cuda:0")
    labels = ops.label_components(ops.clean_masks(dev, 1, eps, eps))
    table = ops.component_table(labels, 0)
    if args.stage_loop:
        for masks_u8 in (None, full, board):  # (in this order in the trace: blobs, all ones, checkerboard; K = 1 then K = 3)
            hard = labels if masks_u8 is None else ops.label_components(masks_u8)
            rows = table if masks_u8 is None else ops.component_table(hard, 0)
            for k in (1, 3):
                for _ in range(args.stage_loop):
                    ops.component_table(hard, 0)
                    ops.component_scores(hard, rows, quantized[k])
        return

    result = {"batch": args.batch, "size": size, "eps": eps, "components": int(len(table)),
              "foreground": float((labels != 0).float().mean()),
              "ms_per_batch": {"without": timed(plain, r) * 1e3, "with_k1": timed(lambda: scored(1), r) * 1e3,
                               "with_k3": timed(lambda: scored(3), r) * 1e3},
              "ms_split": {"component_table": timed(lambda: ops.component_table(labels, 0), r) * 1e3}, "bounds": {}}
    result["ms_per_batch"]["without_again"] = timed(plain, r) * 1e3  # (the spread of the same path in the same process)
    for k in (1, 3):
        result["ms_split"]["component_scores_k{}".format(k)] = timed(lambda: ops.component_scores(labels, table, quantized[k]), r) * 1e3
        result["ms_split"]["component_scores_k{}_with_copy_to_host".format(k)] = timed(
            lambda: ops.component_scores(labels, table, quantized[k]).cpu(), r) * 1e3
    for name, masks_u8 in (("all_ones", full), ("checkerboard", board)):
        hard = ops.label_components(masks_u8)
        rows = ops.component_table(hard, 0)
        entry = {"rows": int(len(rows)), "component_table_ms": timed(lambda: ops.component_table(hard, 0), r) * 1e3}
        for k in (1, 3):
            entry["component_scores_k{}_ms".format(k)] = timed(lambda: ops.component_scores(hard, rows, quantized[k]), r) * 1e3
        result["bounds"][name] = entry

    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "features_score", "bench_score.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


def width_leg(args):
    """The distance transform beside the thinning, and the centerline stages per batch without and with it."""

    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import thin_ref

    from robosat_amd import ops
    from robosat_amd.features import stitch_tables
    from robosat_amd.tiles import Tile

    n, size, eps, r, radius = args.width_block, args.size, args.eps, args.repeat, args.max_width // 2 + 2
    batch = np.stack([thin_ref.roads(size, size, seed, count=6, width=22) for seed in range(args.batch)]).astype(np.uint8)
    block = thin_ref.roads(n * size, n * size, 100, count=6 * n, width=22).astype(np.uint8)
    tiles = np.stack([block[y * size:(y + 1) * size, x * size:(x + 1) * size] for x in range(n) for y in range(n)])
    nbr, origin, _ = stitch_tables([Tile(x, y, 18) for x in range(n) for y in range(n)], (size, size))
    dev, dev_tiles = torch.from_numpy(batch).to("cuda:0"), torch.from_numpy(tiles).to("cuda:0")
    nbr, origin = torch.from_numpy(nbr).to("cuda:0"), torch.from_numpy(origin).to("cuda:0")

    def per_tile(width):
        cleaned = ops.clean_masks(dev, 1, eps, eps)
        labels = ops.label_components(cleaned)
        table = ops.component_table(labels, 0)
        links = ops.skeleton_links(ops.thin_masks(cleaned), labels, table).cpu()
        if width:  # (the skeleton's pixels stand in for the pruned chains: the same few thousand coordinates up, their values back)
            d2 = ops.distance_transform(cleaned, radius)
            at = links[:, [0, 3, 2]].to("cuda:0")
            return links, ops.sample_pixels(d2, at).cpu()
        return links

    def stitched(width):
        if not width:
            return ops.stitched_centerlines(dev_tiles, nbr, origin, 1, eps, eps, 0)[1].cpu()
        _, links, d2 = ops.stitched_centerlines(dev_tiles, nbr, origin, 1, eps, eps, 0, width_radius=radius)
        links = links.cpu()
        slot = torch.div(links[:, 1], size, rounding_mode="floor") * n + torch.div(links[:, 2], size, rounding_mode="floor")
        at = torch.stack([slot, links[:, 2] % size, links[:, 1] % size], dim=1).to(torch.int32).to("cuda:0")
        return links, ops.sample_pixels(d2, at).cpu()

    if args.stage_loop:
        for _ in range(args.stage_loop):
            per_tile(not args.without_only)
            stitched(not args.without_only)
        return

    result = {"batch": args.batch, "size": size, "eps": eps, "block": n, "max_width": args.max_width, "radius": radius, "repeat": r,
              "per_tile": {}, "stitched": {"tiles": len(tiles)}}
    # alternating, so that a drift of the machine shows in both
    rounds = {"per_tile": {False: [], True: []}, "stitched": {False: [], True: []}}
    for _ in range(3):
        for width in ((False,) if args.without_only else (False, True)):
            rounds["per_tile"][width].append(timed(lambda: per_tile(width), r) * 1e3)
            rounds["stitched"][width].append(timed(lambda: stitched(width), r) * 1e3)
    for name in ("per_tile", "stitched"):
        result[name]["centerline_stages_ms_without_width_3_rounds"] = rounds[name][False]
        if not args.without_only:
            result[name]["centerline_stages_ms_with_width_3_rounds"] = rounds[name][True]
    if not args.without_only:
        cleaned = ops.clean_masks(dev, 1, eps, eps)
        d2 = ops.distance_transform(cleaned, radius)
        result["per_tile"].update({
            "foreground_cleaned": float(cleaned.float().mean()), "capped_share_of_foreground": float((d2 == radius * radius).float().sum() / cleaned.sum()),
            "ms_split": {"thin": timed(lambda: ops.thin_masks(cleaned), r) * 1e3,
                         "distance_transform": timed(lambda: ops.distance_transform(cleaned, radius), r) * 1e3,
                         "distance_transform_radius_128": timed(lambda: ops.distance_transform(cleaned, 128), r) * 1e3,
                         "distance_transform_all_ones_radius_128": timed(
                             lambda: ops.distance_transform(torch.ones_like(cleaned), 128), r) * 1e3}})
        cleaned_tiles = ops.clean_masks_stitched(dev_tiles, nbr, 1, eps, eps)
        result["stitched"]["ms_split"] = {"thin": timed(lambda: ops.thin_masks(cleaned_tiles, nbr), r) * 1e3,
                                          "distance_transform": timed(lambda: ops.distance_transform(cleaned_tiles, radius, nbr), r) * 1e3,
                                          "distance_transform_ignoring_seams": timed(lambda: ops.distance_transform(cleaned_tiles, radius), r) * 1e3}
        try:
            from scipy import ndimage

            host = cleaned.cpu().numpy() != 0
            t0 = time.perf_counter()
            for m in host:
                ndimage.distance_transform_edt(np.pad(m, radius, constant_values=True))
            result["per_tile"]["scipy_distance_transform_edt_ms_one_process"] = (time.perf_counter() - t0) * 1e3
        except ImportError as exc:
            result["per_tile"]["scipy_distance_transform_edt_ms_one_process"] = "skipped: {}".format(exc)
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "features_width", "bench_width.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


def split_leg(args):
    """The regrowth at every candidate K, and the polygon stages without and with `--split`."""

    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import split_ref

    from robosat_amd import ops
    from robosat_amd.features import stitch_tables
    from robosat_amd.tiles import Tile

    n, size, r, radius = args.width_block, args.size, args.repeat, args.split_radius
    batch = np.stack([split_ref.touching_blobs(size, size, seed, radius=14, salt=0) for seed in range(args.batch)]).astype(np.uint8)
    block = split_ref.touching_blobs(n * size, n * size, 100, radius=14, salt=0).astype(np.uint8)
    tiles = np.stack([block[y * size:(y + 1) * size, x * size:(x + 1) * size] for x in range(n) for y in range(n)])
    nbr, origin, _ = stitch_tables([Tile(x, y, 18) for x in range(n) for y in range(n)], (size, size))
    dev, dev_tiles = torch.from_numpy(batch).to("cuda:0"), torch.from_numpy(tiles).to("cuda:0")
    nbr, origin = torch.from_numpy(nbr).to("cuda:0"), torch.from_numpy(origin).to("cuda:0")

    def start_of(cleaned, labels, table):
        d2 = ops.distance_transform(cleaned, radius, table)
        cores = (d2 == radius * radius).to(torch.uint8)  # (the bench's own threshold: ops.split_labels has a kernel for it)
        seeds = ops.label_components(cores)
        if table is not None:
            seeds = ops.stitch_labels(seeds, table, inplace=True)
        return cores, ops.split_seeds(labels, seeds, stitched=table is not None)

    labels = ops.label_components(dev)
    cores, start = start_of(dev, labels, None)
    work = {}

    def grow(steps=None, source=start, table=None):
        buf = work.setdefault(tuple(source.shape), torch.empty_like(source))
        buf.copy_(source)
        return ops.grow_labels(buf, table, steps, want_steps=True)

    if args.stage_loop:
        with ops.knob("grow_fused", args.fused):
            for _ in range(args.stage_loop):
                grow()
        return

    final, _ = grow(1)
    final = final.clone()
    block_h, block_w, rule = ops.grow_config()
    result = {"batch": args.batch, "size": size, "radius": radius, "repeat": r, "block": [block_h, block_w], "fused_rule": rule,
              "default_steps_per_chunk": ops.GROW_STEPS, "per_tile": {}, "stitched": {"tiles": len(tiles)}}
    result["per_tile"].update({
        "foreground": float(dev.float().mean()), "unassigned_share_of_foreground": float((start == -1).float().sum() / dev.sum()),
        "components": int(len(ops.component_table(labels, 0))), "instances": int(len(ops.component_table(final, 0))),
        "steps_to_converge": grow(1)[1], "copy_of_the_start_raster_ms": timed(lambda: work[tuple(start.shape)].copy_(start), r) * 1e3})
    # alternating rounds, so that a drift of the machine shows in every K
    by_fused = {k: [] for k in (1, 2, 4, 6, 8, 12, 16)}
    for _ in range(3):
        for k in by_fused:
            with ops.knob("grow_fused", k):
                got, _ = grow()
                assert torch.equal(got, final), "fused = {} changes the result".format(k)
                by_fused[k].append(timed(grow, r) * 1e3)
    result["per_tile"]["grow_ms_by_fused_steps_3_rounds"] = {str(k): v for k, v in by_fused.items()}
    result["per_tile"]["grow_ms_by_steps_per_chunk"] = {str(c): timed(lambda: grow(c), r) * 1e3 for c in (8, 16, 24, 32, 48, 64, 128)}
    grid = {"{}x{}".format(k, c): [] for k in (8, 12, 16) for c in (16, 32, 48)}  # fused steps x steps per chunk, alternating
    for _ in range(3):
        for k in (8, 12, 16):
            with ops.knob("grow_fused", k):
                for c in (16, 32, 48):
                    grid["{}x{}".format(k, c)].append(timed(lambda: grow(c), r) * 1e3)
    result["per_tile"]["grow_ms_by_fused_x_chunk_3_rounds"] = grid
    result["per_tile"]["grow_ms_by_steps_per_chunk_fused_1"] = {}
    with ops.knob("grow_fused", 1):
        for c in (8, 16, 32, 64):
            result["per_tile"]["grow_ms_by_steps_per_chunk_fused_1"][str(c)] = timed(lambda: grow(c), r) * 1e3
    seeds = ops.label_components(cores)
    result["per_tile"]["ms_split"] = {
        "label": timed(lambda: ops.label_components(dev), r) * 1e3,
        "distance_transform": timed(lambda: ops.distance_transform(dev, radius), r) * 1e3,
        "label_cores": timed(lambda: ops.label_components(cores), r) * 1e3,
        "split_seeds": timed(lambda: ops.split_seeds(labels, seeds), r) * 1e3,
        "grow": timed(grow, r) * 1e3,
        "split_labels": timed(lambda: ops.split_labels(dev, labels, radius), r) * 1e3}

    def polygons(split):
        lab = ops.label_components(dev)
        if split:
            lab = ops.split_labels(dev, lab, radius)
        table = ops.component_table(lab, 0)
        return ops.boundary_edges(lab, table).cpu()

    def polygons_stitched(split):
        lab = ops.stitch_labels(ops.label_components(dev_tiles), nbr, inplace=True)
        if split:
            lab = ops.split_labels(dev_tiles, lab, radius, nbr)
        table = ops.component_table_stitched(lab, origin, 0)
        return ops.boundary_edges_stitched(lab, nbr, origin, table).cpu()

    rounds = {"per_tile": {False: [], True: []}, "stitched": {False: [], True: []}}
    for _ in range(3):
        for split in (False, True):
            rounds["per_tile"][split].append(timed(lambda: polygons(split), r) * 1e3)
            rounds["stitched"][split].append(timed(lambda: polygons_stitched(split), r) * 1e3)
    for name in ("per_tile", "stitched"):
        result[name]["label_table_edges_ms_without_split_3_rounds"] = rounds[name][False]
        result[name]["label_table_edges_ms_with_split_3_rounds"] = rounds[name][True]

    stitched_labels = ops.stitch_labels(ops.label_components(dev_tiles), nbr, inplace=True)
    _, stitched_start = start_of(dev_tiles, stitched_labels, nbr)
    stitched_final = grow(1, stitched_start, nbr)[0].clone()
    result["stitched"].update({"instances": int(len(ops.component_table_stitched(stitched_final, origin, 0))),
                               "steps_to_converge": grow(1, stitched_start, nbr)[1], "grow_ms_by_fused_steps": {}})
    for k in (1, 8, 16):
        with ops.knob("grow_fused", k):
            assert torch.equal(grow(None, stitched_start, nbr)[0], stitched_final)
            result["stitched"]["grow_ms_by_fused_steps"][str(k)] = timed(lambda: grow(None, stitched_start, nbr), r) * 1e3
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "features_split", "bench_split.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


EVALUATE_PHASES = ["blobs", "one_cell", "random"]  # (the stage loop's order)


def evaluate_phases(path, loop):
    """The kernel trace of `--evaluate-leg --stage-loop N` (rocprofv3's *_kernel_trace.csv) -> median us per launch of the counting
    kernels and of the label histogram (its two launches, one per raster, summed) in each of the loop's phases (in the trace in the
    loop's order; the boundary kernel runs on the blob batch alone)."""

    import csv
    import statistics

    names = ("eval_confusion_kernel", "eval_boundary_kernel", "label_histogram_kernel")
    with open(path) as fp:
        rows = sorted(csv.DictReader(fp), key=lambda r: int(r["Start_Timestamp"]))
    result = {"loop": loop, "us_per_launch_median": {}}
    for name in names:
        times = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        phases = EVALUATE_PHASES if name != "eval_boundary_kernel" else EVALUATE_PHASES[:1]
        per = 2 if name == "label_histogram_kernel" else 1  # (one launch per raster: an iteration's two are summed)
        if len(times) != per * loop * len(phases):
            raise SystemExit("{} launches of {} in {}, {} x {} x {} expected".format(len(times), name, path, len(phases), loop, per))
        times = [sum(times[i:i + per]) for i in range(0, len(times), per)]
        for i, phase in enumerate(phases):
            key = name if per == 1 else name + "_both_rasters"
            result["us_per_launch_median"].setdefault(phase, {})[key] = round(statistics.median(times[i * loop:(i + 1) * loop]), 2)
    print(json.dumps(result, indent=1, sort_keys=True))


def evaluate_leg(args):
    """`rs evaluate`: the counting pass alone, with the boundary band and with the object stages, beside the polygon stages of
    `rs features` on the same tiles; and the counting kernel at its bounds beside the label histogram over the same bytes."""

    if args.phases:
        return evaluate_phases(args.phases, args.stage_loop)

    import torch

    from robosat_amd import ops
    from robosat_amd.evaluate import match_objects

    size, eps, r, d = args.size, args.eps, args.repeat, args.boundary
    blobs = blob_masks(args.batch, size, 0)
    predicted = torch.from_numpy(blobs).to("cuda:0")
    actual = torch.from_numpy(np.roll(blobs, (3, 5), axis=(1, 2))).to("cuda:0")  # the labels: the same blobs a few pixels away
    rng = np.random.RandomState(9)
    bounds = {
        "blobs": (predicted, actual),
        "one_cell": (torch.ones_like(predicted), torch.ones_like(predicted)),
        "random": tuple(torch.from_numpy(rng.randint(0, 8, size=blobs.shape).astype(np.uint8)).to("cuda:0") for _ in range(2)),
    }
    classes = {"blobs": 2, "one_cell": 2, "random": 8}
    hist = torch.zeros(256, dtype=torch.int64, device="cuda:0")

    def confusion():
        counts, bad = ops.mask_confusion(predicted, actual, 2)
        return counts.cpu(), bad.cpu()

    def masks():
        return ops.clean_masks(predicted, 1, 0, 0), ops.clean_masks(actual, 1, 0, 0)

    def boundary():
        mask_p, mask_g = masks()
        return confusion(), ops.boundary_counts(ops.distance_transform(mask_p, d + 1), ops.distance_transform(mask_g, d + 1), d).cpu()

    def objects():
        mask_p, mask_g = masks()
        labels_p, labels_g = ops.label_components(mask_p), ops.label_components(mask_g)
        table_p, table_g = ops.component_table(labels_p, 0), ops.component_table(labels_g, 0)
        pairs = ops.overlap_table(labels_p, labels_g)
        return confusion(), match_objects(table_p.cpu().numpy(), table_g.cpu().numpy(), pairs.cpu().numpy(), 0.5, False)

    def features():
        labels = ops.label_components(ops.clean_masks(predicted, 1, eps, eps))
        table = ops.component_table(labels, 0)
        return table, ops.boundary_edges(labels, table).cpu()

    if args.stage_loop:
        for name in EVALUATE_PHASES:  # (in this order in the trace)
            p, a = bounds[name]
            for _ in range(args.stage_loop):
                ops.mask_confusion(p, a, classes[name])
                ops.label_histogram_u8(p.view(-1), hist)
                ops.label_histogram_u8(a.view(-1), hist)
        mask_p, mask_g = masks()
        d2_p, d2_g = ops.distance_transform(mask_p, d + 1), ops.distance_transform(mask_g, d + 1)
        for _ in range(args.stage_loop):
            ops.boundary_counts(d2_p, d2_g, d)
        torch.cuda.synchronize()
        return

    labels = ops.label_components(ops.clean_masks(predicted, 1, eps, eps))
    matched = objects()[1]
    mask_p, mask_g = masks()
    labels_p, labels_g = ops.label_components(mask_p), ops.label_components(mask_g)
    tables = [t.cpu().numpy() for t in (ops.component_table(labels_p, 0), ops.component_table(labels_g, 0), ops.overlap_table(labels_p, labels_g))]
    result = {"batch": args.batch, "size": size, "eps": eps, "boundary": d, "block_pixels": ops.eval_config(),
              "objects": {"matched": matched[0], "predicted": matched[1], "actual": matched[2], "pairs": int(len(tables[2]))},
              "ms_per_batch": {"confusion": timed(confusion, r) * 1e3, "with_boundary": timed(boundary, r) * 1e3,
                               "with_objects": timed(objects, r) * 1e3, "features_clean_label_table_edges": timed(features, r) * 1e3},
              "ms_split": {"component_table": timed(lambda: ops.component_table(labels, 0), r) * 1e3,
                           "mask_confusion_no_copy": timed(lambda: ops.mask_confusion(predicted, actual, 2), r) * 1e3,
                           "match_objects_on_the_host": timed(lambda: match_objects(tables[0], tables[1], tables[2], 0.5, False), r) * 1e3,
                           "overlap_table": timed(lambda: ops.overlap_table(labels_p, labels_g), r) * 1e3,
                           "component_table_unopened": timed(lambda: ops.component_table(labels_p, 0), r) * 1e3},
              "bounds_us_per_call": {}}
    result["ms_per_batch"]["confusion_again"] = timed(confusion, r) * 1e3  # (the spread of the same path in the same process)
    for name in EVALUATE_PHASES:  # (calls enqueued back to back: launch + memsets of the outputs, no copy to the host)
        p, a = bounds[name]
        result["bounds_us_per_call"][name] = {
            "mask_confusion": timed(lambda: ops.mask_confusion(p, a, classes[name]), 10 * r) * 1e6,
            "label_histogram_u8_both_rasters": timed(lambda: (ops.label_histogram_u8(p.view(-1), hist), ops.label_histogram_u8(a.view(-1), hist)),
                                                     10 * r) * 1e6,
        }

    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "evaluate", "bench_evaluate.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


PROBS_PHASES = ["blobs", "one_byte", "random", "small_tiles"]  # (the stage loop's order)


def probs_rasters(batch, size):
    """The labels (the blob batch, classes 0 / 1) and the probability rasters of `--evaluate-probs-leg`, as numpy: blob-like
    (the blobs a few pixels away, saturated to bytes 1 and 254 with a soft edge: a 5 x 5 mean of the mask), all one byte, and
    uniformly random bytes; `small_tiles`: the first blob-like tile and its labels as (size / 8)^2 tiles of 8 x 8, so that a block
    of 4 096 pixels holds 64 groups."""

    blobs = blob_masks(batch, size, 0)
    moved = np.roll(blobs, (3, 5), axis=(1, 2)).astype(np.float64)
    mean = sum(np.roll(moved, (dy, dx), axis=(1, 2)) for dy in range(-2, 3) for dx in range(-2, 3)) / 25.0
    soft = (1 + np.rint(253 * mean)).astype(np.uint8)
    rng = np.random.RandomState(9)
    return {
        "blobs": (soft, blobs),
        "one_byte": (np.ones_like(blobs), blobs),
        "random": (rng.randint(0, 256, size=blobs.shape).astype(np.uint8), blobs),
        "small_tiles": (soft[0].reshape(-1, 8, 8), blobs[0].reshape(-1, 8, 8)),
    }


def probs_phases(path, loop):
    """The kernel trace of `--evaluate-probs-leg --stage-loop N` (rocprofv3's *_kernel_trace.csv) -> median us per launch of the
    probability histogram, of the confusion kernel on the same two rasters and of the label histogram (its two launches, one per
    raster, summed) in each of the loop's phases, and the ratio of the first to the second."""

    import csv
    import statistics

    names = ("eval_prob_hist_kernel", "eval_confusion_kernel", "label_histogram_kernel")
    with open(path) as fp:
        rows = sorted(csv.DictReader(fp), key=lambda r: int(r["Start_Timestamp"]))
    result = {"loop": loop, "us_per_launch_median": {}, "prob_hist_over_confusion": {},
              "note": "eval_confusion_kernel reads the probability bytes as class indices here: a byte above 1 is no class, so on the blob-like "
                      "and the random raster most pixels meet in its one bad counter per tile, its slow bound. A ratio below 1 on those "
                      "rasters says that, not that the histogram beats the confusion kernel on class rasters (5.9-7.0 us there)"}
    for name in names:
        times = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        per = 2 if name == "label_histogram_kernel" else 1
        if len(times) != per * loop * len(PROBS_PHASES):
            raise SystemExit("{} launches of {} in {}, {} x {} x {} expected".format(len(times), name, path, len(PROBS_PHASES), loop, per))
        times = [sum(times[i:i + per]) for i in range(0, len(times), per)]
        for i, phase in enumerate(PROBS_PHASES):
            key = name if per == 1 else name + "_both_rasters"
            result["us_per_launch_median"].setdefault(phase, {})[key] = round(statistics.median(times[i * loop:(i + 1) * loop]), 2)
    for phase, row in result["us_per_launch_median"].items():
        result["prob_hist_over_confusion"][phase] = round(row["eval_prob_hist_kernel"] / row["eval_confusion_kernel"], 2)
    print(json.dumps(result, indent=1, sort_keys=True))


def evaluate_probs_leg(args):
    """`rs evaluate --probs`: `ops.prob_histogram` beside `ops.mask_confusion` on the same two rasters (the yardstick: it reads the
    same bytes) and beside the label histogram over both (the design to beat), on the three probability rasters and on small tiles."""

    if args.phases:
        return probs_phases(args.phases, args.stage_loop)

    import torch

    from robosat_amd import ops

    r = args.repeat
    rasters = {name: tuple(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in pair)
               for name, pair in probs_rasters(args.batch, args.size).items()}
    hist = torch.zeros(256, dtype=torch.int64, device="cuda:0")

    if args.stage_loop:
        for name in PROBS_PHASES:  # (in this order in the trace)
            q, a = rasters[name]
            for _ in range(args.stage_loop):
                ops.prob_histogram(q, a, 2, 1)
                ops.mask_confusion(q, a, 2)
                ops.label_histogram_u8(q.view(-1), hist)
                ops.label_histogram_u8(a.view(-1), hist)
        torch.cuda.synchronize()
        return

    result = {"batch": args.batch, "size": args.size, "block_pixels": ops.eval_config(), "us_per_call": {}, "nonempty_bins": {}}
    for name in PROBS_PHASES:  # (calls enqueued back to back: launch + the fill of the outputs, no copy to the host)
        q, a = rasters[name]
        counts = ops.prob_histogram(q, a, 2, 1)[0]
        result["nonempty_bins"][name] = {"tiles": int(counts.shape[0]), "per_tile_mean": float((counts > 0).sum().item() / counts.shape[0])}
        result["us_per_call"][name] = {
            "prob_histogram": timed(lambda: ops.prob_histogram(q, a, 2, 1), 10 * r) * 1e6,
            "mask_confusion": timed(lambda: ops.mask_confusion(q, a, 2), 10 * r) * 1e6,
            "label_histogram_u8_both_rasters": timed(lambda: (ops.label_histogram_u8(q.view(-1), hist), ops.label_histogram_u8(a.view(-1), hist)),
                                                     10 * r) * 1e6,
        }
    q, a = rasters["blobs"]
    result["ms_per_batch_with_copy"] = {
        "prob_histogram": timed(lambda: ops.prob_histogram(q, a, 2, 1)[0].cpu(), r) * 1e3,
        "mask_confusion": timed(lambda: ops.mask_confusion(q, a, 2)[0].cpu(), r) * 1e3,
    }
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "evaluate_probs", "bench_evaluate_probs.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


def device_stage(images, eps):
    import torch

    from robosat_amd import ops

    dev = torch.from_numpy(images).to("cuda:0")
    labels = ops.label_components(ops.clean_masks(dev, 1, eps, eps))
    table = ops.component_table(labels, 0)
    edges = ops.boundary_edges(labels, table)
    return table.cpu().numpy(), edges.cpu().numpy()


def _cpu_tile(args):
    from scipy import ndimage

    image, eps, disc = args
    m = image == 1
    m = ndimage.binary_dilation(ndimage.binary_erosion(m, disc, border_value=1), disc)
    m = ndimage.binary_erosion(ndimage.binary_dilation(m, disc), disc, border_value=1)
    labels, n = ndimage.label(m)
    p = np.pad(labels, 1)
    c = p[1:-1, 1:-1]
    return n, sum(int(((c != 0) & (nb != c)).sum()) for nb in (p[:-2, 1:-1], p[1:-1, 2:], p[2:, 1:-1], p[1:-1, :-2]))


def timed(fn, repeat, warmup=2):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeat):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--eps", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--stage-loop", type=int, default=0)
    ap.add_argument("--stitch-leg", action="store_true", help="only the stitched path against the per-tile path on an n x n block")
    ap.add_argument("--centerline-leg", action="store_true", help="only thinning and links, on a road network and on its n x n block")
    ap.add_argument("--dedupe-leg", action="store_true", help="only rs features --dedupe: the stages with and without the reference")
    ap.add_argument("--score-leg", action="store_true", help="only rs features --score: the stages with and without the per-component sums")
    ap.add_argument("--phases", type=str, default=None, help="--score-leg / --evaluate-leg / --evaluate-probs-leg --stage-loop N: the kernel trace of that run, split by phase (no device)")
    ap.add_argument("--width-leg", action="store_true", help="only rs features --width: the distance transform beside the thinning")
    ap.add_argument("--without-only", action="store_true", help="--width-leg: only the stages without the transform")
    ap.add_argument("--max-width", type=int, default=64, help="--width-leg: as --max_width of rs features (radius N // 2 + 2)")
    ap.add_argument("--width-block", type=int, default=4, help="--width-leg: tiles per side of the stitched call")
    ap.add_argument("--split-leg", action="store_true", help="only rs features --split: the regrowth at every number of fused steps")
    ap.add_argument("--split-radius", type=int, default=8, help="--split-leg: as --split of rs features")
    ap.add_argument("--fused", type=int, default=0, help="--split-leg --stage-loop: the knob grow_fused (0 = the rule)")
    ap.add_argument("--evaluate-leg", action="store_true", help="only rs evaluate: the counting pass, the boundary band and the object stages")
    ap.add_argument("--boundary", type=int, default=3, help="--evaluate-leg: as --boundary of rs evaluate")
    ap.add_argument("--evaluate-probs-leg", action="store_true",
                    help="only rs evaluate --probs: the probability histogram beside the confusion kernel and the label histogram")
    ap.add_argument("--block", type=int, default=8, help="tiles per side of the stitched legs' block")
    ap.add_argument("--out", type=str, default=DEFAULT_OUT)
    args = ap.parse_args()
    if args.stitch_leg:
        return stitch_leg(args)
    if args.centerline_leg:
        return centerline_leg(args)
    if args.dedupe_leg:
        return dedupe_leg(args)
    if args.score_leg:
        return score_leg(args)
    if args.width_leg:
        return width_leg(args)
    if args.split_leg:
        return split_leg(args)
    if args.evaluate_leg:
        return evaluate_leg(args)
    if args.evaluate_probs_leg:
        return evaluate_probs_leg(args)

    import torch

    from robosat_amd import ops

    inputs = {"blobs": blob_masks(args.batch, args.size, 0), "noise": noise_masks(args.batch, args.size, 0)}
    if args.stage_loop:
        for _ in range(args.stage_loop):
            device_stage(inputs["blobs"], args.eps)
        return

    result = {"batch": args.batch, "size": args.size, "eps": args.eps, "device": {}, "cpu": {}, "forms": {}, "labeller": {}}
    for name, images in inputs.items():
        table, edges = device_stage(images, args.eps)
        sec = timed(lambda: device_stage(images, args.eps), args.repeat)
        dev = torch.from_numpy(images).to("cuda:0")
        clean = ops.clean_masks(dev, 1, args.eps, args.eps)
        labels = ops.label_components(clean)
        split = {
            "upload": timed(lambda: torch.from_numpy(images).to("cuda:0"), args.repeat),
            "clean": timed(lambda: ops.clean_masks(dev, 1, args.eps, args.eps), args.repeat),
            "label": timed(lambda: ops.label_components(clean), args.repeat),
            "table": timed(lambda: ops.component_table(labels, 0), args.repeat),
        }
        kept = ops.component_table(labels, 0)
        split["edges"] = timed(lambda: ops.boundary_edges(labels, kept).cpu(), args.repeat)  # (with the list's copy to the host)
        result["device"][name] = {
            "tiles_per_s": args.batch / sec, "ms_per_batch": sec * 1e3, "foreground": float((images == 1).mean()),
            "components": int(len(table)), "edges": int(len(edges)), "ms_split": {k: v * 1e3 for k, v in split.items()},
        }

    try:
        import multiprocessing

        from scipy import ndimage  # noqa: F401

        disc = ops.disc(args.eps).astype(bool)
        with multiprocessing.get_context("spawn").Pool(min(16, os.cpu_count() or 1)) as pool:
            for name, images in inputs.items():
                work = [(im, args.eps, disc) for im in images]
                pool.map(_cpu_tile, work)
                t0 = time.perf_counter()
                pool.map(_cpu_tile, work)
                result["cpu"][name] = {"tiles_per_s": args.batch / (time.perf_counter() - t0), "processes": min(16, os.cpu_count() or 1)}
    except ImportError as exc:
        result["cpu"] = {"skipped": str(exc)}

    dev = torch.from_numpy(inputs["blobs"]).to("cuda:0")
    for name, form in (("lds", ops.CLEAN_LDS), ("hbm", ops.CLEAN_HBM)):
        if form == ops.CLEAN_LDS and ops.clean_form(args.size, args.size) != ops.CLEAN_LDS:
            continue
        sec = timed(lambda: ops.clean_masks(dev, 1, args.eps, args.eps, form=form), args.repeat)
        result["forms"][name] = {"ms_per_batch": sec * 1e3, "tiles_per_s": args.batch / sec}

    # the labeller alone, on what is hard for it
    yy, xx = np.mgrid[:args.size, :args.size]
    spiral = spiral_mask(args.size)
    hard = {"noise50": noise_masks(args.batch, args.size, 3), "checkerboard": np.repeat(((yy + xx) % 2 == 0)[None], args.batch, 0),
            "spiral": np.repeat(spiral[None], args.batch, 0)}
    result["labeller"] = {}
    for name, masks in hard.items():
        dev = torch.from_numpy(np.ascontiguousarray(masks.astype(np.uint8))).to("cuda:0")
        labels = ops.label_components(dev)
        sec = timed(lambda: ops.label_components(dev), args.repeat)
        result["labeller"][name] = {"ms_per_batch": sec * 1e3, "tiles_per_s": args.batch / sec,
                                    "components": int((labels == torch.arange(1, args.size * args.size + 1, device=labels.device,
                                                                              dtype=torch.int32).view(1, args.size, args.size)).sum())}

    # ./rs features from PNGs on disk
    from robosat_amd import png
    from robosat_amd.colors import make_palette

    with tempfile.TemporaryDirectory() as tmp:
        count = 4 * args.batch
        tiles = blob_masks(count, args.size, 1)
        for i, image in enumerate(tiles):
            os.makedirs(os.path.join(tmp, "masks", "18", str(69000 + i // 8)), exist_ok=True)
            png.write_png(os.path.join(tmp, "masks", "18", str(69000 + i // 8), str(104000 + i % 8) + ".png"), image, "P",
                          make_palette("denim", "orange"))
        with open(os.path.join(tmp, "dataset.toml"), "w") as fp:
            fp.write('[common]\nclasses = ["background", "parking"]\ncolors = ["denim", "orange"]\n')
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        cmd = [sys.executable, "-m", "robosat_amd.tools", "features", os.path.join(tmp, "masks"), "--type", "parking", "--dataset",
               os.path.join(tmp, "dataset.toml"), os.path.join(tmp, "out.geojson"), "--batch_size", str(args.batch)]
        t0 = time.perf_counter()
        subprocess.run(cmd, env=env, cwd=ROOT, check=True, capture_output=True)
        whole = time.perf_counter() - t0

        from PIL import Image

        from robosat_amd.features import featurize
        from robosat_amd.tiles import Tile

        t0 = time.perf_counter()
        decoded = np.stack([np.array(Image.open(os.path.join(tmp, "masks", "18", str(69000 + i // 8), str(104000 + i % 8) + ".png")))
                            for i in range(count)])
        decode = time.perf_counter() - t0
        host = 0.0
        for start in range(0, count, args.batch):
            table, edges = device_stage(decoded[start:start + args.batch], args.eps)
            t0 = time.perf_counter()
            featurize(edges, table, [Tile(0, i, 18) for i in range(args.batch)], (args.size, args.size), 0.01)
            host += time.perf_counter() - t0
        result["cli"] = {"tiles": count, "tiles_per_s": count / whole, "seconds": whole, "png_decode_s": decode, "rings_to_features_s": host,
                         "note": "seconds includes interpreter start, torch import and library load"}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
