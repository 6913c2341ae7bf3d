#!/usr/bin/env python
"""Measures the `rs features` stages on the MI355X and writes profiles/features/bench_features.json:

  device   upload of the mask bytes -> clean -> label -> table -> edges back on the host; tiles/s at 512 x 512, batch 16,
           discs 20 / 20, on blob masks (about 10 % foreground) and on 50 % noise (which the opening empties: it times
           the morphology, not the labeller)
  labeller label_components alone on the shapes that are hard for it: 50 % noise unopened, a checkerboard, a one-pixel spiral
  cpu      the same stages through scipy.ndimage in a pool of at most 16 processes, for scale
  forms    the morphology kernel's LDS-resident form against its through-HBM form
  cli      `./rs features` from PNGs on disk, with the host share (PNG decode, ring linking, JSON)

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
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "features", "bench_features.json"))
    args = ap.parse_args()

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
