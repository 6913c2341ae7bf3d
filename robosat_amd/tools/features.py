"""``rs features``: class-index mask PNGs (what ``rs masks`` writes) -> simplified GeoJSON polygons of one class -- the
reference's arguments (``robosat/tools/features.py``) with its handler's thresholds as flags.  Class select, morphological
open / close, connected components and boundary extraction run on the MI355X (``csrc/features.hip``); only the boundary
edges come back to the host, which links them into rings, simplifies and georeferences them (``robosat_amd/features.py``).
The stage definitions, and where they depart from OpenCV's, are in ``include/robosat_hip.h`` and DESIGN.md."""

import argparse
import sys

import numpy as np
import torch
from PIL import Image
from tqdm import tqdm

from robosat_amd import ops
from robosat_amd.config import load_config
from robosat_amd.features import FeatureWriter, featurize
from robosat_amd.tiles import tiles_from_slippy_map


def add_parser(subparser):
    parser = subparser.add_parser(
        "features",
        help="extracts simplified GeoJSON features from segmentation masks",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter,
    )
    parser.add_argument("masks", type=str, help="slippy map directory with segmentation masks")
    parser.add_argument("--type", type=str, required=True, help="class of the dataset to extract features for")
    parser.add_argument("--dataset", type=str, required=True, help="path to dataset configuration file")
    parser.add_argument("out", type=str, help="path to GeoJSON file to store features in")
    parser.add_argument("--denoise", type=int, default=20, help="diameter in pixels of the disc the mask is opened with")
    parser.add_argument("--grow", type=int, default=20, help="diameter in pixels of the disc the mask is closed with")
    parser.add_argument("--simplify", type=float, default=0.01, help="Douglas-Peucker epsilon as a share of a ring's perimeter")
    parser.add_argument("--min_area", type=int, default=0, help="components with fewer pixels are dropped")
    parser.add_argument("--batch_size", type=int, default=16, help="tiles per device launch")
    parser.set_defaults(func=main)


def main(args):
    classes = load_config(args.dataset)["common"]["classes"]
    if args.type not in classes[1:]:
        sys.exit("Error: --type must be a non-background class of the dataset ({}), got '{}'".format(", ".join(classes[1:]), args.type))
    for name in ("denoise", "grow"):
        if not 0 <= getattr(args, name) <= 64:
            sys.exit("Error: --{} must be in 0..64".format(name))
    if not torch.cuda.is_available():
        sys.exit("Error: this build computes on the MI355X only")
    device = torch.device("cuda", 0)
    index = classes.index(args.type)

    by_shape = {}  # (H, W) -> [(tile, path)]: the header gives the size, a mask is decoded when its batch runs
    for tile, path in sorted(tiles_from_slippy_map(args.masks), key=lambda t: (t[0].z, t[0].x, t[0].y)):
        with Image.open(path) as image:
            width, height = image.size
        if not (1 <= height <= 4096 and 1 <= width <= 4096):
            sys.exit("Error: {} is {}x{}; tiles are at most 4096x4096".format(path, height, width))
        by_shape.setdefault((height, width), []).append((tile, path))

    writer = FeatureWriter()
    for shape, items in by_shape.items():  # tiles of one batch share a shape
        # (the library takes B*H*W < 2^29 per call, link_rings fewer than 1024 tiles)
        batch = max(1, min(args.batch_size, 1023, ((1 << 29) - 1) // (shape[0] * shape[1])))
        for start in tqdm(range(0, len(items), batch), desc="Features {}x{}".format(*shape), unit="batch", ascii=True):
            group = items[start:start + batch]
            images = torch.from_numpy(np.stack([np.array(Image.open(path).convert("P"), dtype=np.uint8) for _, path in group])).to(device)
            labels = ops.label_components(ops.clean_masks(images, index, args.denoise, args.grow))
            table = ops.component_table(labels, args.min_area)
            edges = ops.boundary_edges(labels, table)
            writer.add(featurize(edges.cpu().numpy(), table.cpu().numpy(), [tile for tile, _ in group], shape, args.simplify))
    writer.save(args.out)
