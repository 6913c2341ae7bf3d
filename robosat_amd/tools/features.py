"""``rs features``: class-index mask PNGs (what ``rs masks`` writes) -> simplified GeoJSON polygons of one class -- the
reference's arguments (``robosat/tools/features.py``) with its handler's thresholds as flags.  Class select, morphological
open / close, connected components and boundary extraction run on the MI355X (``csrc/features.hip``); only the boundary
edges come back to the host, which links them into rings, simplifies and georeferences them (``robosat_amd/features.py``).
``--stitch`` treats the tiles of a zoom level as one sparse raster, so an object that crosses tile borders is one polygon.
``--geometry centerline`` gives LineStrings for linear classes such as roads: the cleaned mask is thinned to its skeleton on the
device too, and the host links, prunes and simplifies the skeleton's lines.
``--width`` (with ``--geometry centerline``) gives every line its road's width: an exact Euclidean distance transform of the cleaned
mask, capped at ``--max_width // 2 + 2`` pixels, runs on the device beside the thinning and is sampled along the pruned lines; a line
gains ``width_px`` (the median of 2 * distance - 1 over its pixels), ``width_min_px``, ``width_max_px``, ``width_m`` and, where the
road is wider than ``--max_width``, ``width_capped``.
``--dedupe DIR`` drops the polygons the reference labels in DIR already map (the reference's ``rs dedupe``, on rasters): both
sides are labelled on the device, one kernel tabulates the pixels every pair of components shares, and a component whose
intersection over union with the reference objects it touches reaches ``--dedupe_threshold`` is left out.
``--split R`` separates objects that touch, or that a few pixels of false positive join, into instances: the cores a disc of
radius R fits into are labelled and grown back over the mask on the device (geodesic influence zones), and ``--min_area``,
``--dedupe`` and every property then apply to the instances.  Neighbouring instances are simplified one by one, so after
``--simplify`` their shared border may overlap or gap by up to the epsilon.
``--score DIR`` (one per model, as ``rs masks`` takes them) gives every polygon its confidence: the probability tiles ``rs predict``
wrote go to the device beside the labels, one kernel sums every model's bytes of the class over each component, and the host divides
once: ``score`` is the mean over the polygon's pixels, as written, of the probability ``rs masks`` votes with (``--score_weights`` as
its ``--weights``).  ``--min_score S`` drops the polygons below S.
The stage definitions, and where they depart from OpenCV's, are in ``include/robosat_hip.h`` and DESIGN.md."""

import argparse
import math
import os
import sys

import numpy as np
import torch
from PIL import Image
from tqdm import tqdm

from robosat_amd import ops
from robosat_amd.config import load_config
from robosat_amd.features import (FeatureWriter, Widths, centerlines, centerlines_stitched, dedupe_keep, featurize, featurize_stitched,
                                  group_clusters, pack_clusters, scores_from_sums, stitch_tables)
from robosat_amd.tiles import tiles_from_slippy_map
from robosat_amd.tools.masks import load_quantized


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
    parser.add_argument("--simplify", type=float, default=0.01, help="Douglas-Peucker epsilon as a share of a ring's perimeter (ignored with --geometry centerline: see --tolerance)")
    parser.add_argument("--min_area", type=int, default=0, help="components with fewer pixels are dropped")
    parser.add_argument("--batch_size", type=int, default=16, help="tiles per device launch")
    parser.add_argument("--stitch", action="store_true", help="treat the tiles of a zoom level as one raster: whole polygons across tile borders")
    parser.add_argument("--geometry", type=str, default="polygon", choices=["polygon", "centerline"],
                        help="polygon: the outline of every component; centerline: LineStrings along its skeleton (roads). Without "
                        "--stitch a centerline stops about half the road's width short of every tile border (a 20-pixel road crossing a "
                        "tile ends 9-10 pixels inside it), so roads want --stitch. --width adds the road's width to every line")
    parser.add_argument("--prune", type=float, default=20, help="centerline: side branches shorter than this many pixels are removed")
    parser.add_argument("--tolerance", type=float, default=1.5, help="centerline: Douglas-Peucker tolerance in pixels")
    parser.add_argument("--width", action="store_true",
                        help="centerline: every line gains width_px, width_min_px, width_max_px and width_m, from a distance transform of "
                        "the cleaned mask sampled along the line (the median over its pixels); an even width reads one pixel narrow")
    parser.add_argument("--max_width", type=int, default=64, metavar="N",
                        help="with --width: roads up to N pixels wide are measured (1..252); a wider one reads as its cap and is marked "
                        "width_capped. With --stitch N // 2 + 2 pixels must fit the tile's smaller side")
    parser.add_argument("--dedupe", type=str, default=None, metavar="DIR",
                        help="slippy map directory with class-index masks of what is already mapped (a dataset's labels, rasterized "
                        "OpenStreetMap): polygons they cover are dropped, the rest gain the property iou. The reference pixels are "
                        "taken as they are (no --denoise, --grow or --min_area) and only inside the tiles of the masks directory: a "
                        "reference object that runs on into a tile without a mask counts with its pixels inside those tiles alone. "
                        "A mask tile without a file in DIR has nothing mapped. With --stitch objects are compared whole across tile borders")
    parser.add_argument("--dedupe_threshold", type=float, default=None, metavar="T",
                        help="with --dedupe (required): a polygon is dropped where the pixels it shares with the reference objects it "
                        "touches are at least T times the pixels of their union, 0 <= T <= 1")
    parser.add_argument("--split", type=int, default=0, metavar="R",
                        help="polygon: separate touching objects into instances, 0 = off, else 1..64: the parts of the cleaned mask "
                        "a disc of radius R pixels fits into are labelled and grown back over the mask, so a bridge narrower than 2 R "
                        "between two objects is cut; an object no such disc fits into stays as it is. Neighbouring instances are "
                        "simplified one by one, so after --simplify their shared border may overlap or gap by up to the epsilon. "
                        "With --stitch R pixels must fit the tile's smaller side")
    parser.add_argument("--score", type=str, action="append", default=None, metavar="DIR",
                        help="polygon: slippy map directory with the class probabilities rs predict wrote for these masks; give it once "
                        "per model that rs masks voted with (at most 8). Every polygon gains the property score: the mean over its "
                        "pixels, as written (after --denoise, --grow, --stitch and --split), of the probability of --type, averaged over "
                        "the models")
    parser.add_argument("--score_weights", type=float, nargs="+", default=None, metavar="W",
                        help="with --score: one weight per directory for the average over the models, as rs masks --weights")
    parser.add_argument("--min_score", type=float, default=None, metavar="S",
                        help="with --score: polygons with a score below S are dropped (after --min_area and --split, before --dedupe), "
                        "0 <= S <= 1")
    parser.set_defaults(func=main)


def _load(paths, device):
    return torch.from_numpy(np.stack([np.array(Image.open(path).convert("P"), dtype=np.uint8) for path in paths])).to(device)


class Dedupe:
    """``--dedupe``: the reference tiles of a batch or call, and the count of what was examined and dropped."""

    def __init__(self, directory, threshold, index):
        self.paths = {tile: path for tile, path in tiles_from_slippy_map(directory)}
        self.threshold, self.index = threshold, index
        self.examined = self.dropped = 0

    def load(self, tiles, shape, device):
        """uint8 [T, H, W] class-index tiles; a tile without a file is background (the class is never index 0)."""

        planes = []
        for tile in tiles:
            path = self.paths.get(tile)
            if path is None:
                planes.append(np.zeros(shape, dtype=np.uint8))
                continue
            plane = np.array(Image.open(path).convert("P"), dtype=np.uint8)
            if plane.shape != tuple(shape):
                sys.exit("Error: {} is {}x{}; the mask tile {}/{}/{} is {}x{}".format(path, plane.shape[0], plane.shape[1], tile.z, tile.x,
                                                                                    tile.y, shape[0], shape[1]))
            planes.append(plane)
        return torch.from_numpy(np.stack(planes)).to(device)

    def filter(self, labels, table, reference_u8, nbr=None, origin=None):
        """Labels and component table of the masks + the reference tiles (``load``) -> (the table's kept rows, {feature key: iou}
        for ``featurize``).  With ``nbr`` and ``origin`` everything is stitched: labels, table and the reference."""

        reference = ops.label_components(ops.clean_masks(reference_u8, self.index, 0, 0))  # (discs of 0: tile == index as it is)
        if nbr is None:
            ref_table = ops.component_table(reference, 0)
        else:
            reference = ops.stitch_labels(reference, nbr, inplace=True)
            ref_table = ops.component_table_stitched(reference, origin, 0)
        pairs = ops.overlap_table(labels, reference, stitched=nbr is not None)
        rows = table.cpu().numpy()
        keep, iou = dedupe_keep(rows, ref_table.cpu().numpy(), pairs.cpu().numpy(), self.threshold)
        self.examined += len(keep)
        self.dropped += int((~keep).sum())
        kept = rows[keep]
        keys = [(int(r[0]), int(r[1])) for r in kept] if nbr is None else [int(r[0]) for r in kept]
        return table[torch.from_numpy(keep).to(table.device)].contiguous(), dict(zip(keys, iou[keep].tolist()))


class Score:
    """``--score``: the probability tiles of a batch or call, the scores of its components, and the count of what was scored and
    dropped.  ``channel``: the class's channel in the probability tiles (class index - 1)."""

    def __init__(self, directories, weights, channel, min_score=None):
        self.directories = list(directories)
        self.paths = [{tile: path for tile, path in tiles_from_slippy_map(directory)} for directory in self.directories]
        self.weights, self.channel, self.min_score = weights, channel, min_score
        self.scored = self.dropped = 0

    def load(self, tiles, shape, device):
        """uint8 [K, T, H, W]: every model's bytes of the class, the tiles in slot order."""

        planes, channels = [], None
        for directory, paths in zip(self.directories, self.paths):
            for tile in tiles:
                path = paths.get(tile)
                name = "{}/{}/{}".format(tile.z, tile.x, tile.y)
                if path is None:
                    sys.exit("Error: --score {} has no probabilities for the mask tile {}".format(directory, name))
                q = load_quantized(path)
                if q.shape[:2] != tuple(shape):
                    sys.exit("Error: {} is {}x{}; the mask tile {} is {}x{}".format(path, q.shape[0], q.shape[1], name, shape[0], shape[1]))
                if channels is None:
                    channels = (q.shape[2], path)
                if q.shape[2] != channels[0]:
                    sys.exit("Error: {} (tile {}) holds the probabilities of {} classes, {} those of {}: the --score directories are "
                             "of models with the same classes".format(path, name, q.shape[2] + 1, channels[1], channels[0] + 1))
                if self.channel >= q.shape[2]:
                    sys.exit("Error: {} (tile {}) holds the probabilities of {} classes; --type is class {} of the dataset".format(
                        path, name, q.shape[2] + 1, self.channel + 1))
                planes.append(np.ascontiguousarray(q[:, :, self.channel], dtype=np.uint8))
        stack = np.stack(planes).reshape(len(self.directories), len(tiles), shape[0], shape[1])
        return torch.from_numpy(stack).to(device)

    def filter(self, labels, table, quantized, stitched=False):
        """Labels and component table + the probabilities (``load``) -> (the table's kept rows, {feature key: score} for
        ``featurize``)."""

        rows = table.cpu().numpy()
        sums = ops.component_scores(labels, table, quantized, stitched=stitched).cpu().numpy()
        scores = scores_from_sums(sums, rows[:, 1 if stitched else 2], self.weights)
        keep = np.ones(len(rows), dtype=bool) if self.min_score is None else scores >= self.min_score
        self.scored += len(keep)
        self.dropped += int((~keep).sum())
        kept = rows[keep]
        keys = [int(r[0]) for r in kept] if stitched else [(int(r[0]), int(r[1])) for r in kept]
        return table[torch.from_numpy(keep).to(table.device)].contiguous(), dict(zip(keys, scores[keep].tolist()))


def width_radius(max_width):
    """Radius of the distance transform that measures a road of ``max_width`` pixels uncapped."""

    return max_width // 2 + 2


def _sampler(d2):
    """``Widths.sample`` over the raster ``d2`` on the device: the chain pixels go up, their values come back."""

    def sample(coords):
        return ops.sample_pixels(d2, torch.from_numpy(coords).to(d2.device)).cpu().numpy()

    return sample


def _tile_sizes(masks):
    """(tile, path, (height, width)) from the PNG headers, one by one in the order (z, x, y): a mask is decoded when its batch runs."""

    for tile, path in sorted(tiles_from_slippy_map(masks), key=lambda t: (t[0].z, t[0].x, t[0].y)):
        with Image.open(path) as image:
            width, height = image.size
        yield tile, path, (height, width)


def stitched(items, index, args, device, writer, dedupe=None, score=None):
    """``--stitch``: per zoom level, the 8-connected clusters of tiles packed whole into device calls."""

    by_zoom = {}
    for tile, path, shape in items:
        by_zoom.setdefault(tile.z, []).append((tile, path, shape))
    apron = ops.halo_apron(args.denoise, args.grow)
    for z, group in sorted(by_zoom.items()):
        shapes = sorted({shape for _, _, shape in group})
        if len(shapes) > 1:
            sys.exit("Error: --stitch needs tiles of one size per zoom level; zoom {} has {}".format(
                z, ", ".join("{}x{}".format(h, w) for h, w in shapes)))
        h, w = shape = shapes[0]
        if apron > min(h, w) or max(h, w) + 2 * apron > 4096:
            sys.exit("Error: --denoise {} + --grow {} need a border of {} pixels from the neighbouring tiles; tiles of {}x{} take at most {}"
                     .format(args.denoise, args.grow, apron, h, w, min(h, w, (4096 - max(h, w)) // 2)))
        paths = {tile: path for tile, path, _ in group}
        try:
            calls = pack_clusters(group_clusters(paths), (h + 2 * apron) * (w + 2 * apron), side=max(h, w))
        except ValueError as exc:
            sys.exit("Error: {}".format(exc))
        for tiles in tqdm(calls, desc="Features z{} {}x{}".format(z, h, w), unit="call", ascii=True):
            nbr, origin, _ = stitch_tables(tiles, shape)
            nbr, origin = torch.from_numpy(nbr).to(device), torch.from_numpy(origin).to(device)
            images = _load([paths[t] for t in tiles], device)
            iou = scores = widths = None
            if dedupe is not None or args.split or score is not None:
                # (the stages of ops.stitched_features, with the instances behind the labels, the scores and the reference behind the table)
                cleaned = ops.clean_masks_stitched(images, nbr, index, args.denoise, args.grow)
                labels = ops.stitch_labels(ops.label_components(cleaned), nbr, inplace=True)
                if args.split:
                    labels = ops.split_labels(cleaned, labels, args.split, nbr)
                table = ops.component_table_stitched(labels, origin, args.min_area)
                if score is not None:
                    table, scores = score.filter(labels, table, score.load(tiles, shape, device), stitched=True)
                if dedupe is not None:
                    table, iou = dedupe.filter(labels, table, dedupe.load(tiles, shape, device), nbr, origin)
                rows = ops.boundary_edges_stitched(labels, nbr, origin, table)
            else:
                if args.width:
                    radius = width_radius(args.max_width)
                    table, rows, d2 = ops.stitched_centerlines(images, nbr, origin, index, args.denoise, args.grow, args.min_area,
                                                               width_radius=radius)
                    widths = Widths(_sampler(d2), radius)
                else:
                    stages = ops.stitched_centerlines if args.geometry == "centerline" else ops.stitched_features
                    table, rows = stages(images, nbr, origin, index, args.denoise, args.grow, args.min_area)
            try:
                if args.geometry == "centerline":
                    writer.add(centerlines_stitched(rows.cpu().numpy(), table.cpu().numpy(), tiles, shape, args.prune, args.tolerance,
                                                    widths=widths))
                else:
                    writer.add(featurize_stitched(rows.cpu().numpy(), table.cpu().numpy(), tiles, shape, args.simplify, iou=iou,
                                                  score=scores))
            except ValueError as exc:
                sys.exit("Error: {}".format(exc))


def main(args):
    classes = load_config(args.dataset)["common"]["classes"]
    if args.type not in classes[1:]:
        sys.exit("Error: --type must be a non-background class of the dataset ({}), got '{}'".format(", ".join(classes[1:]), args.type))
    for name in ("denoise", "grow"):
        if not 0 <= getattr(args, name) <= 64:
            sys.exit("Error: --{} must be in 0..64".format(name))
    if args.prune < 0 or args.tolerance < 0:
        sys.exit("Error: --prune and --tolerance are lengths in pixels, not negative")
    if (args.dedupe is None) != (args.dedupe_threshold is None):
        sys.exit("Error: --dedupe and --dedupe_threshold come together")
    if args.dedupe is not None:
        if not 0 <= args.dedupe_threshold <= 1:  # (false for nan too)
            sys.exit("Error: --dedupe_threshold is a share of the union's pixels, 0 <= T <= 1, got {}".format(args.dedupe_threshold))
        if not os.path.isdir(args.dedupe):
            sys.exit("Error: --dedupe {} is not a directory".format(args.dedupe))
        if args.geometry == "centerline":
            sys.exit("Error: --dedupe compares areas, which says nothing about lines: not with --geometry centerline")
    if args.split:
        if not 1 <= args.split <= 64:
            sys.exit("Error: --split must be in 1..64 (0 = off)")
        if args.geometry == "centerline":
            sys.exit("Error: --split separates areas, which says nothing about lines: not with --geometry centerline")
        if args.stitch:  # (the tile sizes are in the PNG headers: no device needed to say this)
            for h, w in sorted({shape for _, _, shape in _tile_sizes(args.masks)}):
                if args.split > min(h, w):
                    sys.exit("Error: --split {} needs a border of {} pixels from the neighbouring tiles; tiles of {}x{} take at most {}"
                             .format(args.split, args.split, h, w, min(h, w)))
    if args.score is None:
        if args.score_weights is not None:
            sys.exit("Error: --score_weights {} weighs the models of --score: not without it".format(" ".join(map(str, args.score_weights))))
        if args.min_score is not None:
            sys.exit("Error: --min_score {} is a bound on the --score property: not without --score".format(args.min_score))
    else:
        for directory in args.score:
            if not os.path.isdir(directory):
                sys.exit("Error: --score {} is not a directory".format(directory))
        if len(args.score) > ops.SCORE_MAX_MODELS:
            sys.exit("Error: --score takes at most {} directories, got {}".format(ops.SCORE_MAX_MODELS, len(args.score)))
        if args.score_weights is not None:
            if len(args.score_weights) != len(args.score):
                sys.exit("Error: --score_weights has {} weights for the {} directories of --score".format(len(args.score_weights),
                                                                                                          len(args.score)))
            for weight in args.score_weights:
                if not (math.isfinite(weight) and weight >= 0):
                    sys.exit("Error: --score_weights are finite and not negative, got {}".format(weight))
            if sum(args.score_weights) <= 0:
                sys.exit("Error: --score_weights {} are all 0".format(" ".join(map(str, args.score_weights))))
        if args.min_score is not None and not 0 <= args.min_score <= 1:  # (false for nan too)
            sys.exit("Error: --min_score is a probability, 0 <= S <= 1, got {}".format(args.min_score))
        if args.geometry == "centerline":
            sys.exit("Error: --score sums over areas; lines are not scored yet: not with --geometry centerline (got --score {})".format(
                " ".join(args.score)))
    if args.width:
        if args.geometry != "centerline":
            sys.exit("Error: --width measures along centerlines: only with --geometry centerline")
        if not 1 <= args.max_width <= 252:
            sys.exit("Error: --max_width must be in 1..252")
        if args.stitch:  # (the tile sizes are in the PNG headers: no device needed to say this)
            radius = width_radius(args.max_width)
            for h, w in sorted({shape for _, _, shape in _tile_sizes(args.masks)}):
                if radius > min(h, w):
                    sys.exit("Error: --max_width {} needs a border of {} pixels from the neighbouring tiles; tiles of {}x{} take at most {}"
                             .format(args.max_width, radius, h, w, min(h, w)))
    if not torch.cuda.is_available():
        sys.exit("Error: this build computes on the MI355X only")
    device = torch.device("cuda", 0)
    index = classes.index(args.type)
    dedupe = Dedupe(args.dedupe, args.dedupe_threshold, index) if args.dedupe is not None else None
    score = Score(args.score, args.score_weights, index - 1, args.min_score) if args.score is not None else None

    by_shape = {}  # (H, W) -> [(tile, path)]: the header gives the size, a mask is decoded when its batch runs
    for tile, path, (height, width) in _tile_sizes(args.masks):
        if not (1 <= height <= 4096 and 1 <= width <= 4096):
            sys.exit("Error: {} is {}x{}; tiles are at most 4096x4096".format(path, height, width))
        by_shape.setdefault((height, width), []).append((tile, path))

    writer = FeatureWriter()
    if args.stitch:
        stitched([(tile, path, shape) for shape, items in by_shape.items() for tile, path in items], index, args, device, writer, dedupe,
                 score)
        by_shape = {}
    for shape, items in by_shape.items():  # tiles of one batch share a shape
        # (the library takes B*H*W < 2^29 per call, link_rings fewer than 1024 tiles)
        batch = max(1, min(args.batch_size, 1023, ((1 << 29) - 1) // (shape[0] * shape[1])))
        for start in tqdm(range(0, len(items), batch), desc="Features {}x{}".format(*shape), unit="batch", ascii=True):
            group = items[start:start + batch]
            images = _load([path for _, path in group], device)
            cleaned = ops.clean_masks(images, index, args.denoise, args.grow)
            labels = ops.label_components(cleaned)
            if args.split:
                labels = ops.split_labels(cleaned, labels, args.split)
            table = ops.component_table(labels, args.min_area)
            if args.geometry == "centerline":
                links = ops.skeleton_links(ops.thin_masks(cleaned), labels, table)
                widths = None
                if args.width:  # (the same cleaned mask goes to the thinning and to the transform)
                    radius = width_radius(args.max_width)
                    widths = Widths(_sampler(ops.distance_transform(cleaned, radius)), radius)
                writer.add(centerlines(links.cpu().numpy(), table.cpu().numpy(), [tile for tile, _ in group], shape, args.prune,
                                       args.tolerance, widths=widths))
                continue
            iou = scores = None
            if score is not None:
                table, scores = score.filter(labels, table, score.load([tile for tile, _ in group], shape, device))
            if dedupe is not None:
                table, iou = dedupe.filter(labels, table, dedupe.load([tile for tile, _ in group], shape, device))
            edges = ops.boundary_edges(labels, table)
            writer.add(featurize(edges.cpu().numpy(), table.cpu().numpy(), [tile for tile, _ in group], shape, args.simplify, iou=iou,
                                 score=scores))
    writer.save(args.out)
    if score is not None:
        print("Score: {} components scored, {} dropped below --min_score{}".format(
            score.scored, score.dropped, "" if args.min_score is None else " {}".format(args.min_score)), file=sys.stderr)
    if dedupe is not None:
        print("Dedupe: {} components examined, {} dropped as already mapped".format(dedupe.examined, dedupe.dropped), file=sys.stderr)
