"""``rs evaluate``: how good a directory of class-index masks (what ``rs masks`` writes) is against a directory of labels.  Three
views, all counted on the MI355X (``csrc/evaluate.hip`` and the ``rs features`` raster stages) and divided once on the host
(``robosat_amd/evaluate.py``):

  * pixels: the confusion matrix ``M[actual][predicted]`` per tile (``ops.mask_confusion``), summed over the tiles; per-class IoU,
    mIoU, the IoU of class 1, MCC (``robosat_amd.metrics.Metrics``'s expressions) and accuracy.  ``--tiles`` lists the tiles worst
    first: the list hard negatives are mined from (the reference's ``rs compare --minimum/--maximum``).
  * outlines (``--type --boundary D``): the Boundary IoU of Cheng et al. 2021 at D pixels, from capped distance transforms of both
    sides.  The raster's edge is no boundary here (the paper's code pads with zeros): nothing is known beyond it.
  * objects (``--type``): both sides labelled as they are, the pixels every pair of objects shares tabulated, pairs matched greedily
    by IoU at ``--match``; predicted, actual, matched, precision, recall, F1.  Per tile an object cut by a tile border counts once per
    tile; ``--stitch`` evaluates the one sparse raster the tiles of a zoom level form, where it is one object on both sides.

With ``--type --centerline RHO`` a view for roads is added, the buffer method of Wiedemann and Heipke (1998) on rasters: both
class masks are thinned to skeletons (``ops.thin_masks``), the skeletons' links are counted as straight and diagonal ones, and a
link is matched where both of its end pixels lie within RHO pixels of the other side's skeleton (``ops.centerline_counts``).
Correctness is the matched share of the predicted length, completeness that of the actual length, quality matched predicted
length / (predicted + unmatched actual length).  Pixel and boundary IoU depend on a road's width; these do not.

With the dataset's ``[common] ignore`` a pixel whose LABEL has that value is in no cell of the pixel view: the report and the
``--tiles`` rows count it as ``ignored`` and their ``pixels`` are the valid ones.  A mask byte, or another label byte, that is no
class still ends the run.  With ``--type`` a label tile that holds an ignored pixel ends the run, naming the tile, unless
``--ignored unknown`` is given.  Then an ignored pixel is to the typed views what a pixel outside the raster already is, unknown:
the prediction under it is no part of the predicted class, no distance comes from it and it is in no boundary band (the edge of an
ignored region is no boundary), an object that an ignored region cuts is cut on both sides alike (as at a tile border without
``--stitch``), a predicted object wholly inside one does not exist, and centre lines stop short of it on both sides.  The masks and
the coded rasters of both sides come from one pass (``ops.select_known``), and the band count leaves the unknown pixels out.

With ``--probs DIR`` (the probability tiles ``rs predict`` wrote for these masks, one model) a fourth view is added: the joint
histogram of (label is the class, probability byte) per tile (``ops.prob_histogram``), summed over the tiles, from which the host
forms the 256 operating points "byte >= k", average precision, AUC, the Brier score, a ten-bin calibration table with its ECE, and
the thresholds with the best F1 and IoU (``--curve`` lists every point; ``rs masks --threshold`` applies one).  The class is
``--type`` where given, class 1 otherwise.  The histogram leaves ignored labels out by itself, so on a multi-class dataset with
ignored pixels ``--type --ignored unknown`` is what gives the probability view.

The definitions are in ``include/robosat_hip.h`` and DESIGN.md."""

import argparse
import json
import os
import sys

import numpy as np
import torch
from PIL import Image
from tqdm import tqdm

from robosat_amd import ops
from robosat_amd.config import ignore_label, load_config
from robosat_amd.evaluate import (ObjectScores, boundary_report, brier_score, build_report, centerline_report, curve_rows,
                                  probability_report, tile_rows, write_curve_rows, write_tile_rows)
from robosat_amd.features import group_clusters, pack_clusters, stitch_tables
from robosat_amd.tiles import tiles_from_slippy_map
from robosat_amd.tools.features import _load, _tile_sizes
from robosat_amd.tools.masks import load_quantized


def add_parser(subparser):
    parser = subparser.add_parser(
        "evaluate",
        help="scores segmentation masks against labels: pixels, boundaries and objects",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter,
    )
    parser.add_argument("masks", type=str, help="slippy map directory with segmentation masks (class-index PNGs); its tiles are the set")
    parser.add_argument("labels", type=str, help="slippy map directory with the labels; a mask tile without a label is skipped and counted")
    parser.add_argument("--dataset", type=str, required=True, help="path to dataset configuration file")
    parser.add_argument("out", type=str, help="path to the JSON report")
    parser.add_argument("--type", type=str, default=None, help="class of the dataset to score boundaries and objects for, and to sort --tiles by")
    parser.add_argument("--boundary", type=int, default=0, metavar="D",
                        help="with --type: boundary IoU at D pixels, 0 = off, else 1..127: of each side the pixels of the class within D "
                        "pixels of a pixel that is not, shared / (predicted + actual - shared). The edge of the raster is not a "
                        "boundary (nothing is known beyond it; the paper's code pads with zeros), nor with --stitch a seam between two "
                        "tiles. With --stitch D + 1 pixels must fit the tile's smaller side")
    parser.add_argument("--centerline", type=int, default=0, metavar="RHO",
                        help="with --type: completeness, correctness and quality of the class's centre lines (Wiedemann and Heipke's "
                        "buffer method), 0 = off, else 1..127: both sides are thinned to skeletons, and a piece of one is matched "
                        "where it lies within RHO pixels of the other. Roads want --stitch: per tile a skeleton stops about half a "
                        "road's width short of every tile border, on both sides alike, and a line just beyond the tile edge is unknown "
                        "and matches nothing. With --stitch RHO + 1 pixels must fit the tile's smaller side, and --tiles gets no "
                        "centerline columns")
    parser.add_argument("--match", type=float, default=None, metavar="T",
                        help="with --type: a predicted and an actual object match where their IoU is at least T, 0 < T <= 1 (0.5 where "
                        "not given); pairs are taken greedily, best IoU first")
    parser.add_argument("--min_area", type=int, default=None, metavar="N",
                        help="with --type: objects with fewer pixels are left out on both sides (0 where not given)")
    parser.add_argument("--stitch", action="store_true",
                        help="with --type: objects and boundaries of the one raster the tiles of a zoom level form. Without it objects are "
                        "per tile: an object cut by a tile border counts once per tile, on both sides")
    parser.add_argument("--tiles", type=str, default=None, metavar="CSV",
                        help="path to a CSV with one row per evaluated tile: z, x, y, pixels, the IoU of every class, miou and the share "
                        "of non-background pixels on each side, sorted worst first by the IoU of --type (by miou without it); with the "
                        "dataset's [common] ignore also the tile's ignored label pixels, and pixels are the others")
    parser.add_argument("--probs", type=str, default=None, metavar="DIR",
                        help="slippy map directory with the probabilities rs predict wrote for these masks (one model): adds "
                        "'probability' to the report: the 256 thresholds 'byte >= k' of the class's probability against the labels, "
                        "average precision, AUC, Brier score, calibration and the thresholds with the best F1 and IoU. The class is "
                        "--type where given, else class 1; a dataset with more than two classes needs --type. As --type refuses label "
                        "tiles with ignored pixels by default, a multi-class dataset with ignored pixels has no probability view yet "
                        "unless --ignored unknown is given. With --tiles the rows gain the tile's own Brier score")
    parser.add_argument("--curve", type=str, default=None, metavar="CSV",
                        help="with --probs: path to a CSV with the 256 operating points: threshold_byte, threshold, tp, fp, fn, tn, "
                        "precision, recall, f1, iou")
    parser.add_argument("--ignored", type=str, default="refuse", choices=["refuse", "unknown"],
                        help="with --type on a dataset with [common] ignore: what a label tile with ignored pixels means to the "
                        "boundary, object, centerline and probability views. refuse: the run ends and names the tile. unknown: an "
                        "ignored pixel is unknown on both sides, like a pixel outside the raster: it is in no band and no object, no "
                        "distance comes from it, and objects and centre lines are cut at ignored regions, on both sides alike")
    parser.add_argument("--batch_size", type=int, default=16, help="tiles per device launch")
    parser.set_defaults(func=main)


MATCH_DEFAULT = 0.5


def validate(args, classes, ignore=None):
    """Every check that needs no device; ends the run with a message.  ``ignore``: the dataset's ignore label or None.  Returns
    (match threshold, min_area)."""

    ignored = getattr(args, "ignored", "refuse")
    if ignored not in ("refuse", "unknown"):
        sys.exit("Error: --ignored is refuse or unknown, got '{}'".format(ignored))
    if ignored == "unknown" and args.type is None:
        sys.exit("Error: --ignored unknown says what ignored pixels are to the views of one class: not without --type")
    if ignored == "unknown" and ignore is None:
        sys.exit("Error: --ignored unknown needs the dataset's [common] ignore: without it no label pixel is ignored")
    if not 2 <= len(classes) <= ops.EVAL_MAX_CLASSES:
        sys.exit("Error: 2 to {} classes are counted, the dataset has {}".format(ops.EVAL_MAX_CLASSES, len(classes)))
    if args.type is None:
        for given, flag in ((args.boundary != 0, "--boundary"), (args.centerline != 0, "--centerline"), (args.match is not None, "--match"), (args.min_area is not None, "--min_area"),
                            (args.stitch, "--stitch")):
            if given:
                sys.exit("Error: {} scores the boundaries or objects of one class: not without --type".format(flag))
    elif args.type not in classes[1:]:
        sys.exit("Error: --type must be a non-background class of the dataset ({}), got '{}'".format(", ".join(classes[1:]), args.type))
    if not 0 <= args.boundary <= ops.EVAL_MAX_DISTANCE:
        sys.exit("Error: --boundary must be in 1..{} (0 = off), got {}".format(ops.EVAL_MAX_DISTANCE, args.boundary))
    if not 0 <= args.centerline <= ops.EVAL_MAX_RHO:
        sys.exit("Error: --centerline must be in 1..{} (0 = off), got {}".format(ops.EVAL_MAX_RHO, args.centerline))
    match = MATCH_DEFAULT if args.match is None else args.match
    if not 0 < match <= 1:  # (false for nan too)
        sys.exit("Error: --match is an intersection over union, 0 < T <= 1, got {}".format(match))
    min_area = 0 if args.min_area is None else args.min_area
    if min_area < 0:
        sys.exit("Error: --min_area is a number of pixels, not negative, got {}".format(min_area))
    if args.batch_size < 1:
        sys.exit("Error: --batch_size is at least 1, got {}".format(args.batch_size))
    for name in ("masks", "labels"):
        if not os.path.isdir(getattr(args, name)):
            sys.exit("Error: {} is not a directory".format(getattr(args, name)))
    if args.probs is None:
        if args.curve is not None:
            sys.exit("Error: --curve lists the operating points of the probabilities: not without --probs")
    else:
        if not os.path.isdir(args.probs):
            sys.exit("Error: {} is not a directory".format(args.probs))
        if len(classes) > 2 and args.type is None:
            sys.exit("Error: --probs scores the probabilities of one class; the dataset has {} classes: give --type ({})".format(
                len(classes), ", ".join(classes[1:])))
    if args.stitch and args.boundary:  # (the tile sizes are in the PNG headers: no device needed to say this)
        for h, w in sorted({shape for _, _, shape in _tile_sizes(args.masks)}):
            if args.boundary + 1 > min(h, w):
                sys.exit("Error: --boundary {} needs a border of {} pixels from the neighbouring tiles; tiles of {}x{} take at most {}"
                         .format(args.boundary, args.boundary + 1, h, w, min(h, w) - 1))
    if args.stitch and args.centerline:
        for h, w in sorted({shape for _, _, shape in _tile_sizes(args.masks)}):
            if args.centerline + 1 > min(h, w):
                sys.exit("Error: --centerline {} needs a border of {} pixels from the neighbouring tiles; tiles of {}x{} take at most {}"
                         .format(args.centerline, args.centerline + 1, h, w, min(h, w) - 1))
    return match, min_area


def _name(tile):
    return "{}/{}/{}".format(tile.z, tile.x, tile.y)


class Probabilities:
    """``--probs``: the probability tiles of one model, the plane of one class (``channel`` = class index - 1), and the sums of
    the histograms."""

    def __init__(self, directory, channel, per_tile=False):
        self.directory, self.channel = directory, channel
        self.paths = {tile: path for tile, path in tiles_from_slippy_map(directory)}
        self.pos, self.neg = [0] * 256, [0] * 256  # Python integers: no bound on the pixels of a run
        self.ignored = 0
        self.brier = [] if per_tile else None  # (the tiles' own Brier scores: for --tiles alone)

    def load(self, tiles, shape, device):
        """uint8 [T, H, W]: the bytes of the class, the tiles in order (as ``tools/features.py``'s ``Score.load`` reads them)."""

        planes = []
        for tile in tiles:
            path = self.paths.get(tile)
            if path is None:
                sys.exit("Error: --probs {} has no probabilities for the mask tile {}".format(self.directory, _name(tile)))
            q = load_quantized(path)
            if q.shape[:2] != tuple(shape):
                sys.exit("Error: {} is {}x{}; the mask tile {} is {}x{}".format(path, q.shape[0], q.shape[1], _name(tile), shape[0], shape[1]))
            if self.channel >= q.shape[2]:
                sys.exit("Error: {} (tile {}) holds the probabilities of {} classes; the class to score is class {} of the dataset".format(
                    path, _name(tile), q.shape[2] + 1, self.channel + 1))
            planes.append(np.ascontiguousarray(q[:, :, self.channel], dtype=np.uint8))
        return torch.from_numpy(np.stack(planes)).to(device)

    def add(self, hist, ignored):
        """``ops.prob_histogram``'s [T, 2, 256] and its [T] ignored pixels: summed over the tiles on the device, and with
        ``per_tile`` every tile's own Brier score kept."""

        neg, pos = hist.sum(dim=0).tolist()
        for q in range(256):
            self.pos[q] += pos[q]
            self.neg[q] += neg[q]
        self.ignored += int(ignored.sum())
        if self.brier is not None:
            self.brier.extend(brier_score(tile_pos, tile_neg) for tile_neg, tile_pos in hist.tolist())


class Evaluation:
    """The sums of a run, and the device stages of one batch (tiles on their own) or call (tiles as one sparse raster)."""

    def __init__(self, classes, index, boundary, objects, ignore=None, probs=None, centerline=0, unknown=False):
        self.classes, self.index, self.boundary, self.objects, self.ignore, self.probs = classes, index, boundary, objects, ignore, probs
        self.centerline = centerline
        self.unknown = unknown  # --ignored unknown: ignored label pixels are unknown to the typed views instead of ending the run
        self.links = [0] * 8   # the eight link counts of --centerline, summed
        self.tile_links = []   # and per tile, for --tiles (stays empty for stitched calls: they have no per-tile counts)
        n = len(classes)
        self.matrix = [[0] * n for _ in range(n)]  # Python integers: no bound on the pixels of a run
        self.band = [0, 0, 0]
        self.tiles, self.matrices, self.ignored = [], [], []

    def add(self, tiles, paths, label_paths, shape, device, nbr=None, origin=None):
        predicted = _load([paths[t] for t in tiles], device)
        label_files = []
        for tile in tiles:
            with Image.open(label_paths[tile]) as image:
                if (image.size[1], image.size[0]) != tuple(shape):
                    sys.exit("Error: the label {} of tile {} is {}x{}; its mask is {}x{}".format(label_paths[tile], _name(tile), image.size[1],
                                                                                              image.size[0], shape[0], shape[1]))
            label_files.append(label_paths[tile])
        actual = _load(label_files, device)
        if self.ignore is None:
            counts, bad = ops.mask_confusion(predicted, actual, len(self.classes))
        else:
            counts, bad, ignored = ops.mask_confusion(predicted, actual, len(self.classes), ignore=self.ignore)
            ignored = ignored.tolist()
            for tile, n in zip(tiles, ignored):
                if n and self.index is not None and not self.unknown:
                    sys.exit("Error: the label of tile {} has {} pixels of the ignore value {}; --type scores boundaries and objects, "
                             "which are not defined next to ignored pixels yet: evaluate without --type, or with --ignored unknown to "
                             "take them as unknown on both sides".format(_name(tile), n, self.ignore))
            self.ignored.extend(ignored)
        for tile, wrong in zip(tiles, bad.tolist()):
            if wrong:
                sys.exit("Error: tile {} has {} pixels whose value, in the mask or the label, is none of the dataset's {} classes".format(
                    _name(tile), wrong, len(self.classes)))
        for tile, matrix in zip(tiles, counts.tolist()):
            self.tiles.append(tile)
            self.matrices.append(matrix)
            for a, row in enumerate(matrix):
                for p, v in enumerate(row):
                    self.matrix[a][p] += v
        if self.probs is not None:  # (a pixel view: per tile with or without --stitch)
            hist, wrong, unknown = ops.prob_histogram(self.probs.load(tiles, shape, device), actual, len(self.classes),
                                                      self.probs.channel + 1, ignore=self.ignore)
            # the histogram's own counts of bad and ignored labels.  A bad byte, in the mask or the label, ended the run above, so no
            # label is bad here and the ignored labels are the ones the confusion call counted (it counts them over a mask byte that
            # is a class only): the probability view's pixels + ignored are the report's.
            assert not wrong.any().item() and (self.ignore is None or unknown.tolist() == ignored), "the two counting calls disagree"
            self.probs.add(hist, unknown)
        if self.index is None:
            return
        stitched = nbr is not None
        if self.unknown:
            # the same calls whether this batch holds an ignored pixel or not: the coded planes then hold no 2 and every count is
            # the unflagged one
            coded_p, coded_g, mask_p, mask_g = ops.select_known(predicted, actual, self.index, self.ignore, len(self.classes))
        else:
            # (discs of 0: the class's pixels as they are, on both sides)
            mask_p, mask_g = ops.clean_masks(predicted, self.index, 0, 0), ops.clean_masks(actual, self.index, 0, 0)
            coded_p, coded_g = mask_p, mask_g
        if self.boundary:
            # (of the coded planes: non-zero = set, so distances pass over unknown pixels and come from unset ones only)
            d2_p = ops.distance_transform(coded_p, self.boundary + 1, nbr)
            d2_g = ops.distance_transform(coded_g, self.boundary + 1, nbr)
            for row in ops.boundary_counts(d2_p, d2_g, self.boundary, stitched=stitched, coded=coded_g if self.unknown else None).tolist():
                for k in range(3):
                    self.band[k] += row[k]
        if self.centerline:
            counts = ops.centerline_counts(ops.thin_masks(mask_p, nbr), ops.thin_masks(mask_g, nbr), self.centerline, nbr).tolist()
            for row in counts:
                for k in range(8):
                    self.links[k] += row[k]
            if not stitched:
                self.tile_links.extend(counts)
        labels_p, labels_g = ops.label_components(mask_p), ops.label_components(mask_g)
        if stitched:
            labels_p, labels_g = ops.stitch_labels(labels_p, nbr, inplace=True), ops.stitch_labels(labels_g, nbr, inplace=True)
            table_p = ops.component_table_stitched(labels_p, origin, self.objects.min_area)
            table_g = ops.component_table_stitched(labels_g, origin, self.objects.min_area)
        else:
            table_p, table_g = ops.component_table(labels_p, self.objects.min_area), ops.component_table(labels_g, self.objects.min_area)
        pairs = ops.overlap_table(labels_p, labels_g, stitched=stitched)
        self.objects.add(table_p.cpu().numpy(), table_g.cpu().numpy(), pairs.cpu().numpy())


def main(args):
    # (callers that build the arguments themselves may predate these flags)
    args.probs, args.curve = getattr(args, "probs", None), getattr(args, "curve", None)
    args.centerline = getattr(args, "centerline", 0)
    args.ignored = getattr(args, "ignored", "refuse")
    dataset = load_config(args.dataset)
    classes = dataset["common"]["classes"]
    try:
        ignore = ignore_label(dataset)
    except ValueError as err:
        sys.exit("Error: {}".format(err))
    match, min_area = validate(args, classes, ignore)
    if not torch.cuda.is_available():
        sys.exit("Error: this build computes on the MI355X only")
    device = torch.device("cuda", 0)
    index = None if args.type is None else classes.index(args.type)
    objects = None if index is None else ObjectScores(match, min_area, args.stitch)
    probs = None if args.probs is None else Probabilities(args.probs, (1 if index is None else index) - 1, per_tile=args.tiles is not None)
    run = Evaluation(classes, index, args.boundary, objects, ignore, probs, args.centerline, unknown=args.ignored == "unknown")

    label_paths = {tile: path for tile, path in tiles_from_slippy_map(args.labels)}
    without_label = 0
    by_shape = {}  # (H, W) -> [tile]: the header gives the size, a tile is decoded when its batch runs
    paths = {}
    for tile, path, (height, width) in _tile_sizes(args.masks):
        if tile not in label_paths:
            without_label += 1
            continue
        if not (1 <= height <= 4096 and 1 <= width <= 4096):
            sys.exit("Error: {} is {}x{}; tiles are at most 4096x4096".format(path, height, width))
        paths[tile] = path
        by_shape.setdefault((height, width), []).append(tile)

    if args.stitch:
        by_zoom = {}
        for shape, tiles in by_shape.items():
            for tile in tiles:
                by_zoom.setdefault(tile.z, []).append((tile, shape))
        for z, group in sorted(by_zoom.items()):
            shapes = sorted({shape for _, shape in group})
            if len(shapes) > 1:
                sys.exit("Error: --stitch needs tiles of one size per zoom level; zoom {} has {}".format(
                    z, ", ".join("{}x{}".format(h, w) for h, w in shapes)))
            h, w = shape = shapes[0]
            try:
                calls = pack_clusters(group_clusters([tile for tile, _ in group]), h * w, side=max(h, w))
            except ValueError as exc:
                sys.exit("Error: {}".format(exc))
            for tiles in tqdm(calls, desc="Evaluate z{} {}x{}".format(z, h, w), unit="call", ascii=True):
                nbr, origin, _ = stitch_tables(tiles, shape)
                run.add(tiles, paths, label_paths, shape, device, torch.from_numpy(nbr).to(device), torch.from_numpy(origin).to(device))
        by_shape = {}
    for shape, tiles in by_shape.items():  # tiles of one batch share a shape
        batch = max(1, min(args.batch_size, 65535, ((1 << 29) - 1) // (shape[0] * shape[1])))
        for start in tqdm(range(0, len(tiles), batch), desc="Evaluate {}x{}".format(*shape), unit="batch", ascii=True):
            run.add(tiles[start:start + batch], paths, label_paths, shape, device)

    report = build_report(classes, run.matrix, len(run.tiles), without_label, kind=args.type,
                          objects=None if objects is None else objects.report(),
                          boundary=boundary_report(args.boundary, run.band) if args.boundary else None,
                          centerline=centerline_report(args.centerline, run.links) if args.centerline else None,
                          **({} if ignore is None else {"ignore": ignore, "ignored": sum(run.ignored)}),
                          **({"ignored_as": "unknown"} if run.unknown else {}),
                          **({} if probs is None else {"probability": probability_report(
                              classes[probs.channel + 1], probs.pos, probs.neg, None if ignore is None else probs.ignored)}))
    with open(args.out, "w") as fp:
        json.dump(report, fp, indent=2, allow_nan=False)
        fp.write("\n")
    if args.curve is not None:
        write_curve_rows(args.curve, curve_rows(probs.pos, probs.neg))
    if args.tiles is not None:
        extra = {} if probs is None else {"brier": probs.brier}
        columns = {"brier": probs is not None}
        if args.centerline and not args.stitch:
            extra["centerline"] = run.tile_links
            columns["centerline"] = True
        if ignore is None:
            write_tile_rows(args.tiles, tile_rows(run.tiles, run.matrices, classes, kind=args.type, **extra), classes, **columns)
        else:
            write_tile_rows(args.tiles, tile_rows(run.tiles, run.matrices, classes, kind=args.type, ignored=run.ignored, **extra), classes,
                            ignored=True, **columns)
    if without_label:
        print("Evaluate: {} mask tiles without a label were skipped".format(without_label), file=sys.stderr)
