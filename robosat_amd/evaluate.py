"""Host side of ``rs evaluate``: scores from confusion matrices, object matching from component and overlap tables, the report and
the per-tile list.  The device counts (``ops.mask_confusion``, ``ops.boundary_counts``, the ``rs features`` stages); everything here
works on those integers, as Python numbers, and divides once at the end.  Definitions: DESIGN.md, "rs evaluate"."""

import csv
import math
from fractions import Fraction

import numpy as np

from robosat_amd.metrics import Metrics


def _number(value):
    """A score as the report carries it: a float, or None where the ratio is undefined (NaN never reaches the JSON)."""

    value = float(value)
    return None if math.isnan(value) else value


def _ratio(num, den):
    return num / den if den else None


def confusion_scores(matrix, classes):
    """C x C integers ``M[actual][predicted]`` and the class names -> {"iou": {name: IoU}, "miou", "fg_iou", "mcc", "accuracy"}:
    ``robosat_amd.metrics.Metrics``'s expressions on that matrix (for two classes the reference's own), accuracy = trace / sum;
    None where a ratio is undefined (a class neither present nor predicted; an empty matrix)."""

    matrix = np.asarray(matrix, dtype=np.int64)
    metrics = Metrics.from_confusion(classes, matrix)
    total = int(matrix.sum())
    return {
        "iou": {name: _number(v) for name, v in zip(classes, metrics.get_class_ious())},
        "miou": _number(metrics.get_miou()),
        "fg_iou": _number(metrics.get_fg_iou()),
        "mcc": _number(metrics.get_mcc()),
        "accuracy": _ratio(int(np.trace(matrix)), total),
    }


def match_objects(table_p, table_g, pairs, threshold, stitched):
    """Predicted and actual objects -> (matched, predicted, actual, ious).  ``table_p`` / ``table_g``: the rows of
    ``ops.component_table`` (rows of 7: tile, label, area, ...) or with ``stitched`` of ``ops.component_table_stitched`` (rows of 6:
    label, area, ...), after ``--min_area``; ``pairs``: the rows of ``ops.overlap_table`` (raster, predicted label, actual label,
    shared pixels).  An object's key is (raster, label), raster 0 throughout with ``stitched``: without it a pair lies within one tile
    by construction.  A pair's IoU is inter / (area_p + area_g - inter); a pair with a component that is not among its table's rows (below
    ``--min_area``) is ignored.  Pairs are taken greedily by decreasing IoU, ties by the smaller predicted key, then the smaller actual
    key, and a pair matches where neither side is matched yet and IoU >= ``threshold``.  IoUs are compared as fractions of integers
    (``threshold`` by the exact value of its float), never as rounded quotients.  Above 0.5 the matching is the unique one; at exactly
    0.5 an object can reach two others and the order decides.  ``ious``: the matches' IoUs as floats, in the order they were taken."""

    width = 6 if stitched else 7
    table_p = np.asarray(table_p, dtype=np.int64).reshape(-1, width)
    table_g = np.asarray(table_g, dtype=np.int64).reshape(-1, width)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 4)
    if stitched:
        pairs = pairs.copy()
        pairs[:, 0] = 0

    def areas(table, raster, label):
        """The areas of the pairs' components in ``table`` and whether they are listed there (keys: tiles <= 65535, labels < 2^31)."""

        key = (np.zeros(len(table), dtype=np.int64) if stitched else table[:, 0]) << 31 | table[:, 0 if stitched else 1]
        order = np.argsort(key, kind="stable")
        want = raster << 31 | label
        at = np.minimum(np.searchsorted(key[order], want), max(len(key) - 1, 0))
        if len(key) == 0:
            return np.zeros(len(want), dtype=np.int64), np.zeros(len(want), dtype=bool)
        return table[:, 1 if stitched else 2][order][at], key[order][at] == want

    area_p, listed_p = areas(table_p, pairs[:, 0], pairs[:, 1])
    area_g, listed_g = areas(table_g, pairs[:, 0], pairs[:, 2])
    bound = Fraction(threshold)
    union = area_p + area_g - pairs[:, 3]
    # a float screen first (a quotient of integers below 2^31 is off by far less than the margin), then the exact comparison
    listed = listed_p & listed_g & (pairs[:, 3] / np.maximum(union, 1) >= float(threshold) - 1e-9)
    candidates = []
    for (raster, a, b, inter), u in zip(pairs[listed].tolist(), union[listed].tolist()):
        if inter * bound.denominator >= bound.numerator * u:
            candidates.append((-Fraction(inter, u), (raster, a), (raster, b)))
    candidates.sort()
    taken_p, taken_g, ious = set(), set(), []
    for iou, kp, kg in candidates:
        if kp in taken_p or kg in taken_g:
            continue
        taken_p.add(kp)
        taken_g.add(kg)
        ious.append(float(-iou))
    return len(ious), len(table_p), len(table_g), ious


class ObjectScores:
    """Matches summed over batches or calls -> the report's ``objects``."""

    def __init__(self, threshold, min_area, stitched):
        self.threshold, self.min_area, self.stitched = threshold, min_area, stitched
        self.matched = self.predicted = self.actual = 0
        self.ious = []

    def add(self, table_p, table_g, pairs):
        matched, predicted, actual, ious = match_objects(table_p, table_g, pairs, self.threshold, self.stitched)
        self.matched += matched
        self.predicted += predicted
        self.actual += actual
        self.ious.extend(ious)

    def report(self):
        return {
            "threshold": self.threshold,
            "min_area": self.min_area,
            "stitched": bool(self.stitched),
            "predicted": self.predicted,
            "actual": self.actual,
            "matched": self.matched,
            "precision": _ratio(self.matched, self.predicted),
            "recall": _ratio(self.matched, self.actual),
            "f1": _ratio(2 * self.matched, self.predicted + self.actual),
            "mean_matched_iou": _ratio(math.fsum(self.ious), len(self.ious)),
        }


def boundary_report(d, counts):
    """``d`` and the summed (predicted, actual, shared) band pixels -> the report's ``boundary``."""

    predicted, actual, shared = (int(v) for v in counts)
    return {"d": int(d), "predicted": predicted, "actual": actual, "shared": shared, "iou": _ratio(shared, predicted + actual - shared)}


CENTERLINE_COUNTS = ("straight", "diagonal", "matched_straight", "matched_diagonal")
SQRT2 = math.sqrt(2.0)


def _link_length(straight, diagonal):
    """The length in pixels of ``straight`` E / S links and ``diagonal`` SE / SW links, float64."""

    return straight + diagonal * SQRT2


def centerline_scores(counts):
    """The eight summed link counts of ``ops.centerline_counts`` -> (completeness, correctness, quality): with P and G the lengths
    of the predicted and the actual skeleton and Pm, Gm their matched parts, Gm / G, Pm / P and Pm / (P + G - Gm); None where the
    denominator is zero."""

    ps, pd, pms, pmd, gs, gd, gms, gmd = (int(v) for v in counts)
    p, pm, g, gm = _link_length(ps, pd), _link_length(pms, pmd), _link_length(gs, gd), _link_length(gms, gmd)
    return _ratio(gm, g), _ratio(pm, p), _ratio(pm, p + g - gm)


def centerline_report(rho, counts):
    """``rho`` and the eight link counts summed over all groups (``ops.centerline_counts``'s order) -> the report's ``centerline``:
    the buffer method of Wiedemann and Heipke on skeletons.  Lengths are straight + diagonal * sqrt(2) in float64, formed once from
    the integers; f1 is the harmonic mean of completeness and correctness; an undefined ratio is None."""

    counts = [int(v) for v in counts]
    if len(counts) != 8 or min(counts) < 0:
        raise ValueError("robosat_amd: eight link counts, none below zero")
    sides = {}
    for name, four in (("predicted", counts[:4]), ("actual", counts[4:])):
        side = dict(zip(CENTERLINE_COUNTS, four))
        sides[name] = {"straight": side["straight"], "diagonal": side["diagonal"], "length": _link_length(four[0], four[1]),
                       "matched_straight": side["matched_straight"], "matched_diagonal": side["matched_diagonal"],
                       "matched_length": _link_length(four[2], four[3])}
    completeness, correctness, quality = centerline_scores(counts)
    f1 = None
    if completeness is not None and correctness is not None:
        f1 = _ratio(2 * completeness * correctness, completeness + correctness)
    return {"rho": int(rho), "predicted": sides["predicted"], "actual": sides["actual"], "completeness": completeness,
            "correctness": correctness, "quality": quality, "f1": f1}


def build_report(classes, matrix, tiles, tiles_without_label, kind=None, objects=None, boundary=None, ignore=None, ignored=0,
                 probability=None, centerline=None, ignored_as=None):
    """The report of one run.  ``matrix``: C x C Python integers summed over every evaluated tile; ``kind``: ``--type`` or None;
    ``objects`` / ``boundary``: ``ObjectScores.report()`` / ``boundary_report()`` or None.  With the dataset's ``ignore`` label the
    report also carries it and ``ignored``, the pixels whose label has that value: they are in no cell, so ``pixels`` (the matrix's
    sum) counts the valid ones and ``pixels + ignored`` is every pixel of the evaluated tiles.  ``probability`` (with ``--probs``):
    ``probability_report()``, the last key.  ``centerline`` (with ``--centerline``): ``centerline_report()``, behind ``boundary``.
    ``ignored_as`` (with ``--ignored unknown``): what the ignored pixels were to the typed views, a key behind ``ignored``."""

    matrix = [[int(v) for v in row] for row in matrix]
    report = {
        "classes": list(classes),
        "tiles": int(tiles),
        "tiles_without_label": int(tiles_without_label),
        "pixels": sum(sum(row) for row in matrix),
        "confusion": matrix,
    }
    report.update(confusion_scores(matrix, classes))
    if ignore is not None:
        report["ignore"] = int(ignore)
        report["ignored"] = int(ignored)
        if ignored_as is not None:
            report["ignored_as"] = ignored_as
    if kind is not None:
        report["type"] = kind
        report["objects"] = objects
    if boundary is not None:
        report["boundary"] = boundary
    if centerline is not None:
        report["centerline"] = centerline
    if probability is not None:
        report["probability"] = probability
    return report


def tile_rows(tiles, matrices, classes, kind=None, ignored=None, brier=None, centerline=None):
    """One row per evaluated tile: ``tiles`` and their C x C matrices -> dicts with z, x, y, pixels, iou_<class> per class, miou,
    predicted_share, actual_share (the share of non-background pixels on each side), sorted worst first: by the IoU of ``kind``
    (``--type``), or by miou without it, undefined values last, then by (z, x, y).  ``ignored`` (with the dataset's ignore label):
    the tiles' counts of ignored label pixels, an ``ignored`` entry of each row; ``pixels`` and the shares are over the valid ones.
    ``brier`` (with ``--probs``): the tiles' own Brier scores (``brier_score``), a ``brier`` entry of each row; it has no say in the
    order.  ``centerline`` (with ``--centerline``, per tile): the tiles' own eight link counts; the rows gain
    ``centerline_completeness``, ``centerline_correctness`` and ``centerline_quality``, which have no say in the order either."""

    rows = []
    for i, (tile, matrix) in enumerate(zip(tiles, matrices)):
        matrix = np.asarray(matrix, dtype=np.int64)
        scores = confusion_scores(matrix, classes)
        total = int(matrix.sum())
        row = {"z": int(tile.z), "x": int(tile.x), "y": int(tile.y), "pixels": total}
        if ignored is not None:
            row["ignored"] = int(ignored[i])
        for name in classes:
            row["iou_" + name] = scores["iou"][name]
        row["miou"] = scores["miou"]
        row["predicted_share"] = _ratio(total - int(matrix[:, 0].sum()), total)
        row["actual_share"] = _ratio(total - int(matrix[0, :].sum()), total)
        if brier is not None:
            row["brier"] = brier[i]
        if centerline is not None:
            for name, value in zip(CENTERLINE_COLUMNS, centerline_scores(centerline[i])):
                row[name] = value
        rows.append(row)
    column = "miou" if kind is None else "iou_" + kind
    rows.sort(key=lambda r: (r[column] is None, r[column] if r[column] is not None else 0.0, r["z"], r["x"], r["y"]))
    return rows


CENTERLINE_COLUMNS = ["centerline_completeness", "centerline_correctness", "centerline_quality"]


def tile_columns(classes, ignored=False, brier=False, centerline=False):
    return (["z", "x", "y", "pixels"] + (["ignored"] if ignored else []) + ["iou_" + name for name in classes]
            + ["miou", "predicted_share", "actual_share"] + (["brier"] if brier else []) + (CENTERLINE_COLUMNS if centerline else []))


def write_tile_rows(path, rows, classes, ignored=False, brier=False, centerline=False):
    """``tile_rows`` as CSV; an undefined value is an empty field, a float is written with ``repr`` (it reads back as it was).
    ``ignored`` / ``brier`` / ``centerline``: the rows carry those columns (``tile_rows`` was given the values)."""

    with open(path, "w", newline="") as fp:
        writer = csv.writer(fp)
        columns = tile_columns(classes, ignored, brier, centerline)
        writer.writerow(columns)
        for row in rows:
            writer.writerow(["" if row[c] is None else repr(row[c]) for c in columns])


# ---- rs evaluate --probs: scores of the probability bytes of one class ("rs evaluate --probs") ----------------------
CALIBRATION_BINS = 10
ANCHORS = np.linspace(0, 1, 256)  # a byte's probability: what ``rs masks`` and ``rs features --score`` un-quantise it to

POINT_COLUMNS = ["threshold_byte", "threshold", "tp", "fp", "fn", "tn", "precision", "recall", "f1", "iou"]


def _fraction(num, den):
    return Fraction(num, den) if den else None


def _float(value):
    return None if value is None else float(value)


def _histograms(pos, neg):
    pos, neg = [int(v) for v in pos], [int(v) for v in neg]
    if len(pos) != 256 or len(neg) != 256 or min(pos + neg) < 0:
        raise ValueError("robosat_amd: 256 counts of positives and 256 of negatives, none below zero")
    return pos, neg


def _points(pos, neg):
    """The 256 operating points "predict the class where byte >= k" as (k, tp, fp, fn, tn)."""

    p, n = sum(pos), sum(neg)
    points, tp, fp = [None] * 256, 0, 0
    for k in range(255, -1, -1):
        tp += pos[k]
        fp += neg[k]
        points[k] = (k, tp, fp, p - tp, n - fp)
    return points


def _point_scores(point):
    """(precision, recall, F1, IoU) of an operating point as fractions, None where undefined."""

    _, tp, fp, fn, _ = point
    return _fraction(tp, tp + fp), _fraction(tp, tp + fn), _fraction(2 * tp, 2 * tp + fp + fn), _fraction(tp, tp + fp + fn)


def _point_row(point):
    k, tp, fp, fn, tn = point
    precision, recall, f1, iou = _point_scores(point)
    return {"threshold_byte": k, "threshold": float(ANCHORS[k]), "tp": tp, "fp": fp, "fn": fn, "tn": tn,
            "precision": _float(precision), "recall": _float(recall), "f1": _float(f1), "iou": _float(iou)}


def _best(points, which):
    """The point with the highest exact score (2: F1, 3: IoU), the smallest k among equals; None where no point has one."""

    best, best_score = None, None
    for point in points:
        score = _point_scores(point)[which]
        if score is not None and (best_score is None or score > best_score):
            best, best_score = point, score
    return best


def curve_rows(pos, neg):
    """The 256 operating points, k = 0 .. 255: dicts of ``POINT_COLUMNS``."""

    return [_point_row(point) for point in _points(*_histograms(pos, neg))]


def write_curve_rows(path, rows):
    """``curve_rows`` as CSV; an undefined value is an empty field, a float is written with ``repr``, like ``write_tile_rows``."""

    with open(path, "w", newline="") as fp:
        writer = csv.writer(fp)
        writer.writerow(POINT_COLUMNS)
        for row in rows:
            writer.writerow(["" if row[c] is None else repr(row[c]) for c in POINT_COLUMNS])


def brier_score(pos, neg):
    """sum_q (pos[q] (255 - q)^2 + neg[q] q^2) / (255^2 (P + N)) as a float, None for no pixels."""

    pos, neg = _histograms(pos, neg)
    total = sum(pos) + sum(neg)
    return _float(_fraction(sum(pos[q] * (255 - q) ** 2 + neg[q] * q * q for q in range(256)), 255 * 255 * total))


def probability_scores(pos, neg):
    """``pos[q]`` / ``neg[q]``: the pixels with probability byte q whose label is / is not the class, 256 integers each, summed
    over the tiles -> the report's ``probability`` scores: ap, auc, brier, ece, calibration, best_f1, best_iou, at_half.  Every
    score is an exact fraction of integers turned into a float once; an undefined one is None."""

    pos, neg = _histograms(pos, neg)
    p, n = sum(pos), sum(neg)
    total = p + n
    points = _points(pos, neg)

    ap = None
    if p:
        ap, above = Fraction(0), 0  # above: TP_{k+1}
        for k, tp, fp, _, _ in reversed(points):
            if tp != above:  # (a step of recall; tp > 0 here, so the precision is defined)
                ap += Fraction(tp - above, p) * Fraction(tp, tp + fp)
            above = tp
    auc = None
    if p and n:
        below, wins = 0, 0  # below: N_{<q}; wins: twice the pairs won, ties counting half
        for q in range(256):
            wins += pos[q] * (2 * below + neg[q])
            below += neg[q]
        auc = Fraction(wins, 2 * p * n)

    bins = []
    ece = Fraction(0) if total else None
    for b in range(CALIBRATION_BINS):
        members = [q for q in range(256) if min(CALIBRATION_BINS * q // 255, CALIBRATION_BINS - 1) == b]
        pixels = sum(pos[q] + neg[q] for q in members)
        confidence = _fraction(sum(q * (pos[q] + neg[q]) for q in members), 255 * pixels)
        accuracy = _fraction(sum(pos[q] for q in members), pixels)
        if pixels:
            ece += Fraction(pixels, total) * abs(accuracy - confidence)
        bins.append({"lo": float(ANCHORS[members[0]]), "hi": float(ANCHORS[members[-1]]), "pixels": pixels,
                     "confidence": _float(confidence), "accuracy": _float(accuracy)})

    best_f1, best_iou = _best(points, 2), _best(points, 3)
    return {
        "ap": _float(ap),
        "auc": _float(auc),
        "brier": brier_score(pos, neg),
        "ece": _float(ece),
        "calibration": bins,
        "best_f1": None if best_f1 is None else _point_row(best_f1),
        "best_iou": None if best_iou is None else _point_row(best_iou),
        "at_half": _point_row(points[128]),
    }


def probability_report(kind, pos, neg, ignored=None):
    """The report's ``probability``: the class, ``pixels`` (those with a label that is a class), ``positives``, with the dataset's
    ignore label ``ignored``, and ``probability_scores``."""

    pos, neg = _histograms(pos, neg)
    report = {"class": kind, "pixels": sum(pos) + sum(neg), "positives": sum(pos)}
    if ignored is not None:
        report["ignored"] = int(ignored)
    report.update(probability_scores(pos, neg))
    return report
