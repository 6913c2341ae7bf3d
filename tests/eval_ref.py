"""Restatement in numpy of what ``rs evaluate`` counts (include/robosat_hip.h): the confusion matrix per group, the
boundary band of a mask, and object matching by brute force over label rasters.  Not a test module; ``test_evaluate_cpu.py`` pins the
band against ``edt_ref.edt_brute`` and the host's ``match_objects`` against ``match`` here."""

from fractions import Fraction

import numpy as np

import edt_ref as E


def confusion(predicted, actual, classes, stitched=False):
    """uint8 [B, H, W] twice -> (int64 [G, C, C] with [g][actual][predicted], int64 [G] of the pixels with a value >= C, which are in
    no cell); G = B, or 1 with ``stitched``."""

    predicted, actual = np.asarray(predicted), np.asarray(actual)
    groups = 1 if stitched else predicted.shape[0]
    p, a = predicted.reshape(groups, -1).astype(np.int64), actual.reshape(groups, -1).astype(np.int64)
    counts = np.zeros((groups, classes, classes), dtype=np.int64)
    bad = np.zeros(groups, dtype=np.int64)
    for g in range(groups):
        wrong = (p[g] >= classes) | (a[g] >= classes)
        bad[g] = wrong.sum()
        counts[g] = np.bincount(a[g][~wrong] * classes + p[g][~wrong], minlength=classes * classes).reshape(classes, classes)
    return counts, bad


def band(mask, d, coded=False):
    """bool [H, W]: the set pixels within ``d`` pixels, centre to centre, of an unset pixel of the raster: 1 <= d2 <= d*d in the
    transform capped at d + 1."""

    d2 = E.edt(mask, d + 1, coded=coded)
    return (d2 >= 1) & (d2 <= d * d)


def band_stitched(grid, d):
    """bool [T, H, W]: ``band`` of the canvas the grid's tiles form (unknown where no tile is), cut back into the tiles."""

    d2 = E.edt_stitched(grid, d + 1)
    return (d2 >= 1) & (d2 <= d * d)


def boundary(band_a, band_b, stitched=False):
    """bool [B, H, W] twice -> int64 [G, 3]: (|A|, |B|, |A and B|) per group."""

    groups = 1 if stitched else band_a.shape[0]
    a, b = np.asarray(band_a).reshape(groups, -1), np.asarray(band_b).reshape(groups, -1)
    return np.stack([a.sum(axis=1), b.sum(axis=1), (a & b).sum(axis=1)], axis=1).astype(np.int64)


def overlap_rows(labels_p, labels_g):
    """Label rasters [B, H, W] twice -> sorted rows (raster, label_p, label_g, shared pixels), one per pair that shares a pixel."""

    rows = []
    for raster, (p, g) in enumerate(zip(labels_p, labels_g)):
        both = (p != 0) & (g != 0)
        pairs, counts = np.unique(np.stack([p[both], g[both]], axis=1).reshape(-1, 2), axis=0, return_counts=True)
        rows += [(raster, int(a), int(b), int(n)) for (a, b), n in zip(pairs, counts)]
    return np.array(sorted(rows), dtype=np.int64).reshape(-1, 4)


def match(labels_p, labels_g, threshold, min_area=0):
    """Brute force over label rasters [B, H, W] (0 = background), every raster on its own: objects = the labels with at least
    ``min_area`` pixels; the IoU of EVERY pair of a raster as a fraction; pairs in the order (IoU descending, predicted (raster, label),
    actual (raster, label)); a pair matches where both are free and IoU >= threshold (the float's exact value).
    -> (matched, predicted, actual, [IoU fractions of the matches in that order])."""

    bound = Fraction(threshold)
    pairs, predicted, actual = [], 0, 0
    for raster, (p, g) in enumerate(zip(labels_p, labels_g)):
        objects_p = [(int(v), p == v) for v in np.unique(p[p != 0]) if (p == v).sum() >= min_area]
        objects_g = [(int(v), g == v) for v in np.unique(g[g != 0]) if (g == v).sum() >= min_area]
        predicted += len(objects_p)
        actual += len(objects_g)
        for a, mask_a in objects_p:
            for b, mask_b in objects_g:
                iou = Fraction(int((mask_a & mask_b).sum()), int((mask_a | mask_b).sum()))
                pairs.append((-iou, (raster, a), (raster, b)))
    pairs.sort()
    used_p, used_g, ious = set(), set(), []
    for iou, kp, kg in pairs:
        if -iou >= bound and -iou > 0 and kp not in used_p and kg not in used_g:
            used_p.add(kp)
            used_g.add(kg)
            ious.append(-iou)
    return len(ious), predicted, actual, ious
