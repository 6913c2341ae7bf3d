"""``rs evaluate --probs`` restated on the raw pixels, in numpy and ``Fraction``: the histogram by ``np.bincount``, the operating
points by comparing the bytes with k, AUC over every (positive, negative) pair, average precision by sorting, calibration and the
Brier score pixel by pixel.  Nothing here is shared with ``robosat_amd/evaluate.py``; nothing goes through a histogram except the
histogram itself."""

from fractions import Fraction

import numpy as np

LIN = np.linspace(0, 1, 256)  # a byte's probability, as ``rs masks`` un-quantises it


def histogram(prob, actual, classes, cls, stitched=False, ignore=None):
    """uint8 [B, H, W] twice -> (hist int64 [G, 2, 256], bad int64 [G], ignored int64 [G])."""

    prob, actual = np.asarray(prob), np.asarray(actual)
    groups = 1 if stitched else prob.shape[0]
    q, a = prob.reshape(groups, -1).astype(np.int64), actual.reshape(groups, -1).astype(np.int64)
    hist = np.zeros((groups, 2, 256), dtype=np.int64)
    bad, ignored = np.zeros(groups, dtype=np.int64), np.zeros(groups, dtype=np.int64)
    for g in range(groups):
        valid = a[g] < classes
        is_ignored = (a[g] == ignore) if ignore is not None else np.zeros_like(valid)
        ignored[g] = int(is_ignored.sum())
        bad[g] = int((~valid & ~is_ignored).sum())
        hist[g] = np.bincount((a[g][valid] == cls) * 256 + q[g][valid], minlength=512).reshape(2, 256)
    return hist, bad, ignored


def _frac(num, den):
    return Fraction(int(num), int(den)) if den else None


def _f(value):
    return None if value is None else float(value)


def point(q, y, k):
    """The operating point "predict the class where byte >= k" on the pixels ``q`` (bytes) and ``y`` (bool: the label is the class)."""

    predicted = q >= k
    tp, fp = int((predicted & y).sum()), int((predicted & ~y).sum())
    fn, tn = int((~predicted & y).sum()), int((~predicted & ~y).sum())
    return {"threshold_byte": k, "threshold": float(LIN[k]), "tp": tp, "fp": fp, "fn": fn, "tn": tn,
            "precision": _f(_frac(tp, tp + fp)), "recall": _f(_frac(tp, tp + fn)), "f1": _f(_frac(2 * tp, 2 * tp + fp + fn)),
            "iou": _f(_frac(tp, tp + fp + fn))}


def _exact(p, name):
    tp, fp, fn = p["tp"], p["fp"], p["fn"]
    return _frac(2 * tp, 2 * tp + fp + fn) if name == "f1" else _frac(tp, tp + fp + fn)


def best(points, name):
    """The first point (smallest k) among those with the highest exact score; None where none has one."""

    scored = [(_exact(p, name), p) for p in points if _exact(p, name) is not None]
    if not scored:
        return None
    top = max(s for s, _ in scored)
    return next(p for s, p in scored if s == top)


def auc(q, y):
    """The share of (positive, negative) pairs the positive wins, a tie counting half: every pair."""

    pos, neg = q[y].astype(np.int64), q[~y].astype(np.int64)
    if len(pos) == 0 or len(neg) == 0:
        return None
    wins = ties = 0
    for start in range(0, len(pos), 256):  # (every pair, 256 positives at a time: the table of a few tiles would not fit otherwise)
        diff = pos[start:start + 256, None] - neg[None, :]
        wins += int((diff > 0).sum())
        ties += int((diff == 0).sum())
    return _f(Fraction(2 * wins + ties, 2 * len(pos) * len(neg)))


def average_precision(q, y):
    """Step-wise AP over the distinct scores: the pixels sorted by decreasing byte, a step of recall times the precision at the end
    of every run of equal bytes."""

    positives = int(y.sum())
    if positives == 0:
        return None
    order = np.argsort(-q.astype(np.int64), kind="stable")
    qs, ys = q[order], y[order]
    total, tp, seen, last_tp = Fraction(0), 0, 0, 0
    for i in range(len(qs)):
        tp += int(ys[i])
        seen += 1
        if i + 1 == len(qs) or qs[i + 1] != qs[i]:
            total += Fraction(tp - last_tp, positives) * Fraction(tp, seen)
            last_tp = tp
    return _f(total)


def brier(q, y):
    if len(q) == 0:
        return None
    return _f(sum((Fraction(int(v), 255) - int(t)) ** 2 for v, t in zip(q.tolist(), y.tolist())) / len(q))


def calibration(q, y, bins=10):
    """(the table, ECE): every pixel put in the bin min(bins * q // 255, bins - 1) of its byte."""

    which = np.minimum(bins * q.astype(np.int64) // 255, bins - 1)
    table, ece = [], (Fraction(0) if len(q) else None)
    for b in range(bins):
        members = which == b
        n = int(members.sum())
        confidence = sum((Fraction(int(v), 255) for v in q[members].tolist()), Fraction(0)) / n if n else None
        accuracy = _frac(int(y[members].sum()), n)
        if n:
            ece += Fraction(n, len(q)) * abs(accuracy - confidence)
        table.append({"pixels": n, "confidence": _f(confidence), "accuracy": _f(accuracy)})
    return table, _f(ece)


def scores(prob, actual, classes, cls, ignore=None):
    """Everything the report's ``probability`` holds, over the pixels whose label is a class (a label equal to ``ignore`` is
    counted, any other is an error here), plus ``curve``: the 256 points."""

    q, a = np.asarray(prob).reshape(-1), np.asarray(actual).reshape(-1)
    is_ignored = (a == ignore) if ignore is not None else np.zeros(a.shape, dtype=bool)
    assert ((a < classes) | is_ignored).all()
    q, y = q[~is_ignored], a[~is_ignored] == cls
    points = [point(q, y, k) for k in range(256)]
    table, ece = calibration(q, y)
    return {"pixels": int(len(q)), "positives": int(y.sum()), "ignored": int(is_ignored.sum()), "ap": average_precision(q, y),
            "auc": auc(q, y), "brier": brier(q, y), "ece": ece, "calibration": table, "best_f1": best(points, "f1"),
            "best_iou": best(points, "iou"), "at_half": points[128], "curve": points}
