"""References for the clDice topology loss and its soft skeleton (include/robosat_hip.h).

``soft_skeleton`` / ``cldice_term`` are the definition written with torch CPU ops; with ``requires_grad`` inputs they double as the
autograd reference, in float32 and float64 alike.  ``soft_skeleton_paper`` is the paper's published form, which recomputes the erosion
inside every opening.  ``skeleton_bwd_numpy`` is an explicit per-pixel implementation of the backward tie rules in scatter form:
it shares no code with torch's autograd and none of its structure with the kernels' gather form."""

import numpy as np
import torch
import torch.nn.functional as F


def erode(x):
    """min(v, h) of planes [M, H, W]: v over (N, C, S), h over (W, C, E); max_pool2d pads with -inf, so nothing lies beyond the edge."""

    v = -F.max_pool2d(-x, (3, 1), (1, 1), (1, 0))
    h = -F.max_pool2d(-x, (1, 3), (1, 1), (0, 1))
    return torch.min(v, h)


def dilate(x):
    return F.max_pool2d(x, (3, 3), (1, 1), (1, 1))


def soft_skeleton(x, iters):
    """The shared-erosion form: E_{k+1} = erode(E_k), D_k = relu(E_k - dilate(E_{k+1})), S_k = S_{k-1} + relu(D_k - S_{k-1} D_k)."""

    e = x
    skel = None
    for _ in range(iters + 1):
        nxt = erode(e)
        d = F.relu(e - dilate(nxt))
        skel = d if skel is None else skel + F.relu(d - skel * d)
        e = nxt
    return skel


def soft_skeleton_paper(x, iters):
    """``soft_skel`` as published with the paper (clDice/cldice_loss/pytorch/soft_skeleton.py)."""

    def soft_open(img):
        return dilate(erode(img))

    img = x
    skel = F.relu(img - soft_open(img))
    for _ in range(iters):
        img = erode(img)
        delta = F.relu(img - soft_open(img))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def cldice_planes(logits, targets, classes=None, ignore=None, dtype=torch.float32):
    """(P, Y), each [N * K, H, W] in the order [image][class ascending], both zeroed under the ignore label."""

    n, c, h, w = logits.shape
    picked = list(range(1, c)) if classes is None else sorted(classes)
    probs = torch.softmax(logits.to(dtype), dim=1)
    valid = torch.ones_like(targets, dtype=dtype) if ignore is None else (targets != ignore).to(dtype)
    p = torch.stack([probs[:, k] * valid for k in picked], dim=1).reshape(n * len(picked), h, w)
    y = torch.stack([(targets == k).to(dtype) * valid for k in picked], dim=1).reshape(n * len(picked), h, w)
    return p, y


def cldice_term(logits, targets, iters, smooth=1.0, classes=None, ignore=None, dtype=torch.float32):
    """The clDice term: the mean over all (image, class) pairs of 1 - 2 Tprec Tsens / (Tprec + Tsens)."""

    p, y = cldice_planes(logits, targets, classes, ignore, dtype)
    sp = soft_skeleton(p, iters)
    sy = soft_skeleton(y, iters)
    tprec = ((sp * y).sum(dim=(1, 2)) + smooth) / (sp.sum(dim=(1, 2)) + smooth)
    tsens = ((sy * p).sum(dim=(1, 2)) + smooth) / (sy.sum(dim=(1, 2)) + smooth)
    return (1.0 - 2.0 * tprec * tsens / (tprec + tsens)).mean()


def skeleton_autograd(x, iters, grad, dtype=torch.float32):
    """(skeleton, d / d x of sum(skeleton * grad)) by torch CPU autograd in ``dtype``, from the bits of ``x`` and ``grad``."""

    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    skel = soft_skeleton(xx, iters)
    (dx,) = torch.autograd.grad(skel, xx, grad.detach().cpu().to(dtype))
    return skel.detach(), dx


def _first_min(values):
    """Index of the first of ``values`` (a list of (value, cell)) attaining the minimum."""

    best = 0
    for i in range(1, len(values)):
        if values[i][0] < values[best][0]:
            best = i
    return best


def _erode_numpy(e):
    h, w = e.shape
    out = np.empty_like(e)
    sel = {}
    for y in range(h):
        for x in range(w):
            vert = [(e[yy, x], (yy, x)) for yy in (y - 1, y, y + 1) if 0 <= yy < h]
            hori = [(e[y, xx], (y, xx)) for xx in (x - 1, x, x + 1) if 0 <= xx < w]
            v, hh = vert[_first_min(vert)], hori[_first_min(hori)]
            out[y, x] = min(v[0], hh[0])
            if v[0] < hh[0]:
                sel[(y, x)] = [(v[1], 1.0)]
            elif hh[0] < v[0]:
                sel[(y, x)] = [(hh[1], 1.0)]
            else:
                sel[(y, x)] = [(v[1], 0.5), (hh[1], 0.5)]
    return out, sel


def _dilate_numpy(e):
    h, w = e.shape
    out = np.empty_like(e)
    sel = {}
    for y in range(h):
        for x in range(w):
            best = None
            for yy in (y - 1, y, y + 1):
                for xx in (x - 1, x, x + 1):
                    if 0 <= yy < h and 0 <= xx < w and (best is None or e[yy, xx] > e[best]):
                        best = (yy, xx)
            out[y, x] = e[best]
            sel[(y, x)] = best
    return out, sel


def skeleton_bwd_numpy(x, iters, grad):
    """d / d x of sum(skeleton(x) * grad) for planes [M, H, W] by the tie rules, pixel by pixel, in the dtype of ``x``."""

    x = np.asarray(x)
    grad = np.asarray(grad, dtype=x.dtype)
    out = np.zeros_like(x)
    for m in range(x.shape[0]):
        es, erode_sel, dil_sel, ds, ss = [x[m]], [], [], [], []
        for k in range(iters + 1):
            nxt, sel = _erode_numpy(es[k])
            es.append(nxt)
            erode_sel.append(sel)
            o, dsel = _dilate_numpy(nxt)
            dil_sel.append(dsel)
            diff = es[k] - o
            ds.append((np.maximum(diff, 0), diff > 0))
            d = ds[k][0]
            ss.append(d if k == 0 else ss[k - 1] + np.maximum(d - ss[k - 1] * d, 0))
        ge = [np.zeros_like(x[m]) for _ in range(iters + 2)]
        gs = grad[m].copy()
        gd = [None] * (iters + 1)
        for k in range(iters, 0, -1):
            d = ds[k][0]
            on = (d - ss[k - 1] * d) > 0
            gr = np.where(on, gs, 0).astype(x.dtype)
            gd[k] = gr - gr * ss[k - 1]
            gs = gs - gr * d
        gd[0] = gs
        for k in range(iters, -1, -1):
            g = np.where(ds[k][1], gd[k], 0).astype(x.dtype)  # relu'(0) = 0
            ge[k] += g
            for cell, src in dil_sel[k].items():  # O_k = dilate(E_{k+1}) enters with a minus sign
                ge[k + 1][src] -= g[cell]
        for k in range(iters, -1, -1):
            for cell, parts in erode_sel[k].items():
                for src, share in parts:
                    ge[k][src] += x.dtype.type(share) * ge[k + 1][cell]
        out[m] = ge[0]
    return out
