"""float64 numpy restatement of the native optimiser (robosat_amd/optim.py, csrc/optim.hip): the schedule table, the global gradient
norm with its clipping coefficient, and one AdamW step.  The yardstick of tests/test_gpu_optim.py; tests/test_optim_cpu.py pins it to
``torch.optim.AdamW`` / ``Adam`` in float64.  Written from the definitions, not from the code under test."""

import math

import numpy as np


def rates(lr, total_steps, kind="constant", power=0.9, warmup_steps=0, lr_min=0.0):
    out = np.empty(total_steps, dtype=np.float64)
    for t in range(total_steps):
        tau = (t - warmup_steps) / max(1, total_steps - warmup_steps)
        tau = min(1.0, max(0.0, tau))
        if kind == "constant":
            r = lr
        elif kind == "poly":
            r = lr_min + (lr - lr_min) * (1.0 - tau) ** power
        elif kind == "cosine":
            r = lr_min + (lr - lr_min) * (1.0 + math.cos(math.pi * tau)) / 2.0
        else:
            raise ValueError(kind)
        if t < warmup_steps:
            r = r * (t + 1) / warmup_steps
        out[t] = r
    return out


def table(lr, total_steps, kind="constant", power=0.9, warmup_steps=0, lr_min=0.0, betas=(0.9, 0.999), wd=0.0, ema=None):
    """float64 [T, 4]: (lr_t / (1 - b1^(t+1)), 1 / sqrt(1 - b2^(t+1)), 1 - lr_t wd, min(ema, (1 + t) / (10 + t)) or 0)."""

    r = rates(lr, total_steps, kind, power, warmup_steps, lr_min)
    out = np.empty((total_steps, 4), dtype=np.float64)
    for t in range(total_steps):
        out[t] = (r[t] / (1.0 - betas[0] ** (t + 1)), 1.0 / math.sqrt(1.0 - betas[1] ** (t + 1)), 1.0 - r[t] * wd,
                  0.0 if ema is None else min(ema, (1.0 + t) / (10.0 + t)))
    return out


def sumsq(grads):
    """The float64 sum of squares over a list of arrays (math.fsum: exact to the last rounding)."""

    return math.fsum(float(x) for g in grads for x in (np.asarray(g, dtype=np.float64).ravel() ** 2))


def coef(sumsq_value, clip):
    """clip_grad_norm_'s coefficient: min(1, clip / (norm + 1e-6))."""

    return min(1.0, clip / (math.sqrt(sumsq_value) + 1e-6))


def step(p, g, m, v, s, row, beta1, beta2, eps, decay, coef_value=None):
    """One step in float64 from arrays of any float type; returns (p', m', v', s' | None, u, g^)."""

    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    a, b, c, d = (float(x) for x in row)
    gh = g if coef_value is None else float(coef_value) * g
    m1 = beta1 * m + (1.0 - beta1) * gh
    v1 = beta2 * v + (1.0 - beta2) * gh * gh
    u = a * m1 / (np.sqrt(v1) * b + eps)
    p1 = (c * p if decay else p) - u
    s1 = None if s is None else d * np.asarray(s, dtype=np.float64) + (1.0 - d) * p1
    return p1, m1, v1, s1, u, gh
