"""CPU checks of the native optimiser's host side: the ``[opt]`` keys, the schedule table, the float64 reference against torch's own
AdamW / Adam, the optimiser's state layout, and the new symbols of the C ABI.  No kernel is launched here."""

import math
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as R
from robosat_amd.config import optimizer_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(**opt):
    return {"opt": dict({"lr": 0.001, "loss": "Lovasz", "epochs": 2}, **opt)}


# ---- option parsing -----------------------------------------------------------------------------------------------------------
def test_no_keys_is_the_reference_path():
    assert optimizer_options(_model()) is None
    assert optimizer_options({"opt": {"lr": "anything", "loss": "Lovasz"}}) is None  # (not even lr is looked at)


@pytest.mark.parametrize("opt, want", [
    ({"weight_decay": 0.01}, {"weight_decay": 0.01}),
    ({"weight_decay": 0}, {"weight_decay": 0.0}),
    ({"clip_norm": 1}, {"clip_norm": 1.0}),
    ({"ema": 0.999}, {"ema": 0.999}),
    ({"schedule": "constant"}, {"schedule": "constant"}),
    ({"schedule": "poly"}, {"schedule": "poly", "schedule_power": 0.9, "warmup_steps": 0, "lr_min": 0.0}),
    ({"schedule": "poly", "schedule_power": 2, "warmup_steps": 5, "lr_min": 1e-5},
     {"schedule": "poly", "schedule_power": 2.0, "warmup_steps": 5, "lr_min": 1e-5}),
    ({"schedule": "cosine", "warmup_steps": 3, "lr_min": 0.001}, {"schedule": "cosine", "warmup_steps": 3, "lr_min": 0.001}),
    ({"weight_decay": 0.05, "schedule": "cosine", "clip_norm": 0.5, "ema": 0.9},
     {"weight_decay": 0.05, "schedule": "cosine", "clip_norm": 0.5, "ema": 0.9}),
])
def test_accepted_keys(opt, want):
    got = optimizer_options(_model(**opt))
    base = {"weight_decay": 0.0, "schedule": None, "schedule_power": 0.9, "warmup_steps": 0, "lr_min": 0.0, "clip_norm": None, "ema": None}
    assert got == dict(base, **want)
    assert isinstance(got["warmup_steps"], int)


@pytest.mark.parametrize("opt, message", [
    ({"weight_decay": -0.1}, "[opt] weight_decay must be a finite number >= 0, got -0.1"),
    ({"weight_decay": "0.1"}, "[opt] weight_decay must be a finite number >= 0, got '0.1'"),
    ({"weight_decay": True}, "[opt] weight_decay must be a finite number >= 0, got true"),
    ({"weight_decay": float("inf")}, "[opt] weight_decay must be a finite number >= 0, got inf"),
    ({"clip_norm": 0}, "[opt] clip_norm must be a finite number > 0, got 0"),
    ({"clip_norm": -1.0}, "[opt] clip_norm must be a finite number > 0, got -1.0"),
    ({"clip_norm": float("nan")}, "[opt] clip_norm must be a finite number > 0, got nan"),
    ({"ema": 0}, "[opt] ema must be a number in (0, 1), got 0"),
    ({"ema": 1.0}, "[opt] ema must be a number in (0, 1), got 1.0"),
    ({"ema": "yes"}, "[opt] ema must be a number in (0, 1), got 'yes'"),
    ({"schedule": "step"}, "[opt] schedule must be one of \"constant\", \"poly\", \"cosine\", got 'step'"),
    ({"schedule": 1}, "[opt] schedule must be one of \"constant\", \"poly\", \"cosine\", got 1"),
    ({"schedule": "poly", "schedule_power": 0}, "[opt] schedule_power must be a finite number > 0, got 0"),
    ({"schedule": "poly", "warmup_steps": -1}, "[opt] warmup_steps must be an integer >= 0, got -1"),
    ({"schedule": "poly", "warmup_steps": 2.5}, "[opt] warmup_steps must be an integer >= 0, got 2.5"),
    ({"schedule": "poly", "warmup_steps": True}, "[opt] warmup_steps must be an integer >= 0, got true"),
    ({"schedule": "poly", "lr_min": -1e-6}, "[opt] lr_min must be a finite number in [0, lr], got -1e-06"),
    ({"schedule": "poly", "lr_min": 0.01}, "[opt] lr_min must be a finite number in [0, lr], got 0.01"),
    ({"schedule_power": 0.9}, "[opt] schedule_power needs [opt] schedule (one of \"constant\", \"poly\", \"cosine\")"),
    ({"warmup_steps": 10, "ema": 0.99}, "[opt] warmup_steps needs [opt] schedule (one of \"constant\", \"poly\", \"cosine\")"),
    ({"lr_min": 0.0, "weight_decay": 0.1}, "[opt] lr_min needs [opt] schedule (one of \"constant\", \"poly\", \"cosine\")"),
    ({"ema": 0.99, "lr": 0}, "[opt] lr must be a finite number > 0 for the native optimiser, got 0"),
])
def test_refused_keys(opt, message):
    with pytest.raises(ValueError) as err:
        optimizer_options(_model(**opt))
    assert str(err.value) == message


# ---- the schedule table -------------------------------------------------------------------------------------------------------
def test_table_rows_against_closed_forms():
    from robosat_amd.optim import schedule_table

    lr, T, w, lr_min, power, b1, b2, wd, ema = 0.01, 100, 10, 0.001, 0.9, 0.9, 0.999, 0.05, 0.99
    for kind in ("poly", "cosine"):
        table = schedule_table(lr, T, kind, power, w, lr_min, (b1, b2), wd, ema)
        assert table.dtype == torch.float32 and tuple(table.shape) == (T, 4)

        def shape(tau):
            return (1 - tau) ** power if kind == "poly" else (1 + math.cos(math.pi * tau)) / 2

        def row(t, rate):
            return np.array([rate / (1 - b1 ** (t + 1)), 1 / math.sqrt(1 - b2 ** (t + 1)), 1 - rate * wd, min(ema, (1 + t) / (10 + t))],
                            dtype=np.float64).astype(np.float32)

        # first row (tau clamps to 0: the full rate, times 1 / warmup), the last warm-up row, the first full row, middle, last
        cases = {0: lr / w, w - 1: lr * w / w, w: lr, 55: lr_min + (lr - lr_min) * shape(45 / 90), T - 1: lr_min + (lr - lr_min) * shape(89 / 90)}
        for t, rate in cases.items():
            assert np.array_equal(table[t].numpy(), row(t, rate)), (kind, t)
        # and every row against the float64 restatement, rounded once
        assert np.array_equal(table.numpy(), R.table(lr, T, kind, power, w, lr_min, (b1, b2), wd, ema).astype(np.float32))


def test_table_constant_without_decay_or_ema():
    from robosat_amd.optim import schedule_table

    table = schedule_table(0.003, 50, "constant").numpy()
    assert np.all(table[:, 2] == 1.0)  # c_t exactly 1: p passes through the decay untouched
    assert np.all(table[:, 3] == 0.0)
    assert table[0, 0] == np.float32(0.003 / (1 - 0.9)) and table[0, 1] == np.float32(1 / math.sqrt(1 - 0.999))


def test_table_ema_decay_is_monotone_and_reaches_ema():
    from robosat_amd.optim import saturation_steps, schedule_table

    d = schedule_table(0.001, 2000, "constant", ema=0.99).numpy()[:, 3]
    assert d[0] == np.float32(0.1) and np.all(np.diff(d) >= 0) and d[-1] == np.float32(0.99)
    assert d[889] < np.float32(0.99) and d[890] == np.float32(0.99)  # (1 + t) / (10 + t) >= 0.99 from t = 890: 0.01 t >= 8.9
    # a table without a set length ends where nothing moves any more: the last row is every later step's
    T = saturation_steps((0.9, 0.999), 0.99)
    last = schedule_table(0.001, T + 1, "constant", ema=0.99).numpy()
    assert np.array_equal(last[T - 1], last[T]) and last[T - 1, 1] == 1.0 and last[T - 1, 0] == np.float32(0.001)


def test_schedule_errors():
    from robosat_amd.optim import schedule_table

    with pytest.raises(ValueError):
        schedule_table(0.001, 10, "step")
    with pytest.raises(ValueError):
        schedule_table(0.001, 0, "poly")


# ---- the reference is torch's definition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_reference_is_torch_adamw_and_adam_in_float64(wd):
    rng = np.random.default_rng(7)
    shapes = [(5, 3), (7,), (2, 3, 2, 2)]
    lr, b1, b2, eps, steps = 0.01, 0.9, 0.999, 1e-8, 10
    p0 = [rng.standard_normal(s) for s in shapes]
    grads = [[rng.standard_normal(s) * 10.0 ** rng.integers(-3, 2) for s in shapes] for _ in range(steps)]
    params = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p0]
    # (decay on every tensor here: torch's optimisers know no exemption; the flag itself is checked on the GPU)
    opt = (torch.optim.AdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd) if wd
           else torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps))
    table = R.table(lr, steps, "constant", betas=(b1, b2), wd=wd)
    p, m, v = [x.copy() for x in p0], [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    for t in range(steps):
        for i, q in enumerate(params):
            q.grad = torch.from_numpy(grads[t][i].copy())
            p[i], m[i], v[i], _, _, _ = R.step(p[i], grads[t][i], m[i], v[i], None, table[t], b1, b2, eps, True)
        opt.step()
    for i, q in enumerate(params):
        np.testing.assert_allclose(p[i], q.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(m[i], opt.state[q]["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v[i], opt.state[q]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)


def test_reference_norm_and_coef_are_clip_grad_norm():
    rng = np.random.default_rng(3)
    grads = [rng.standard_normal(n) for n in (5, 1, 130)]
    params = [torch.nn.Parameter(torch.zeros(len(g), dtype=torch.float64)) for g in grads]
    for q, g in zip(params, grads):
        q.grad = torch.from_numpy(g.copy())
    total = float(torch.nn.utils.clip_grad_norm_(params, 0.5))
    ss = R.sumsq(grads)
    assert abs(math.sqrt(ss) - total) <= 1e-12 * total
    for q, g in zip(params, grads):
        np.testing.assert_allclose(q.grad.numpy(), R.coef(ss, 0.5) * g, rtol=1e-12, atol=0)
    assert R.coef(ss, 1e9) == 1.0


# ---- the optimiser's host side --------------------------------------------------------------------------------------------------
def test_state_layout_and_decay_rule_on_the_host():
    from robosat_amd.optim import AdamW

    conv = torch.nn.Conv2d(3, 4, 3)
    bn = torch.nn.BatchNorm2d(4)
    params = list(conv.parameters()) + list(bn.parameters())
    opt = AdamW(params, lr=0.01, weight_decay=0.1, ema=0.9, clip_norm=1.0, schedule={"kind": "poly", "total_steps": 7, "warmup_steps": 2})
    assert all(g["capturable"] is True for g in opt.param_groups)
    stock = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).param_groups[0]
    assert set(stock) <= set(opt.param_groups[0])  # a stock Adam that loads these groups finds every key it reads
    state = opt.state_dict()
    assert set(state) == {"state", "param_groups", "ema"} and state["state"] == {}
    assert len(state["ema"]) == len(params) and all(torch.equal(s, p) for s, p in zip(state["ema"], params))
    assert opt.lr_at(0) == 0.005 and opt.lr_at(1) == 0.01 and opt.lr_at(10 ** 9) == opt.lr_at(6) and opt.steps_taken() == 0
    assert "poly" in opt.describe() and "ema = 0.9" in opt.describe() and "clip_norm = 1.0" in opt.describe()
    # a stock Adam's state resumes here: moments and step counter as saved, the shadow from the parameters
    adam = torch.optim.Adam(params, lr=0.01)
    for q in params:
        q.grad = torch.ones_like(q)
    adam.step()
    adam.step()
    opt.load_state_dict(adam.state_dict())
    assert opt.steps_taken() == 2 and all(g["capturable"] is True and g["weight_decay"] == 0.1 for g in opt.param_groups)
    assert torch.equal(opt.state[params[0]]["exp_avg"], adam.state[params[0]]["exp_avg"])
    assert all(torch.equal(s, p) for s, p in zip(opt.shadows, params))
    # ... and the other way round
    fresh = torch.optim.Adam(params, lr=0.01)
    fresh.load_state_dict(opt.state_dict())
    assert float(fresh.state[params[1]]["step"]) == 2.0
    with pytest.raises(ValueError):
        AdamW(params, lr=0.01, ema=1.0)
    with pytest.raises(ValueError):
        AdamW(params, lr=0.01, clip_norm=0.0)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    from robosat_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    for name in ("rs_optim_limits", "rs_optim_workspace_bytes", "rs_optim_grad_norm", "rs_optim_step"):
        assert re.search(r"\b{}\s*\(".format(name), header), name
        assert name in _lib.SIGNATURES, name
    assert "typedef struct rs_optim_item" in header
    assert _lib.ABI_VERSION == 24
    assert re.search(r"int\s+rs_abi_version\s*\(\s*(void)?\s*\)\s*\{\s*return\s+24\s*;", "".join(
        open(os.path.join(ROOT, "robosat_amd", "csrc", n)).read() for n in sorted(os.listdir(os.path.join(ROOT, "robosat_amd", "csrc")))
        if n.endswith(".hip")))
    import ctypes

    assert ctypes.sizeof(ops._OptimItem) == 56 and ops._OptimItem.numel.offset == 40 and ops._OptimItem.decay.offset == 48


def test_item_struct_layout_matches_the_c_header(tmp_path):
    """The ctypes mirror of rs_optim_item against what gcc makes of the declaration (the header compiles as plain C)."""
    import ctypes
    import shutil
    import subprocess

    from robosat_amd import ops

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "robosat_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rs_optim_item));']
    for name, _ in ops._OptimItem._fields_:
        lines.append('  printf("{0} %zu\\n", offsetof(rs_optim_item, {0}));'.format(name))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(ops._OptimItem)
    for name, _ in ops._OptimItem._fields_:
        assert int(got[name]) == getattr(ops._OptimItem, name).offset, name
