"""The native optimiser step on the MI355X (csrc/optim.hip, robosat_amd/optim.py) against the float64 reference of tests/optim_ref.py.

Bounds of one step, from the operation count (u is seven rounded operations, at most 8 * 2^-24 relative, doubled):
    |m' - m'_ref| <= 2^-22 (|beta1 m| + |(1 - beta1) g^|)          |v' - v'_ref| likewise with g^ g^
    |p' - p'_ref| <= 2^-23 |p| + 2^-20 |u_ref|
    |s' - s'_ref| <= 2^-22 (|s| + |p'_ref|) + |p' - p'_ref|
The bound of p' is relative to |u_ref| and counts u's own operations: it presumes that m' carries the relative accuracy of its two
operands, which holds where they do not cancel.  The random inputs therefore give m the sign of g (an Adam moment has the sign of the
recent gradients); an item of mixed signs is stepped too and held to the bounds of m', v' and s', which are cancellation-proof, and to
the bound of p' plus the bound of m' carried through u = a m' / den.
"""

import copy
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
GUARD = 4  # floats either side of every tensor (a multiple of 4: the view keeps the buffer's 16-byte alignment)
SENTINEL = -7.25e30
B1, B2, EPS = 0.9, 0.999, 1e-8
B1F, B2F, EPSF = (float(np.float32(x)) for x in (B1, B2, EPS))  # what the kernel receives: the reference computes with these


@pytest.fixture(scope="module")
def limits():
    from robosat_amd import ops

    chunk, items = ops.optim_limits()
    assert chunk >= 256 and chunk % 4 == 0 and items >= 8
    return chunk, items


def _sizes(chunk):
    return [1, 3, 4, 5, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]


class Guarded:
    """A device tensor of ``n`` floats with guard words either side; ``off`` = 1 starts it 4 bytes off a 16-byte boundary."""

    def __init__(self, values, off=0):
        n = len(values)
        self.buf = torch.full((n + 2 * GUARD + 4,), SENTINEL, device=DEV, dtype=torch.float32)
        self.lo = GUARD + off
        self.t = self.buf[self.lo:self.lo + n]
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
        assert self.t.data_ptr() % 16 == 4 * off

    def get(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:self.lo] == np.float32(SENTINEL)) and np.all(b[self.lo + self.t.numel():] == np.float32(SENTINEL)))


def _magnitudes(rng, n, lo, hi):
    return 10.0 ** rng.uniform(lo, hi, n)


def _make_item(rng, n, index, mixed=False):
    """fp32 inputs of one item: magnitudes from 1e-8 to 1e3 (v: their squares' range), the first element all zero (u must be 0)."""

    g = (_magnitudes(rng, n, -8, 3) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], n) if mixed else np.sign(g)
    m = (_magnitudes(rng, n, -8, 3) * sign).astype(np.float32)
    v = _magnitudes(rng, n, -16, 6).astype(np.float32)
    p = (_magnitudes(rng, n, -8, 3) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    s = (_magnitudes(rng, n, -8, 3) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[0] = m[0] = v[0] = 0.0
    return {"p": p, "g": g, "m": m, "v": v, "s": s if index % 2 else None, "decay": bool((index // 2) % 2), "off": int(index % 5 == 3)}


def _upload(items):
    dev = []
    for it in items:
        dev.append({k: (None if it[k] is None else Guarded(it[k], it["off"])) for k in ("p", "g", "m", "v", "s")})
    return dev


def _entries(items, dev):
    return [(d["p"].t, d["g"].t, d["m"].t, d["v"].t, None if d["s"] is None else d["s"].t, it["decay"]) for it, d in zip(items, dev)]


def _ctl(step=0, coef=1.0):
    ctl = torch.zeros(32, device=DEV, dtype=torch.uint8)
    ctl.view(torch.int64)[0:1].fill_(step)
    ctl.view(torch.float32)[4:5].fill_(coef)
    return ctl


def _check_item(it, d, row, coef, mixed=False):
    """One stepped item against the float64 reference; returns the worst ratio error / bound seen (p')."""

    p1, m1, v1, s1, u, gh = R.step(it["p"], it["g"], it["m"], it["v"], it["s"], row, B1F, B2F, EPSF, it["decay"], coef)
    gp, gm, gv = (d[k].get().astype(np.float64) for k in ("p", "m", "v"))
    m64, v64, p64 = (it[k].astype(np.float64) for k in ("m", "v", "p"))
    bm = 2.0 ** -22 * (np.abs(B1F * m64) + np.abs((1 - B1F) * gh))
    bv = 2.0 ** -22 * (np.abs(B2F * v64) + np.abs((1 - B2F) * gh * gh))
    bp = 2.0 ** -23 * np.abs(p64) + 2.0 ** -20 * np.abs(u)
    if mixed:  # the bound of m' carried through u = a m' / den (module docstring)
        bp = bp + float(row[0]) * bm / (np.sqrt(v1) * float(row[1]) + EPSF) * (1 + 2.0 ** -20)
    assert np.all(np.abs(gm - m1) <= bm), ("m", float(np.max(np.abs(gm - m1) / np.maximum(bm, 1e-300))))
    assert np.all(np.abs(gv - v1) <= bv), ("v", float(np.max(np.abs(gv - v1) / np.maximum(bv, 1e-300))))
    ep = np.abs(gp - p1)
    worst = float(np.max(ep / np.maximum(bp, 1e-300)))
    assert np.all(ep <= bp), ("p", worst, int(np.argmax(ep / np.maximum(bp, 1e-300))))
    if it["s"] is not None:
        gs = d["s"].get().astype(np.float64)
        bs = 2.0 ** -22 * (np.abs(it["s"].astype(np.float64)) + np.abs(p1)) + ep
        assert np.all(np.abs(gs - s1) <= bs), ("s", float(np.max(np.abs(gs - s1) / np.maximum(bs, 1e-300))))
    # v = 0 with g = 0 (and m = 0): u is exactly 0, p' is c p (one rounding) or p itself
    want0 = np.float32(row[2]) * it["p"][0] if it["decay"] else it["p"][0]
    assert d["p"].get()[0] == want0 and d["m"].get()[0] == 0.0 and d["v"].get()[0] == 0.0
    assert np.array_equal(d["g"].get().view(np.uint32), it["g"].view(np.uint32))  # g is read, never written
    assert all(d[k].guards_intact() for k in ("p", "g", "m", "v", "s") if d[k] is not None)
    return worst


def _table():
    from robosat_amd.optim import schedule_table

    return schedule_table(0.01, 9, "poly", 0.9, 3, 1e-4, (B1, B2), 0.05, 0.9)


@pytest.mark.parametrize("use_coef", [0, 1])
@pytest.mark.parametrize("count", ["ITEMS-1", "ITEMS", "ITEMS+1", "2*ITEMS+1"])
def test_one_step_against_the_float64_reference(limits, count, use_coef):
    from robosat_amd import ops

    chunk, nitems = limits
    n = {"ITEMS-1": nitems - 1, "ITEMS": nitems, "ITEMS+1": nitems + 1, "2*ITEMS+1": 2 * nitems + 1}[count]
    sizes = _sizes(chunk)
    rng = np.random.default_rng(1000 + n + use_coef)
    items = [_make_item(rng, sizes[i % len(sizes)], i + i // len(sizes)) for i in range(n)]
    assert any(it["off"] for it in items) and {(it["s"] is None, it["decay"]) for it in items} == {(a, b) for a in (True, False) for b in (True, False)}
    dev = _upload(items)
    table = _table()
    step, coef = 4, np.float32(0.37)
    ctl = _ctl(step, float(coef))
    arr, chunks = ops.optim_items(_entries(items, dev))
    assert chunks == sum((len(it["p"]) + chunk - 1) // chunk for it in items)
    ops.optim_step(arr, table.to(DEV), ctl, B1, B2, EPS, use_coef)
    torch.cuda.synchronize()
    row = table[step].numpy().astype(np.float64)
    worst = max(_check_item(it, d, row, float(coef) if use_coef else None) for it, d in zip(items, dev))
    print("{} items, use_coef {}: worst |p' - p'_ref| / bound = {:.3f}".format(n, use_coef, worst))
    assert int(ctl.view(torch.int64)[0]) == step + 1  # advanced once, behind the element pass


def test_one_step_of_mixed_signs_and_rows_beyond_the_table(limits):
    from robosat_amd import ops

    chunk, _ = limits
    rng = np.random.default_rng(77)
    items = [_make_item(rng, n, i, mixed=True) for i, n in enumerate([chunk + 5, 65, 2 * chunk + 3, 7])]
    dev = _upload(items)
    table = _table()
    ctl = _ctl(1000)  # beyond T - 1: the last row
    arr, _ = ops.optim_items(_entries(items, dev))
    ops.optim_step(arr, table.to(DEV), ctl, B1, B2, EPS, 0)
    torch.cuda.synchronize()
    row = table[-1].numpy().astype(np.float64)
    for it, d in zip(items, dev):
        _check_item(it, d, row, None, mixed=True)


def test_invalid_arguments_are_refused(limits):
    from robosat_amd import ops

    x = [torch.zeros(8, device=DEV) for _ in range(5)]
    table, ctl = _table().to(DEV), _ctl()
    arr, _ = ops.optim_items([(x[0], x[1], x[2], x[3], x[4], True)])
    ws = torch.empty(64, device=DEV, dtype=torch.uint8)
    for bad in (dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1.0), dict(eps=float("nan"))):
        kw = dict(beta1=B1, beta2=B2, eps=EPS)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.optim_step(arr, table, ctl, kw["beta1"], kw["beta2"], kw["eps"], 0)
    for clip in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.optim_grad_norm(arr, clip, ctl, ws)
    arr[0].numel = 0
    with pytest.raises(ValueError):
        ops.optim_step(arr, table, ctl, B1, B2, EPS, 0)
    arr[0].numel = 8
    arr[0].m = None
    with pytest.raises(ValueError):
        ops.optim_step(arr, table, ctl, B1, B2, EPS, 0)
    arr[0].m = x[2].data_ptr() + 2  # misaligned
    with pytest.raises(ValueError):
        ops.optim_step(arr, table, ctl, B1, B2, EPS, 0)
    with pytest.raises(ValueError):  # tensors in different memory orders
        ops.optim_items([(torch.zeros(4, 6, device=DEV), torch.zeros(6, 4, device=DEV).t(), torch.zeros(4, 6, device=DEV),
                          torch.zeros(4, 6, device=DEV), None, True)])
    torch.cuda.synchronize()
    assert int(ctl.view(torch.int64)[0]) == 0 and all(float(t.abs().sum()) == 0.0 for t in x)  # nothing was enqueued


def test_grad_norm(limits):
    from robosat_amd import ops

    chunk, nitems = limits
    rng = np.random.default_rng(5)
    sizes = (_sizes(chunk) * ((nitems + 12) // 11 + 1))[:nitems + 3]  # crosses the launch-block edge
    # one flat buffer, NaN between the items (the arena's padding is uninitialised memory): item i starts 16-byte aligned, bar every fifth
    starts, at = [], 4
    for i, n in enumerate(sizes):
        at = (at + 3) // 4 * 4 + (1 if i % 5 == 3 else 0)
        starts.append(at)
        at += n + 2
    flat = np.full(at + 8, np.nan, dtype=np.float32)
    grads = []
    for s, n in zip(starts, sizes):
        flat[s:s + n] = (_magnitudes(rng, n, -6, 2) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        grads.append(flat[s:s + n].copy())
    buf = torch.from_numpy(flat).to(DEV)
    dummy = torch.zeros(max(sizes), device=DEV)
    entries = [(dummy[:n], buf[s:s + n], dummy[:n], dummy[:n], None, False) for s, n in zip(starts, sizes)]
    arr, chunks = ops.optim_items(entries)
    ws = torch.empty(ops.optim_workspace_bytes(chunks), device=DEV, dtype=torch.uint8)
    want = R.sumsq(grads)

    def run(clip):
        ctl = _ctl()
        ops.optim_grad_norm(arr, clip, ctl, ws)
        torch.cuda.synchronize()
        return ctl.cpu()

    big = run(2.0 * math.sqrt(want))
    got = float(big.view(torch.float64)[1])
    print("sumsq {:.17e} against {:.17e}: relative error {:.2e}".format(got, want, abs(got - want) / want))
    assert abs(got - want) <= 1e-12 * want
    assert float(big.view(torch.float32)[4]) == 1.0  # the norm is below clip: exactly 1
    assert torch.equal(big, run(2.0 * math.sqrt(want)))  # the same bits on a second run
    clip = 0.25 * math.sqrt(want)
    small = run(clip)
    coef = float(small.view(torch.float32)[4])
    assert abs(coef - R.coef(want, float(np.float32(clip)))) <= 2.0 ** -23 * coef and coef < 0.2500001
    assert int(small.view(torch.int64)[0]) == 0  # the norm does not move the step counter
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), flat.view(np.uint32))
    # a non-finite norm propagates, as clip_grad_norm_(error_if_nonfinite=False) lets it
    buf[starts[2]] = float("nan")
    assert math.isnan(float(run(1.0).view(torch.float32)[4]))


def test_grouping_independence(limits):
    from robosat_amd import ops

    chunk, nitems = limits
    rng = np.random.default_rng(11)
    probe = _make_item(rng, 2 * chunk + 3, 3)  # (index 3: with a shadow, with decay, 4 bytes off the 16-byte boundary)
    assert probe["s"] is not None and probe["decay"] and probe["off"] == 1
    table = _table().to(DEV)
    alone = _upload([probe])
    arr, _ = ops.optim_items(_entries([probe], alone))
    ops.optim_step(arr, table, _ctl(2, 0.5), B1, B2, EPS, 1)
    others = [_make_item(rng, [5, 64, chunk + 1][i % 3], i) for i in range(nitems + 5)]
    others[nitems + 3] = probe
    many = _upload(others)
    arr, _ = ops.optim_items(_entries(others, many))
    ops.optim_step(arr, table, _ctl(2, 0.5), B1, B2, EPS, 1)
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "s"):
        assert np.array_equal(alone[0][k].get().view(np.uint32), many[nitems + 3][k].get().view(np.uint32)), k


# ---- the optimiser class ---------------------------------------------------------------------------------------------------------
SHAPES = [(65, 33), (300,), (3, 5, 3, 3), (1,)]
HYPER = dict(lr=0.01, betas=(B1, B2), eps=EPS, weight_decay=0.05, clip_norm=1.5, ema=0.9,
             schedule={"kind": "poly", "total_steps": 20, "power": 0.9, "warmup_steps": 4, "lr_min": 1e-4})


@pytest.fixture(scope="module")
def run20():
    """20 steps of fixed parameters and gradients: the inputs, shared and left unchanged."""

    rng = np.random.default_rng(2024)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    grads = [[(rng.standard_normal(s) * 10.0 ** rng.uniform(-2, 1)).astype(np.float32) for s in SHAPES] for _ in range(20)]
    return p0, grads


def _native(p0, **over):
    from robosat_amd.optim import AdamW

    params = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in p0]
    return params, AdamW(params, **dict(HYPER, **over))


def _steps(params, opt, grads, first, last):
    for t in range(first, last):
        for q, g in zip(params, grads[t]):
            q.grad = torch.from_numpy(g).to(DEV)
        opt.step()


def test_trajectory_of_20_steps(run20):
    p0, grads = run20
    params, opt = _native(p0)
    _steps(params, opt, grads, 0, 20)
    torch.cuda.synchronize()
    assert opt.steps_taken() == 20
    table = opt._table_host.numpy().astype(np.float64)

    # the float64 trajectory from the same fp32 table, with the clipping coefficient as the float the definition makes it
    p, m, v = [x.astype(np.float64) for x in p0], [np.zeros(s) for s in SHAPES], [np.zeros(s) for s in SHAPES]
    s = [x.astype(np.float64) for x in p0]
    one_step = 0.0
    for t in range(20):
        coef = float(np.float32(R.coef(R.sumsq(grads[t]), HYPER["clip_norm"])))
        for i in range(len(SHAPES)):
            before = np.abs(p[i])
            p[i], m[i], v[i], s[i], u, _ = R.step(p[i], grads[t][i], m[i], v[i], s[i], table[t], B1F, B2F, EPSF, len(SHAPES[i]) > 1, coef)
            one_step = max(one_step, float(np.max(2.0 ** -23 * before + 2.0 ** -20 * np.abs(u))))

    # torch's fused AdamW on the same schedule (the table's rates through lr as a tensor, decay on the same tensors, no EMA)
    tparams = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in p0]
    lr = torch.zeros((), device=DEV)
    groups = [{"params": [q for q in tparams if q.dim() > 1], "weight_decay": HYPER["weight_decay"]},
              {"params": [q for q in tparams if q.dim() <= 1], "weight_decay": 0.0}]
    topt = torch.optim.AdamW(groups, lr=lr, betas=(B1, B2), eps=EPS, fused=True)
    for t in range(20):
        for g in topt.param_groups:
            g["lr"].fill_(float(opt.rates[t]))
        for q, g in zip(tparams, grads[t]):
            q.grad = torch.from_numpy(g).to(DEV)
        torch.nn.utils.clip_grad_norm_(tparams, HYPER["clip_norm"])
        topt.step()
    torch.cuda.synchronize()

    dev_native = max(float(np.max(np.abs(q.detach().cpu().numpy().astype(np.float64) - r))) for q, r in zip(params, p))
    dev_torch = max(float(np.max(np.abs(q.detach().cpu().numpy().astype(np.float64) - r))) for q, r in zip(tparams, p))
    dev_shadow = max(float(np.max(np.abs(q.cpu().numpy().astype(np.float64) - r))) for q, r in zip(opt.shadows, s))
    print("max |p - p_ref| after 20 steps: native {:.3e}, torch fused AdamW {:.3e}; one-step bound {:.3e}; shadow {:.3e}".format(
        dev_native, dev_torch, one_step, dev_shadow))
    assert dev_native <= max(2.0 * dev_torch, 20.0 * one_step)
    # (the shadow is an average of the p' it saw: their deviation, plus its own 20 roundings of values of |p|'s size)
    assert dev_shadow <= max(2.0 * dev_torch, 20.0 * one_step) + 20 * 2.0 ** -22 * max(float(np.max(np.abs(x))) for x in p)
    # the schedule did fall, and the 1-D tensors were not decayed: step them again without a gradient signal to see the rule
    assert opt.lr_at(3) == 0.01 and opt.lr_at(19) < opt.lr_at(10) < 0.01


def test_decay_exemption_and_missing_gradients(run20):
    p0, _ = run20
    params, opt = _native(p0, clip_norm=None, ema=0.5, schedule=None, lr=0.1, weight_decay=0.5)
    for q in params[:3]:
        q.grad = torch.zeros_like(q)  # g = 0: u = 0, so p' = c p where the tensor decays and p where it does not
    opt.step()
    torch.cuda.synchronize()
    c = np.float32(1.0 - 0.1 * 0.5)
    assert np.array_equal(params[0].detach().cpu().numpy(), c * p0[0]) and np.array_equal(params[2].detach().cpu().numpy(), c * p0[2])
    assert np.array_equal(params[1].detach().cpu().numpy(), p0[1])  # one dimension: no decay
    # the parameter without a gradient: untouched, no state, its shadow still the copy
    assert np.array_equal(params[3].detach().cpu().numpy(), p0[3]) and params[3] not in opt.state
    assert np.array_equal(opt.shadows[3].cpu().numpy(), p0[3])
    assert set(opt.state[params[0]]) == {"step", "exp_avg", "exp_avg_sq"}
    # swap_ema exchanges the contents and puts them back
    raw = [q.detach().clone() for q in params]
    ema = [s.clone() for s in opt.shadows]
    ptrs = [q.data_ptr() for q in params]
    with opt.swap_ema():
        assert all(torch.equal(q, e) for q, e in zip(params, ema)) and all(torch.equal(s, r) for s, r in zip(opt.shadows, raw))
    assert all(torch.equal(q, r) for q, r in zip(params, raw)) and all(torch.equal(s, e) for s, e in zip(opt.shadows, ema))
    assert ptrs == [q.data_ptr() for q in params] and not torch.equal(raw[0], ema[0])


def test_state_round_trip(run20):
    p0, grads = run20
    straight, opt_a = _native(p0)
    _steps(straight, opt_a, grads, 0, 4)
    first, opt_b = _native(p0)
    _steps(first, opt_b, grads, 0, 3)
    saved = copy.deepcopy(opt_b.state_dict())
    assert all(float(st["step"]) == 3.0 and not st["step"].is_cuda for st in saved["state"].values()) and len(saved["ema"]) == len(SHAPES)
    again, opt_c = _native([q.detach().cpu().numpy() for q in first])
    opt_c.load_state_dict(saved)
    assert opt_c.steps_taken() == 3
    _steps(again, opt_c, grads, 3, 4)
    torch.cuda.synchronize()
    assert opt_c.steps_taken() == opt_a.steps_taken() == 4
    for a, c in zip(straight, again):
        assert torch.equal(a, c)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[a][k], opt_c.state[c][k])
    assert all(torch.equal(x, y) for x, y in zip(opt_a.shadows, opt_c.shadows))
    # a stock Adam takes the file as it is
    stock = torch.optim.Adam(again, lr=0.01)
    stock.load_state_dict(opt_c.state_dict())
    assert float(stock.state[again[0]]["step"]) == 4.0


class _Tiny(torch.nn.Module):
    """A stand-in network of element-wise torch operations: per-pixel class scores w^T x + b."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        self.w = torch.nn.Parameter(torch.randn(3, 4, generator=g))
        self.b = torch.nn.Parameter(torch.zeros(4))

    def forward(self, x):
        return (x[:, :, None] * self.w[None, :, :, None, None]).sum(1) + self.b[None, :, None, None]


def test_captured_step_equals_eager_steps():
    from robosat_amd.graph import TrainStepGraph
    from robosat_amd.optim import AdamW

    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(2, 3, 8, 8, generator=g).to(DEV), torch.randint(0, 4, (2, 8, 8), generator=g).to(DEV)) for _ in range(5)]
    hyper = dict(lr=0.05, weight_decay=0.1, clip_norm=0.05, ema=0.8, schedule={"kind": "cosine", "total_steps": 6, "warmup_steps": 2})
    results = []
    for enabled in (False, True):
        net = _Tiny().to(DEV).train()
        opt = AdamW(net.parameters(), **hyper)
        stepper = TrainStepGraph(net, torch.nn.CrossEntropyLoss(), opt, warmup=2, enabled=enabled)
        assert stepper.enabled == enabled
        for x, t in batches:
            stepper(x, t)
        torch.cuda.synchronize()
        assert stepper.captured == enabled
        results.append(([q.detach().clone() for q in net.parameters()], [s.clone() for s in opt.shadows], opt.steps_taken(),
                        float(opt._ctl.view(torch.float32)[4])))
    (p_e, s_e, n_e, coef_e), (p_g, s_g, n_g, coef_g) = results
    assert n_e == n_g == 5  # two eager steps and three replays moved the device's counter: step 5 ran with row 4
    assert coef_e == coef_g and coef_e < 1.0  # (clipping was active)
    assert all(torch.equal(a, b) for a, b in zip(p_e, p_g)) and all(torch.equal(a, b) for a, b in zip(s_e, s_g))
    # row 4's rate is not row 3's: a replay that froze the schedule at the captured step would not have matched
    opt = AdamW(_Tiny().parameters(), **hyper)
    assert opt.lr_at(4) < opt.lr_at(3) < opt.lr_at(2)


def test_two_ranks_hold_identical_parameters_and_shadows(tmp_path):
    from robosat_amd import launch

    env = dict(os.environ)
    env["ROBOSAT_DIST_BACKEND"] = "gloo"
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    rc = launch.spawn_ranks([sys.executable, os.path.join(ROOT, "tests", "optim_dp_worker.py"), str(tmp_path)], 2, env=env, timeout=600)
    assert rc == 0
    res = [json.load(open(os.path.join(str(tmp_path), "rank{}.json".format(r)))) for r in range(2)]
    print(res)
    for r in res:
        assert r["params_equal"] and r["shadows_equal"] and r["steps"] == 3, r
        assert r["coef"] < 1.0 and r["moved"] > 0.0 and r["shadow_differs_from_params"], r
    assert res[0]["coef"] == res[1]["coef"] and res[0]["loss_first"] != res[1]["loss_first"]  # different shards, one coefficient
