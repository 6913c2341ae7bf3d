"""The native optimiser of ``rs train``: AdamW with a learning-rate schedule, gradient clipping by the global norm and an
exponential moving average (EMA) of the weights, as ONE pass over the parameters (``csrc/optim.hip``).

``torch.optim.AdamW``'s update -- ``Adam``'s with ``weight_decay = 0`` -- per element, with the row ``(a_t, b_t, c_t, d_t)`` of step t:

    g^ = coef g                      (coef = min(1, clip_norm / (|g|_2 + 1e-6)) over ALL gradients; 1 without ``clip_norm``)
    m' = beta1 m + (1 - beta1) g^    v' = beta2 v + (1 - beta2) g^ g^
    p' = (decay ? c_t p : p) - a_t m' / (sqrt(v') b_t + eps)
    s' = d_t s + (1 - d_t) p'        (the EMA shadow, with ``ema``)

    a_t = lr_t / (1 - beta1^(t+1))   b_t = 1 / sqrt(1 - beta2^(t+1))   c_t = 1 - lr_t wd   d_t = min(ema, (1 + t) / (10 + t))

The rows are a table on the device, made here in float64 and rounded once (``schedule_table``); the step counter lives on the device
too, so a captured step (``[model] graph = true``) advances the schedule on every replay and no scalar crosses the bus per step.
Decay applies to tensors with more than one dimension (the convolution weights); BatchNorm's gamma / beta and biases get none.
"""

import contextlib
import math

import numpy as np
import torch

SCHEDULES = ("constant", "poly", "cosine")


def learning_rates(lr, total_steps, kind="constant", power=0.9, warmup_steps=0, lr_min=0.0):
    """float64 [T]: the rate of steps 0 .. T-1.  ``poly``: lr_min + (lr - lr_min) (1 - tau)^power, ``cosine``: lr_min + (lr - lr_min)
    (1 + cos(pi tau)) / 2, tau = (t - warmup) / (T - warmup) clamped to [0, 1]; both times (t + 1) / warmup while t < warmup."""

    if kind not in SCHEDULES:
        raise ValueError("schedule must be one of {}, got {!r}".format(", ".join(SCHEDULES), kind))
    T, w = int(total_steps), int(warmup_steps)
    if T <= 0 or w < 0:
        raise ValueError("total_steps must be > 0 and warmup_steps >= 0, got {} and {}".format(total_steps, warmup_steps))
    t = np.arange(T, dtype=np.float64)
    tau = np.clip((t - w) / max(1, T - w), 0.0, 1.0)
    if kind == "constant":
        rate = np.full(T, float(lr), dtype=np.float64)
    elif kind == "poly":
        rate = lr_min + (lr - lr_min) * (1.0 - tau) ** float(power)
    else:
        rate = lr_min + (lr - lr_min) * (1.0 + np.cos(np.pi * tau)) / 2.0
    if w > 0:
        rate = np.where(t < w, rate * (t + 1.0) / w, rate)
    return rate


def ema_decays(ema, total_steps):
    """float64 [T]: d_t = min(ema, (1 + t) / (10 + t)) -- an early shadow does not lag a fast-moving start; zeros without ``ema``."""

    t = np.arange(int(total_steps), dtype=np.float64)
    if ema is None:
        return np.zeros_like(t)
    return np.minimum(float(ema), (1.0 + t) / (10.0 + t))


def schedule_table(lr, total_steps, kind="constant", power=0.9, warmup_steps=0, lr_min=0.0, betas=(0.9, 0.999), wd=0.0, ema=None):
    """fp32 [T, 4] (a CPU tensor): row t = (a_t, b_t, c_t, d_t) of the module docstring, in float64 and rounded once."""

    rate = learning_rates(lr, total_steps, kind, power, warmup_steps, lr_min)
    t1 = np.arange(1, len(rate) + 1, dtype=np.float64)
    table = np.stack([rate / (1.0 - float(betas[0]) ** t1), 1.0 / np.sqrt(1.0 - float(betas[1]) ** t1), 1.0 - rate * float(wd),
                      ema_decays(ema, len(rate))], axis=1)
    return torch.from_numpy(table.astype(np.float32))


def saturation_steps(betas, ema):
    """Rows a table without a set length needs: past them both bias corrections are 1.0f and d_t = ema, so the last row is every
    later step's (``rs_optim_step`` uses row T-1 beyond the table)."""

    steps = 1
    for beta in betas:
        if beta > 0:
            steps = max(steps, int(math.ceil(math.log(2.0 ** -26) / math.log(beta))) + 1)
    if ema is not None:
        steps = max(steps, int(math.ceil((10.0 * ema - 1.0) / (1.0 - ema))) + 1)
    return steps


class AdamW(torch.optim.Optimizer):
    """``AdamW(params, lr, betas, eps, weight_decay, clip_norm, ema, schedule)``: see the module docstring.

    ``schedule``: None (a constant rate) or a dict ``{"kind", "total_steps", "power", "warmup_steps", "lr_min"}`` (``kind`` and
    ``total_steps`` required).  Per-parameter state under Adam's names (``step``, ``exp_avg``, ``exp_avg_sq``), so a stock ``Adam``
    resumes from this optimiser's ``state_dict()`` and the other way round; the shadows travel under the extra key ``ema``, in
    parameter order.  Parameters without a gradient are skipped; their shadow stays a copy.  The step counter is one int64 on the
    device (``steps_taken()`` reads it), every ``param_groups[i]["capturable"]`` is True: ``TrainStepGraph`` captures the step."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, clip_norm=None, ema=None, schedule=None):
        if not (isinstance(lr, (int, float)) and math.isfinite(lr) and lr >= 0):
            raise ValueError("lr must be a finite number >= 0, got {!r}".format(lr))
        if not all(0.0 <= b < 1.0 for b in betas) or len(betas) != 2:
            raise ValueError("betas must be two numbers in [0, 1), got {!r}".format(betas))
        if not (math.isfinite(eps) and eps >= 0) or not (math.isfinite(weight_decay) and weight_decay >= 0):
            raise ValueError("eps and weight_decay must be finite and >= 0, got {!r} and {!r}".format(eps, weight_decay))
        if clip_norm is not None and not (math.isfinite(clip_norm) and clip_norm > 0):
            raise ValueError("clip_norm must be a finite number > 0, got {!r}".format(clip_norm))
        if ema is not None and not 0.0 < ema < 1.0:
            raise ValueError("ema must lie in (0, 1), got {!r}".format(ema))
        # (the stock Adam keys, so that a stock Adam that loads this optimiser's param groups finds every key it reads)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=True, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.ema = None if ema is None else float(ema)
        schedule = dict(schedule or {"kind": "constant", "total_steps": saturation_steps(self.betas, self.ema)})
        self.schedule = {"kind": schedule["kind"], "total_steps": int(schedule["total_steps"]), "power": float(schedule.get("power", 0.9)),
                         "warmup_steps": int(schedule.get("warmup_steps", 0)), "lr_min": float(schedule.get("lr_min", 0.0))}
        self.rates = learning_rates(self.lr, **self.schedule)  # float64, for the log
        self._table_host = schedule_table(self.lr, betas=self.betas, wd=self.weight_decay, ema=self.ema, **self.schedule)
        self._table = self._ctl = self._workspace = None
        self._start = 0  # the step count a load_state_dict() asked for before the device buffers exist
        self._plan = None
        self.shadows = None
        if self.ema is not None:
            self.shadows = [p.detach().clone(memory_format=torch.preserve_format) for p in self._params()]

    def _params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _device_state(self, device):
        if self._ctl is None or self._ctl.device != device:
            self._table = self._table_host.to(device)
            self._ctl = torch.zeros(32, device=device, dtype=torch.uint8)
            self._ctl.view(torch.int64)[0:1].fill_(self._start)
            self._ctl.view(torch.float32)[4:5].fill_(1.0)
        return self._ctl

    def steps_taken(self):
        """The device's step counter (a host synchronisation)."""

        return self._start if self._ctl is None else int(self._ctl.view(torch.int64)[0].item())

    def lr_at(self, step):
        """The learning rate step ``step`` (0-based) is taken with."""

        return float(self.rates[min(max(int(step), 0), len(self.rates) - 1)])

    def grad_norm(self):
        """The global gradient norm of the last clipped step, as a device scalar (float64)."""

        return self._ctl.view(torch.float64)[1].sqrt()

    def _items(self):
        """The item array of this step.  The checked layout of (p, m, v, s) is kept between steps; only the gradients' addresses
        (a fresh arena per backward) are read again, each checked against its parameter's strides."""

        from . import ops

        params = [p for p in self._params() if p.grad is not None]
        if not params:
            return None
        key = tuple(id(p) for p in params)
        plan = self._plan
        if plan is not None and plan["key"] == key and all(p.data_ptr() == q for p, q in zip(params, plan["ptrs"])):
            items = plan["items"]
            for i, p in enumerate(params):
                g = p.grad
                if g.dtype != torch.float32 or g.device != p.device or g.stride() != plan["gstrides"][i]:
                    break
                items[i].g = g.data_ptr()
            else:
                return plan
        shadow = dict(zip((id(p) for p in self._params()), self.shadows)) if self.shadows is not None else {}
        entries = []
        for p in params:
            st = self.state[p]
            if "exp_avg" not in st:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            entries.append((p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], shadow.get(id(p)), p.dim() > 1))
        items, chunks = ops.optim_items(entries)
        # (`keep`: the tensors whose addresses the array holds, bar the gradients -- an arena must not outlive its step)
        self._plan = {"key": key, "ptrs": [p.data_ptr() for p in params], "gstrides": [p.grad.stride() for p in params],
                      "items": items, "chunks": chunks, "keep": [e[2:5] for e in entries], "device": params[0].device}
        return self._plan

    @torch.no_grad()
    def step(self, closure=None):
        from . import ops

        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._items()
        if plan is None:
            return loss
        device = plan["device"]
        ctl = self._device_state(device)
        if self.clip_norm is not None:
            need = ops.optim_workspace_bytes(plan["chunks"])
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
                self._workspace = torch.empty(need, device=device, dtype=torch.uint8)
            ops.optim_grad_norm(plan["items"], self.clip_norm, ctl, self._workspace)
        ops.optim_step(plan["items"], self._table, ctl, self.betas[0], self.betas[1], self.eps, self.clip_norm is not None)
        return loss

    def state_dict(self):
        """A stock Adam's layout (every ``step`` = the device counter, as a host tensor) plus ``ema``: the shadows in parameter order."""

        steps = float(self.steps_taken())
        for st in self.state.values():
            if "exp_avg" in st:
                st["step"] = torch.tensor(steps, dtype=torch.float32)
        state = super().state_dict()
        if self.shadows is not None:
            state["ema"] = list(self.shadows)
        return state

    def load_state_dict(self, state_dict):
        """From this optimiser's ``state_dict()`` or a stock Adam's: the moments as saved, the device counter from the saved ``step``,
        the shadows from ``ema`` where the file has them and from the current parameters where it does not.  The hyperparameters
        stay this instance's: they follow the run's configuration, not the file's."""

        state_dict = dict(state_dict)
        saved = state_dict.pop("ema", None)
        groups = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, mine in zip(self.param_groups, groups):
            g.update(mine)
        steps = max([int(round(float(st["step"]))) for st in self.state.values() if "step" in st] or [0])
        for p, st in self.state.items():
            if "step" in st:
                st["step"] = torch.tensor(float(steps), dtype=torch.float32)
            for name in ("exp_avg", "exp_avg_sq"):
                if name in st and (st[name].stride() != p.stride() or st[name].dtype != torch.float32):
                    st[name] = torch.empty_like(p, dtype=torch.float32, memory_format=torch.preserve_format).copy_(st[name])
        self._start = steps
        if self._ctl is not None:
            self._ctl.view(torch.int64)[0:1].fill_(steps)
        if self.shadows is not None:
            params = self._params()
            if saved is not None and len(saved) != len(params):
                raise ValueError("the checkpoint's ema holds {} tensors for {} parameters".format(len(saved), len(params)))
            with torch.no_grad():
                for i, (p, s) in enumerate(zip(params, self.shadows)):
                    s.copy_(p.detach() if saved is None else saved[i])
        self._plan = None

    def sync_ema(self):
        """Shadows = the parameters as they are now: after the weights were loaded or broadcast behind this optimiser's back."""

        if self.shadows is not None:
            with torch.no_grad():
                for p, s in zip(self._params(), self.shadows):
                    s.copy_(p.detach())

    @contextlib.contextmanager
    def swap_ema(self, net=None):
        """Inside the block the parameters hold the EMA weights and the shadows the raw ones; exchanged back on the way out.  The
        CONTENTS change places, not the tensors: every address a captured step or a derived-weight table holds stays what it was.
        ``net``: the module (or its ``.module``) whose ``invalidate_caches()`` is called on both edges -- the step writes through raw
        pointers, which the caches' keys (``_version``, ``data_ptr``) do not see."""

        if self.shadows is None:
            raise RuntimeError("swap_ema() needs ema")

        def exchange():
            with torch.no_grad():
                for p, s in zip(self._params(), self.shadows):
                    keep = p.detach().clone(memory_format=torch.preserve_format)
                    p.copy_(s)
                    s.copy_(keep)
            target = net
            while target is not None and not hasattr(target, "invalidate_caches") and hasattr(target, "module"):
                target = target.module
            if target is not None and hasattr(target, "invalidate_caches"):
                target.invalidate_caches()

        exchange()
        try:
            yield self
        finally:
            exchange()

    def describe(self):
        """What is on, for ``rs train``'s ``Optimizer:`` line."""

        s = self.schedule
        parts = ["AdamW (native step)", "weight_decay = {}".format(self.weight_decay)]
        if s["kind"] == "constant" and s["warmup_steps"] == 0:
            parts.append("constant rate")
        else:
            parts.append("schedule = {} over {} steps{}{}{}".format(
                s["kind"], s["total_steps"], ", power {}".format(s["power"]) if s["kind"] == "poly" else "",
                ", warm-up {} steps".format(s["warmup_steps"]) if s["warmup_steps"] else "",
                ", lr_min {}".format(s["lr_min"]) if s["lr_min"] else ""))
        parts.append("clip_norm = {}".format(self.clip_norm) if self.clip_norm is not None else "no clipping")
        parts.append("ema = {}".format(self.ema) if self.ema is not None else "no EMA")
        return ", ".join(parts)
