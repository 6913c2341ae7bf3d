"""The ``[opt] weight_decay / schedule / clip_norm / ema`` keys of ``rs train`` end to end on the MI355X, on tests/synth.py's tiny
dataset (8 training tiles of 128 x 128, batches of 2: four steps per epoch), two epochs: the ``Optimizer:`` line and the per-epoch
learning rates, the ``-ema.pth`` checkpoint and ``rs predict`` on it, ``--resume``, the untouched path without the keys, bad keys."""

import argparse
import os
import random
import re

import numpy as np
import pytest
import torch

import synth
from robosat_amd.config import load_config, save_config

pytestmark = pytest.mark.gpu
SIZE = 128
KEYS = {"weight_decay": 0.01, "schedule": "poly", "warmup_steps": 2, "lr_min": 1e-6, "clip_norm": 1.0, "ema": 0.9}


def _args(tmp, root, opt, name="pth", graph=False, checkpoint=None, resume=False):
    ckdir = os.path.join(tmp, name)
    model_toml, ds_toml = synth.write_configs(tmp, root, ckdir, loss="Lovasz", batch_size=2, image_size=SIZE, epochs=2, lr=1e-3)
    cfg = load_config(model_toml)
    if graph:
        cfg.setdefault("model", {})["graph"] = True
    cfg["opt"].update(opt)
    save_config(cfg, model_toml)
    return argparse.Namespace(model=model_toml, dataset=ds_toml, checkpoint=checkpoint, resume=resume, workers=0), ckdir


def _train(tmp, root, opt, **kw):
    from robosat_amd.tools import train as train_tool

    os.makedirs(tmp, exist_ok=True)
    args, ckdir = _args(tmp, root, opt, **kw)
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    train_tool.main(args)
    return args, ckdir, open(os.path.join(ckdir, "log")).read()


def _rates(log):
    """[(first, last, first step, last step)] of the log's ``Learning rate:`` lines."""

    found = re.findall(r"^Learning rate:\t (\S+) -> (\S+) \(steps (\d+) \.\. (\d+)\)$", log, flags=re.M)
    return [(float(a), float(b), int(c), int(d)) for a, b, c, d in found]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return synth.make_dataset(str(tmp_path_factory.mktemp("optimizer") / "ds"), n_train=8, n_val=4, size=SIZE)


@pytest.fixture(scope="module")
def straight(root, tmp_path_factory):
    """The two-epoch run with every key, shared by the tests that read its files."""

    return _train(str(tmp_path_factory.mktemp("straight")), root, KEYS)


def test_log_names_the_optimizer_and_the_falling_rates(straight):
    from robosat_amd.optim import learning_rates

    _, _, log = straight
    lines = [l for l in log.splitlines() if l.startswith("Optimizer:")]
    assert lines == ["Optimizer:\t AdamW (native step), weight_decay = 0.01, schedule = poly over 8 steps, power 0.9, warm-up 2 steps, "
                     "lr_min 1e-06, clip_norm = 1.0, ema = 0.9"], log
    rates = _rates(log)
    want = learning_rates(1e-3, 8, "poly", 0.9, 2, 1e-6)
    assert [(c, d) for _, _, c, d in rates] == [(1, 4), (5, 8)], log
    for (a, b, c, d) in rates:
        assert a == float("{:.6e}".format(want[c - 1])) and b == float("{:.6e}".format(want[d - 1]))
    assert rates[0][0] == 5e-4 and rates[0][1] > rates[1][0] > rates[1][1] > 1e-6  # warm-up, then falling under poly
    assert log.count("Validate loss:") == 2


def test_ema_checkpoint_differs_and_loads_in_rs_predict(straight, root, tmp_path):
    from robosat_amd.tools import predict as predict_tool

    args, ckdir, _ = straight
    raw = torch.load(os.path.join(ckdir, "checkpoint-00002-of-00002.pth"), map_location="cpu")
    ema = torch.load(os.path.join(ckdir, "checkpoint-00002-of-00002-ema.pth"), map_location="cpu")
    assert set(ema) == {"epoch", "state_dict"} and ema["epoch"] == 2 and set(raw) == {"epoch", "state_dict", "optimizer"}
    assert raw["state_dict"].keys() == ema["state_dict"].keys()
    w = "module.dec5.block.weight"
    assert not torch.equal(raw["state_dict"][w], ema["state_dict"][w])
    assert all(torch.isfinite(v).all() for v in ema["state_dict"].values() if v.is_floating_point())
    # the BatchNorm running statistics are the live ones; the shadow travels inside `optimizer` for --resume
    assert torch.equal(raw["state_dict"]["module.resnet.bn1.running_mean"], ema["state_dict"]["module.resnet.bn1.running_mean"])
    names = list(raw["state_dict"])
    params = [k for k in names if not ("running_" in k or "num_batches" in k)]
    assert len(raw["optimizer"]["ema"]) == len(params)
    index = params.index(w)
    assert torch.equal(raw["optimizer"]["ema"][index].cpu(), ema["state_dict"][w])
    assert all(float(st["step"]) == 8.0 for st in raw["optimizer"]["state"].values())
    # rs predict takes the file as any checkpoint (its tiles are 256 pixels at the least: two of the same synthetic kind)
    tiles = synth.make_dataset(str(tmp_path / "ds256"), n_train=1, n_val=2, size=256)
    probs = str(tmp_path / "probs")
    predict_tool.main(argparse.Namespace(batch_size=2, checkpoint=os.path.join(ckdir, "checkpoint-00002-of-00002-ema.pth"), overlap=32,
                                         tile_size=256, workers=0, tiles=os.path.join(tiles, "validation", "images"), probs=probs,
                                         model=args.model, dataset=args.dataset))
    assert sum(len(files) for _, _, files in os.walk(probs)) == 2


def test_resume_continues_the_schedule(straight, root, tmp_path):
    _, ckdir, log = straight
    _, _, resumed = _train(str(tmp_path), root, KEYS, checkpoint=os.path.join(ckdir, "checkpoint-00001-of-00002.pth"), resume=True)
    assert "Epoch: 1/2" not in resumed and "Epoch: 2/2" in resumed
    assert _rates(resumed) == _rates(log)[1:]  # the same first (and last) rate of epoch 2 as the straight run


def test_the_keys_under_a_captured_graph(root, tmp_path):
    _, ckdir, log = _train(str(tmp_path), root, KEYS, graph=True)
    assert [(c, d) for _, _, c, d in _rates(log)] == [(1, 4), (5, 8)], log  # the replays advanced the device's counter
    ck = torch.load(os.path.join(ckdir, "checkpoint-00002-of-00002.pth"), map_location="cpu")
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())


def test_without_the_keys_nothing_changes(root, tmp_path):
    _, ckdir, log = _train(str(tmp_path), root, {})
    assert "Optimizer:" not in log and "Learning rate:\t 1" not in log and _rates(log) == []
    assert not [f for f in os.listdir(ckdir) if f.endswith("-ema.pth")]
    state = torch.load(os.path.join(ckdir, "checkpoint-00002-of-00002.pth"), map_location="cpu")["optimizer"]
    # the layout a stock Adam writes: its keys, its groups, its per-parameter state
    stock = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    stock.param_groups[0]["params"][0].grad = torch.zeros(1)
    stock.step()
    want = stock.state_dict()
    assert set(state) == set(want) == {"state", "param_groups"}
    assert set(state["param_groups"][0]) == set(want["param_groups"][0])
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in state["state"].values()) and len(state["state"]) > 100


@pytest.mark.parametrize("opt, message", [
    ({"weight_decay": -1}, "Error: [opt] weight_decay must be a finite number >= 0, got -1"),
    ({"schedule": "step"}, "Error: [opt] schedule must be one of \"constant\", \"poly\", \"cosine\", got 'step'"),
    ({"schedule": "poly", "schedule_power": 0}, "Error: [opt] schedule_power must be a finite number > 0, got 0"),
    ({"schedule": "poly", "warmup_steps": 1.5}, "Error: [opt] warmup_steps must be an integer >= 0, got 1.5"),
    ({"schedule": "poly", "lr_min": 1.0}, "Error: [opt] lr_min must be a finite number in [0, lr], got 1.0"),
    ({"clip_norm": 0}, "Error: [opt] clip_norm must be a finite number > 0, got 0"),
    ({"ema": 1}, "Error: [opt] ema must be a number in (0, 1), got 1"),
    ({"warmup_steps": 3}, "Error: [opt] warmup_steps needs [opt] schedule (one of \"constant\", \"poly\", \"cosine\")"),
    ({"lr_min": 0.0}, "Error: [opt] lr_min needs [opt] schedule (one of \"constant\", \"poly\", \"cosine\")"),
    ({"schedule_power": 2.0}, "Error: [opt] schedule_power needs [opt] schedule (one of \"constant\", \"poly\", \"cosine\")"),
])
def test_a_bad_key_ends_rs_train(root, tmp_path, opt, message):
    from robosat_amd.tools import train as train_tool

    args, ckdir = _args(str(tmp_path), root, opt)
    with pytest.raises(SystemExit) as err:
        train_tool.main(args)
    assert str(err.value) == message
    assert not os.path.exists(ckdir)
