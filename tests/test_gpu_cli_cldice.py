"""``[opt] cldice`` end to end on the MI355X, on the small synthetic dataset of tests/test_gpu_cli_tversky.py: one epoch of ``rs train``
runs, logs the ``clDice:`` line and writes a finite checkpoint; once as a captured graph; the logged loss is ``(1 - a) x base + a x
term``; a bad key ends the tool with ``Error: [opt] cldice...``; and without the key no wrapper is built.

How the mix is shown: with ``lr = 0`` the optimizer leaves every weight where it is, so runs with different losses end on the same
network, bit for bit (asserted on the checkpoints), and the logged epoch means are linear in the per-batch terms.  A plain CrossEntropy
run gives CE, a run with a = 0.75 gives the term T = (L_0.75 - 0.25 CE) / 0.75, and the run with a = 0.5 must log 0.5 CE + 0.5 T.  Each
logged value is rounded to 4 decimals (5e-5), so the bar is 5e-5 x (1 + 0.5 + 0.5 x (1 + 0.25) / 0.75) = 1.17e-4."""

import argparse
import os
import random

import numpy as np
import pytest
import torch

import synth
from robosat_amd.config import load_config, save_config

pytestmark = pytest.mark.gpu
SIZE = 128


def _configs(tmp, root, loss, opt, graph=False, lr=1e-4):
    ckdir = os.path.join(tmp, "pth-{}".format(loss))
    model_toml, ds_toml = synth.write_configs(tmp, root, ckdir, loss=loss, batch_size=2, image_size=SIZE, epochs=1, lr=lr)
    cfg = load_config(model_toml)
    if graph:
        cfg.setdefault("model", {})["graph"] = True
    cfg["opt"].update(opt)
    save_config(cfg, model_toml)
    return argparse.Namespace(model=model_toml, dataset=ds_toml, checkpoint=None, resume=False, workers=0), ckdir


def _train(root, tmp, loss, opt, **kw):
    """One epoch from fixed seeds; returns (log text, {"Train" | "Valid": the loss as the log prints it}, the checkpoint's state_dict)."""

    from robosat_amd.tools import train as train_tool

    os.makedirs(tmp, exist_ok=True)
    args, ckdir = _configs(tmp, root, loss, opt, **kw)
    torch.manual_seed(0)  # the random decoder
    random.seed(0)  # the flips and quarter turns of the training tiles
    np.random.seed(0)
    train_tool.main(args)
    log = open(os.path.join(ckdir, "log")).read()
    values = {}
    for line in log.splitlines():
        if line.startswith(("Train    loss:", "Validate loss:")):
            values[line[:5]] = line.split("loss:")[1].split(",")[0].strip()
            assert np.isfinite(float(values[line[:5]])) and float(values[line[:5]]) >= 0.0, line
    assert set(values) == {"Train", "Valid"}, log
    ck = torch.load(os.path.join(ckdir, "checkpoint-00001-of-00001.pth"), map_location="cpu")
    assert int(ck["state_dict"]["module.resnet.bn1.num_batches_tracked"]) == 4
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())
    return log, values, ck["state_dict"]


def _same_network(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return synth.make_dataset(str(tmp_path_factory.mktemp("cldice") / "ds"), n_train=8, n_val=4, size=SIZE)


def test_rs_train_one_epoch(root, tmp_path):
    log, values, _ = _train(root, str(tmp_path / "t"), "CrossEntropy", {"cldice": 0.3, "cldice_iters": 3})
    line = "clDice:\t a = 0.3, iters = 3, smooth = 1.0, classes all: loss = 0.7 x CrossEntropy + 0.3 x clDice"
    assert [l for l in log.splitlines() if l.startswith("clDice:")] == [line], log
    assert "Loss function:\t CrossEntropy" in log
    assert 0.0 < float(values["Train"]) and 0.0 < float(values["Valid"])


def test_rs_train_as_a_captured_graph(root, tmp_path):
    log, values, _ = _train(root, str(tmp_path / "g"), "CrossEntropy", {"cldice": 0.3, "cldice_iters": 3}, graph=True)
    assert "clDice:\t a = 0.3, iters = 3" in log
    assert 0.0 < float(values["Train"]) and 0.0 < float(values["Valid"])


def test_the_logged_loss_is_the_mix_of_base_and_term(root, tmp_path, monkeypatch):
    """Also: ``rs train`` hands its criterion to ``TrainStepGraph`` -- with the key a ``ClDiceLoss2d`` around the criterion of
    ``[opt] loss``, without it the plain criterion as before, no wrapper."""

    import robosat_amd.graph as graph_module
    from robosat_amd.losses import ClDiceLoss2d, CrossEntropyLoss2d

    seen = []
    original = graph_module.TrainStepGraph

    def recording(net, criterion, optimizer, **kw):
        seen.append(criterion)
        return original(net, criterion, optimizer, **kw)

    monkeypatch.setattr(graph_module, "TrainStepGraph", recording)
    plain_log, pixel, state_a = _train(root, str(tmp_path / "a"), "CrossEntropy", {}, lr=0.0)
    _, other, state_b = _train(root, str(tmp_path / "b"), "CrossEntropy", {"cldice": 0.75, "cldice_iters": 3}, lr=0.0)
    _, mixed, state_c = _train(root, str(tmp_path / "c"), "CrossEntropy", {"cldice": 0.5, "cldice_iters": 3}, lr=0.0)
    assert "clDice:" not in plain_log
    assert type(seen[0]) is CrossEntropyLoss2d  # (without the key: the criterion object as before)
    assert type(seen[2]) is ClDiceLoss2d and type(seen[2].base) is CrossEntropyLoss2d and seen[2].iters == 3
    assert _same_network(state_a, state_b) and _same_network(state_a, state_c)
    bar = 5e-5 * (1 + 0.5 + 0.5 * (1 + 0.25) / 0.75)
    for key in ("Train", "Valid"):
        ce = float(pixel[key])
        term = (float(other[key]) - 0.25 * ce) / 0.75
        print(key, pixel[key], other[key], mixed[key], term)
        assert abs(float(mixed[key]) - (0.5 * ce + 0.5 * term)) <= bar, (key, pixel, other, mixed)
        assert ce > 1e-3 and 1e-3 < term <= 1.0 + 1e-3  # (both terms are there to be mixed; the term is a Dice-like score)


@pytest.mark.parametrize("opt, message", [
    ({"cldice": 1.0}, "cldice must be a number with 0 < a < 1"),
    ({"cldice": 0.3, "cldice_iters": 0}, "cldice_iters must be an integer in 1..64"),
    ({"cldice": 0.3, "cldice_smooth": -1.0}, "cldice_smooth must be a finite number >= 0"),
    ({"cldice": 0.3, "cldice_classes": ["river"]}, "cldice_classes: 'river' is no non-background class"),
    ({"cldice_iters": 3}, "cldice_iters needs [opt] cldice"),
], ids=["a-bad-weight", "bad-iters", "a-bad-smooth", "an-unknown-class", "a-key-without-cldice"])
def test_a_bad_key_ends_rs_train(root, tmp_path, opt, message):
    from robosat_amd.tools import train as train_tool

    args, ckdir = _configs(str(tmp_path), root, "CrossEntropy", opt)
    with pytest.raises(SystemExit) as err:
        train_tool.main(args)
    assert str(err.value).startswith("Error: [opt] " + message), str(err.value)
    assert not os.path.exists(ckdir)
