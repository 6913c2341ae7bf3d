"""The model config's ``[opt] hard_fraction`` / ``hard_below`` end to end on the MI355X, on the small synthetic dataset of
tests/test_gpu_cli_boundary.py: one epoch of ``rs train`` with the keys runs, logs the ``Hard pixels:`` line and writes a checkpoint;
the validation loss it logs is the UNMINED loss of that checkpoint; once as a captured graph together with the boundary weight; and a
bad key ends the tool with ``Error: [opt] hard_...``.

How "the unmined loss of that checkpoint" is shown: with ``lr = 0`` the optimizer leaves every weight where it is, and the BatchNorm
statistics depend on the seeded batches alone, so a run with the keys and a run without them end on the same network, bit for bit
(asserted on the two checkpoints).  Their logged validation losses must then be the same text, while their training losses differ."""

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
    return synth.make_dataset(str(tmp_path_factory.mktemp("hard") / "ds"), n_train=8, n_val=4, size=SIZE)


def test_rs_train_one_epoch_with_the_keys(root, tmp_path):
    log, values, _ = _train(root, str(tmp_path / "hard"), "CrossEntropy", {"hard_fraction": 0.25})
    line = "Hard pixels:\t the hardest 0.25 of every image's valid pixels (training only; validation loss unmined)"
    assert [l for l in log.splitlines() if l.startswith("Hard pixels:")] == [line], log
    plain_log, _, _ = _train(root, str(tmp_path / "plain"), "CrossEntropy", {})
    assert "Hard pixels" not in plain_log and "Loss function:\t CrossEntropy" in plain_log


@pytest.mark.parametrize("loss, opt, graph", [
    ("Focal", {"hard_fraction": 0.1, "hard_below": 0.3}, False),
    ("CrossEntropy", {"hard_fraction": 0.25, "boundary_weight": 4.0, "boundary_sigma": 2.0}, True),
], ids=["focal-with-a-bound", "graph-with-the-boundary-weight"])
def test_the_logged_validation_loss_is_the_unmined_one(root, tmp_path, loss, opt, graph):
    """``lr = 0``: the run with the keys and the run without them end on the same network; the second case captures keys, selection,
    plane, loss and backward into the step's graph (``[model] graph = true``) with the boundary plane as the base."""

    log, mined, state = _train(root, str(tmp_path / "hard"), loss, opt, graph=graph, lr=0.0)
    assert "Hard pixels:\t the hardest {} of".format(opt["hard_fraction"]) in log
    assert ("p(true class) < 0.3" in log) == ("hard_below" in opt) and ("Boundary weight:" in log) == ("boundary_weight" in opt)
    rest = {k: v for k, v in opt.items() if not k.startswith("hard_")}
    plain_log, plain, plain_state = _train(root, str(tmp_path / "plain"), loss, rest, graph=graph, lr=0.0)
    assert "Hard pixels" not in plain_log
    assert _same_network(state, plain_state)
    assert mined["Valid"] == plain["Valid"], (mined, plain)
    assert float(mined["Train"]) > float(plain["Train"]), (mined, plain)  # the mean over the hardest pixels of the same batches


@pytest.mark.parametrize("opt, key", [({"hard_fraction": 1.5}, "hard_fraction"), ({"hard_below": 0.3}, "hard_below")])
def test_a_bad_key_ends_rs_train(root, tmp_path, opt, key):
    from robosat_amd.tools import train as train_tool

    args, ckdir = _configs(str(tmp_path), root, "CrossEntropy", opt)
    with pytest.raises(SystemExit) as err:
        train_tool.main(args)
    assert str(err.value).startswith("Error: [opt] " + key), str(err.value)
    assert not os.path.exists(ckdir)
