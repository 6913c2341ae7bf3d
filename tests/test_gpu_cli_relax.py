"""The model config's ``[opt] relax`` end to end on the MI355X: one epoch of ``rs train`` with CrossEntropy and Focal on a small synthetic
dataset (the pattern of tests/test_gpu_cli_separation.py), which logs the ``Label relaxation:`` line and another training loss and
writes a checkpoint that ``rs predict`` loads; the same run without the key, twice, which logs no such line and the same loss both
times; a run with the boundary weight beside it as a captured graph; and a bad key, which ends ``rs train`` before the device is
asked for."""

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
LOSSES = ["CrossEntropy", "Focal"]
LINE = "Label relaxation:\t R = 2 px: near an outline every class within a 5 x 5 window is accepted (training only; validation loss strict)"


def _configs(tmp, root, loss, keys=True, graph=False, boundary=False, extra=None):
    ckdir = os.path.join(tmp, "pth-{}".format(loss))
    model_toml, ds_toml = synth.write_configs(tmp, root, ckdir, loss=loss, batch_size=2, image_size=SIZE, epochs=1)
    cfg = load_config(model_toml)
    if graph:
        cfg.setdefault("model", {})["graph"] = True
    if keys:
        cfg["opt"]["relax"] = 2
    if boundary:
        cfg["opt"]["boundary_weight"] = 4.0
    cfg["opt"].update(extra or {})
    save_config(cfg, model_toml)
    return argparse.Namespace(model=model_toml, dataset=ds_toml, checkpoint=None, resume=False, workers=0), ckdir


def _train(root, tmp, loss, **kw):
    """One epoch; returns (log text, logged training loss, logged validation loss, checkpoint path)."""

    from robosat_amd.tools import train as train_tool

    os.makedirs(tmp, exist_ok=True)
    args, ckdir = _configs(tmp, root, loss, **kw)
    torch.manual_seed(0)  # (the random decoder: runs with and without the key start from the same network)
    random.seed(0)  # (the flips and quarter turns of the training tiles: two runs see the same batches)
    np.random.seed(0)
    train_tool.main(args)
    log = open(os.path.join(ckdir, "log")).read()
    values = {}
    for line in log.splitlines():
        if line.startswith(("Train    loss:", "Validate loss:")):
            values[line[:5]] = float(line.split("loss:")[1].split(",")[0])
            assert np.isfinite(values[line[:5]]) and values[line[:5]] >= 0.0, line
    assert set(values) == {"Train", "Valid"}, log
    path = os.path.join(ckdir, "checkpoint-00001-of-00001.pth")
    ck = torch.load(path, map_location="cpu")
    assert int(ck["state_dict"]["module.resnet.bn1.num_batches_tracked"]) == 4
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())
    return log, values["Train"], values["Valid"], path


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The dataset (8 training tiles, 4 validation tiles of 128 x 128) and, per loss, the run WITHOUT the key."""

    tmp = str(tmp_path_factory.mktemp("relax"))
    root = synth.make_dataset(os.path.join(tmp, "ds"), n_train=8, n_val=4, size=SIZE)
    plain = {loss: _train(root, os.path.join(tmp, "plain-{}".format(loss)), loss, keys=False) for loss in LOSSES}
    return {"tmp": tmp, "root": root, "plain": plain}


@pytest.mark.parametrize("loss", LOSSES)
def test_rs_train_one_epoch_with_the_key(data, tmp_path, loss):
    """The line is logged once, the training loss is another number than the strict run's, and ``rs predict`` loads the checkpoint."""

    from robosat_amd.tools import predict as predict_tool

    log, train_loss, val_loss, path = _train(data["root"], str(tmp_path), loss)
    assert [l for l in log.splitlines() if l.startswith("Label relaxation:")] == [LINE], log
    _, plain_train, _, _ = data["plain"][loss]
    assert train_loss != plain_train, (train_loss, plain_train)
    # rs predict takes the file as any checkpoint (its tiles are 256 pixels at the least: two of the same synthetic kind)
    args, _ = _configs(str(tmp_path), data["root"], loss)
    tiles = synth.make_dataset(str(tmp_path / "ds256"), n_train=1, n_val=2, size=256)
    probs = str(tmp_path / "probs")
    predict_tool.main(argparse.Namespace(batch_size=2, checkpoint=path, overlap=32, tile_size=256, workers=0,
                                         tiles=os.path.join(tiles, "validation", "images"), probs=probs, model=args.model, dataset=args.dataset))
    assert sum(len(files) for _, _, files in os.walk(probs)) == 2


def test_without_the_key_the_run_is_the_one_it_was(data, tmp_path):
    """No such line in the log, and a second run on the same seed with the key absent logs the same loss values to the digit."""

    log, train_loss, val_loss, _ = data["plain"]["CrossEntropy"]
    assert "relaxation" not in log and "Loss function:\t CrossEntropy" in log
    again, train_again, val_again, _ = _train(data["root"], str(tmp_path), "CrossEntropy", keys=False)
    assert (train_again, val_again) == (train_loss, val_loss)
    pick = lambda text: [l for l in text.splitlines() if "loss:" in l]  # noqa: E731
    assert pick(again) == pick(log)


def test_rs_train_relaxed_with_the_boundary_weight_as_a_captured_graph(data, tmp_path):
    """``[model] graph = true``: the boundary plane, the set plane, loss and backward are captured after two eager batches and replayed."""

    log, train_loss, _, _ = _train(data["root"], str(tmp_path), "Focal", graph=True, boundary=True)
    assert LINE in log and "Boundary weight:" in log and train_loss != data["plain"]["Focal"][1]


@pytest.mark.parametrize("extra, prefix", [({"relax": 17}, "Error: [opt] relax must be"), ({"relax": 2.0}, "Error: [opt] relax must be"),
                                           ({"relax": True}, "Error: [opt] relax must be"),
                                           ({"loss": "Lovasz"}, "Error: [opt] relax relaxes"),
                                           ({"hard_fraction": 0.25}, "Error: [opt] relax cannot stand beside [opt] hard_fraction")])
def test_a_bad_key_ends_rs_train_before_the_device_is_asked_for(data, tmp_path, monkeypatch, extra, prefix):
    from robosat_amd.tools import train as train_tool

    args, ckdir = _configs(str(tmp_path), data["root"], "CrossEntropy", extra=extra)

    def no_device(*a, **k):
        raise AssertionError("rs train asked for the device before it refused the key")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(SystemExit) as err:
        train_tool.main(args)
    assert str(err.value).startswith(prefix), str(err.value)
    assert err.value.code != 0 and not os.path.exists(ckdir)
