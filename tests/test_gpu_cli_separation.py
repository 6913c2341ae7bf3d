"""The model config's ``[opt] separation_weight`` / ``separation_sigma`` end to end on the MI355X: one epoch of ``rs train`` with
CrossEntropy and Focal on a small synthetic dataset (the pattern of tests/test_gpu_cli_boundary.py) whose label tiles all hold two
squares three pixels apart; the same run without the keys, twice, which logs no such line, another loss, and the same loss both times;
a run with both weights as a captured graph; and a bad key, which ends ``rs train`` before the device is asked for."""

import argparse
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import synth
from robosat_amd.config import load_config, save_config
from robosat_amd.tiles import tiles_from_slippy_map

pytestmark = pytest.mark.gpu
SIZE = 128
LOSSES = ["CrossEntropy", "Focal"]
LINE = "Separation weight:\t ws = 10.0, sigma = 2.0 px (reach 6 px)"


def _configs(tmp, root, loss, keys=True, graph=False, sigma=2.0, boundary=False, extra=None):
    ckdir = os.path.join(tmp, "pth-{}".format(loss))
    model_toml, ds_toml = synth.write_configs(tmp, root, ckdir, loss=loss, batch_size=2, image_size=SIZE, epochs=1)
    cfg = load_config(model_toml)
    if graph:
        cfg.setdefault("model", {})["graph"] = True
    if keys:
        cfg["opt"]["separation_weight"] = 10.0
        if sigma is not None:
            cfg["opt"]["separation_sigma"] = sigma
    if boundary:
        cfg["opt"]["boundary_weight"] = 4.0
    cfg["opt"].update(extra or {})
    save_config(cfg, model_toml)
    return argparse.Namespace(model=model_toml, dataset=ds_toml, checkpoint=None, resume=False, workers=0), ckdir


def _train(root, tmp, loss, **kw):
    """One epoch; returns (log text, logged training loss, logged validation loss)."""

    from robosat_amd.tools import train as train_tool

    os.makedirs(tmp, exist_ok=True)
    args, ckdir = _configs(tmp, root, loss, **kw)
    torch.manual_seed(0)  # (the random decoder: runs with and without the keys start from the same network)
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
    ck = torch.load(os.path.join(ckdir, "checkpoint-00001-of-00001.pth"), map_location="cpu")
    assert int(ck["state_dict"]["module.resnet.bn1.num_batches_tracked"]) == 4
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())
    return log, values["Train"], values["Valid"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The dataset (8 training tiles, 4 validation tiles of 128 x 128, two squares three pixels apart painted into every label, so
    that every tile has a gap to weigh) and, per loss, the run WITHOUT the keys."""

    tmp = str(tmp_path_factory.mktemp("separation"))
    root = synth.make_dataset(os.path.join(tmp, "ds"), n_train=8, n_val=4, size=SIZE)
    for split in ("training", "validation"):
        for _, path in tiles_from_slippy_map(os.path.join(root, split, "labels")):
            with Image.open(path) as image:
                label = np.array(image, dtype=np.uint8)
            label[2:36, 2:36] = 0
            label[4:14, 4:14] = 1
            label[4:14, 17:27] = 1
            out = Image.fromarray(label, mode="P")
            out.putpalette([0, 0, 0, 250, 0, 0] + [0] * (254 * 3))
            out.save(path)
    plain = {loss: _train(root, os.path.join(tmp, "plain-{}".format(loss)), loss, keys=False) for loss in LOSSES}
    return {"tmp": tmp, "root": root, "plain": plain}


@pytest.mark.parametrize("loss", LOSSES)
def test_rs_train_one_epoch_with_the_keys(data, tmp_path, loss):
    log, train_loss, val_loss = _train(data["root"], str(tmp_path), loss)
    assert [l for l in log.splitlines() if l.startswith("Separation weight:")] == [LINE], log
    plain_log, plain_train, plain_val = data["plain"][loss]
    # the weighted mean is another number than the plain one, in training and in validation (the criterion serves both)
    assert train_loss != plain_train and val_loss != plain_val, (train_loss, plain_train, val_loss, plain_val)


def test_without_the_keys_the_run_is_the_one_it_was(data, tmp_path):
    """No such line in the log, and a second run on the same seed with the keys absent logs the same loss values to the digit."""

    log, train_loss, val_loss = data["plain"]["CrossEntropy"]
    assert "Separation" not in log and "Loss function:\t CrossEntropy" in log
    again, train_again, val_again = _train(data["root"], str(tmp_path), "CrossEntropy", keys=False)
    assert (train_again, val_again) == (train_loss, val_loss)
    pick = lambda text: [l for l in text.splitlines() if "loss:" in l]  # noqa: E731
    assert pick(again) == pick(log)


def test_only_the_weight_given_means_five_pixels(data, tmp_path):
    log, _, _ = _train(data["root"], str(tmp_path), "CrossEntropy", sigma=None)
    assert "Separation weight:\t ws = 10.0, sigma = 5.0 px (reach 15 px)" in log


def test_rs_train_with_both_weights_as_a_captured_graph(data, tmp_path):
    """``[model] graph = true``: both planes, loss and backward are captured after two eager batches and replayed."""

    log, train_loss, _ = _train(data["root"], str(tmp_path), "Focal", graph=True, boundary=True)
    assert LINE in log and "Boundary weight:" in log and train_loss != data["plain"]["Focal"][1]


@pytest.mark.parametrize("extra, key", [({"separation_sigma": 10.7}, "separation_sigma"), ({"separation_weight": -1.0}, "separation_weight"),
                                        ({"loss": "Lovasz"}, "separation_weight")])
def test_a_bad_key_ends_rs_train_before_the_device_is_asked_for(data, tmp_path, monkeypatch, extra, key):
    from robosat_amd.tools import train as train_tool

    args, ckdir = _configs(str(tmp_path), data["root"], "CrossEntropy", extra=extra)

    def no_device(*a, **k):
        raise AssertionError("rs train asked for the device before it refused the key")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(SystemExit) as err:
        train_tool.main(args)
    assert str(err.value).startswith("Error: [opt] " + key), str(err.value)
    assert err.value.code != 0 and not os.path.exists(ckdir)
