"""The model config's ``[opt] boundary_weight`` / ``boundary_sigma`` end to end on the MI355X: one epoch of ``rs train`` with
CrossEntropy and Focal on a small synthetic dataset (the pattern of tests/test_gpu_cli_ignore.py), through the default loaders and
through the decoded-tile cache with a zoom table, once as a captured graph and once with an ignore label; and the same runs without
the keys, which log no such line and another loss."""

import argparse
import os

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
FEEDS = ["default-loaders", "device-augment-zoom"]
LINE = "Boundary weight:\t w0 = 4.0, sigma = 2.0 px (reach 6 px)"


def _configs(tmp, root, loss, keys=True, feed="default-loaders", graph=False, ignore=False, sigma=2.0):
    ckdir = os.path.join(tmp, "pth-{}".format(loss))
    model_toml, ds_toml = synth.write_configs(tmp, root, ckdir, loss=loss, batch_size=2, image_size=SIZE, epochs=1)
    cfg = load_config(model_toml)
    if feed == "device-augment-zoom":
        cfg.setdefault("model", {})["device_augment"] = True
        cfg["augment"] = {"zoom": 1.5}
    if graph:
        cfg.setdefault("model", {})["graph"] = True
    if keys:
        cfg["opt"]["boundary_weight"] = 4.0
        if sigma is not None:
            cfg["opt"]["boundary_sigma"] = sigma
    save_config(cfg, model_toml)
    if ignore:
        ds = load_config(ds_toml)
        ds["common"]["ignore"] = 255
        save_config(ds, ds_toml)
    return argparse.Namespace(model=model_toml, dataset=ds_toml, checkpoint=None, resume=False, workers=0), ckdir


def _train(root, tmp, loss, **kw):
    """One epoch; returns (log text, logged training loss, logged validation loss)."""

    from robosat_amd.tools import train as train_tool

    os.makedirs(tmp, exist_ok=True)
    args, ckdir = _configs(tmp, root, loss, **kw)
    torch.manual_seed(0)  # (the random decoder: runs with and without the keys start from the same network)
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
    """The dataset (8 training tiles, 4 validation tiles of 128 x 128) and, per (loss, feed), the run WITHOUT the keys."""

    tmp = str(tmp_path_factory.mktemp("boundary"))
    root = synth.make_dataset(os.path.join(tmp, "ds"), n_train=8, n_val=4, size=SIZE)
    plain = {}
    for loss in LOSSES:
        for feed in FEEDS:
            plain[(loss, feed)] = _train(root, os.path.join(tmp, "plain-{}-{}".format(loss, feed)), loss, keys=False, feed=feed)
    return {"tmp": tmp, "root": root, "plain": plain}


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("feed", FEEDS)
def test_rs_train_one_epoch_with_the_keys(data, tmp_path, loss, feed):
    log, train_loss, val_loss = _train(data["root"], str(tmp_path), loss, feed=feed)
    assert [l for l in log.splitlines() if l.startswith("Boundary weight:")] == [LINE], log
    plain_log, plain_train, plain_val = data["plain"][(loss, feed)]
    # the weighted mean is another number than the plain one, in training and in validation (the criterion serves both)
    assert train_loss != plain_train and val_loss != plain_val, (train_loss, plain_train, val_loss, plain_val)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("feed", FEEDS)
def test_without_the_keys_the_log_has_no_such_line(data, loss, feed):
    log = data["plain"][(loss, feed)][0]
    assert "Boundary" not in log and "Loss function:\t {}".format(loss) in log


def test_only_the_weight_given_means_three_pixels(data, tmp_path):
    log, _, _ = _train(data["root"], str(tmp_path), "CrossEntropy", sigma=None)
    assert "Boundary weight:\t w0 = 4.0, sigma = 3.0 px (reach 9 px)" in log


def test_rs_train_as_a_captured_graph(data, tmp_path):
    """``[model] graph = true``: plane, loss and backward are captured after two eager batches and replayed (no host sync in them)."""

    log, train_loss, _ = _train(data["root"], str(tmp_path), "Focal", graph=True)
    assert LINE in log and train_loss != data["plain"][("Focal", "default-loaders")][1]


def test_rs_train_with_an_ignore_label(data, tmp_path):
    """``[common] ignore = 255`` on labels whose left third is 255, one of them everywhere: both keys at once."""

    root = synth.make_dataset(str(tmp_path / "ds"), n_train=8, n_val=4, size=SIZE)
    for split in ("training", "validation"):
        for k, (_, path) in enumerate(sorted(tiles_from_slippy_map(os.path.join(root, split, "labels")), key=lambda e: e[1])):
            with Image.open(path) as image:
                label = np.array(image, dtype=np.uint8)
            label[:, : SIZE // 3] = 255
            if k == 0:
                label[:] = 255
            out = Image.fromarray(label, mode="P")
            out.putpalette([0, 0, 0, 250, 0, 0] + [0] * (254 * 3))
            out.save(path)
    log, _, _ = _train(root, str(tmp_path / "run"), "CrossEntropy", ignore=True)
    assert LINE in log and "Ignore label:\t 255" in log
