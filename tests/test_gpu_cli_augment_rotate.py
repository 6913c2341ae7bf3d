"""``rs train`` with ``[augment] rotate`` end to end: one epoch on a synthetic dataset through the default loaders and through the
decoded-tile cache (``[model] device_augment``), the ``Augmentation:`` line of the log, and a bad angle that ends the run first."""

import argparse
import os

import pytest
import torch

import synth
from robosat_amd.config import load_config, save_config

pytestmark = pytest.mark.gpu
TABLE = {"zoom": 1.5, "brightness": [0.8, 1.2], "contrast": [0.8, 1.2], "saturation": [0.8, 1.2], "gamma": [0.8, 1.25]}


def _setup(tmp, table, device_augment):
    ds_root = synth.make_dataset(os.path.join(tmp, "ds"), n_train=8, n_val=4, size=256)
    ckdir = os.path.join(tmp, "pth")
    model_toml, ds_toml = synth.write_configs(tmp, ds_root, ckdir, loss="Lovasz", batch_size=2, image_size=256, epochs=1)
    cfg = load_config(model_toml)
    if device_augment:
        cfg.setdefault("model", {})["device_augment"] = True
    cfg["augment"] = table
    save_config(cfg, model_toml)
    return argparse.Namespace(model=model_toml, dataset=ds_toml, checkpoint=None, resume=False, workers=0), ckdir


@pytest.mark.parametrize("device_augment", [False, True], ids=["default-loaders", "device-augment"])
def test_rs_train_with_a_rotating_augment_table(tmp_path, device_augment):
    from robosat_amd.tools import train as train_tool

    args, ckdir = _setup(str(tmp_path), dict(TABLE, rotate=180), device_augment)
    train_tool.main(args)
    log = open(os.path.join(ckdir, "log")).read()
    assert "Train    loss:" in log and "Validate loss:" in log
    lines = [l for l in log.splitlines() if l.startswith("Augmentation:\t ")]
    assert len(lines) == 1 and "zoom <= 1.5" in lines[0] and lines[0].endswith("rotate <= 180 deg"), log
    ck = torch.load(os.path.join(ckdir, "checkpoint-00001-of-00001.pth"), map_location="cpu")
    assert int(ck["state_dict"]["module.resnet.bn1.num_batches_tracked"]) == 4
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())


def test_rs_train_ends_on_a_bad_angle_before_any_training(tmp_path):
    from robosat_amd.tools import train as train_tool

    args, ckdir = _setup(str(tmp_path), dict(TABLE, rotate=270), False)
    with pytest.raises(SystemExit) as err:
        train_tool.main(args)
    assert str(err.value).startswith("Error: [augment] rotate ")
    assert not os.path.exists(ckdir)  # (not even the checkpoint directory: nothing had started)
