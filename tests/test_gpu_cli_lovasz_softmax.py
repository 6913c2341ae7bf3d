"""``rs train`` with ``[opt] loss = "LovaszSoftmax"`` end to end on a synthetic 3-class dataset: one process, two
data-parallel ranks (per image), the refusal of the flattened form over two ranks, and a bad ``lovasz_classes``."""

import argparse
import os
import random
import re
import subprocess
import sys

import pytest
import torch

import synth
from robosat_amd.config import load_config, save_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = r"^(Train   |Validate) loss: \d+\.\d{4}, mIoU: (\d\.\d{3}|nan), parking IoU: (\d\.\d{3}|nan), MCC: (-?\d\.\d{3}|nan)$"


def _setup(tmp, batch_size=2, **opt):
    ds_root = synth.make_dataset(os.path.join(tmp, "ds"), n_train=8, n_val=4, size=256, classes=3)
    ckdir = os.path.join(tmp, "pth")
    model_toml, ds_toml = synth.write_configs(tmp, ds_root, ckdir, loss="LovaszSoftmax", batch_size=batch_size, image_size=256,
                                              epochs=1, classes=3)
    model = load_config(model_toml)
    model["opt"].update(opt)
    save_config(model, model_toml)
    ds = load_config(ds_toml)
    del ds["weights"]  # (the loss needs none)
    save_config(ds, ds_toml)
    return model_toml, ds_toml, ckdir


def _rs(args, env_extra, cwd):
    env = dict(os.environ)
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "-m", "robosat_amd.tools"] + args, env=env, cwd=cwd, capture_output=True, text=True,
                          timeout=900)


def _check_artifacts(ckdir, batches):
    log = open(os.path.join(ckdir, "log")).read().splitlines()
    assert "Loss function:\t LovaszSoftmax" in log
    assert sum(bool(re.match(LINE, l)) for l in log) == 2, log
    ck = torch.load(os.path.join(ckdir, "checkpoint-00001-of-00001.pth"), map_location="cpu")
    assert ck["epoch"] == 1 and int(ck["state_dict"]["module.resnet.bn1.num_batches_tracked"]) == batches
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())


@pytest.mark.parametrize("opt", [{}, {"lovasz_per_image": False, "lovasz_classes": "all"}], ids=["default", "flat-all"])
def test_rs_train_one_process(tmp_path, opt):
    from robosat_amd.tools import train as train_tool

    model_toml, ds_toml, ckdir = _setup(str(tmp_path), **opt)
    random.seed(0)
    torch.manual_seed(0)
    train_tool.main(argparse.Namespace(model=model_toml, dataset=ds_toml, checkpoint=None, resume=False, workers=0))
    _check_artifacts(ckdir, 4)  # 8 tiles / batch 2


def test_rs_train_two_ranks_per_image_and_the_flat_refusal(tmp_path):
    two = {"ROBOSAT_GPUS": "2", "ROBOSAT_DIST_BACKEND": "gloo"}
    tmp = str(tmp_path / "img")
    os.makedirs(tmp)
    model_toml, ds_toml, ckdir = _setup(tmp, batch_size=4)
    r = _rs(["train", "--model", model_toml, "--dataset", ds_toml], two, tmp)
    assert r.returncode == 0, r.stdout + r.stderr
    _check_artifacts(ckdir, 2)  # 8 tiles / GLOBAL batch 4

    tmp = str(tmp_path / "flat")
    os.makedirs(tmp)
    model_toml, ds_toml, ckdir = _setup(tmp, batch_size=4, lovasz_per_image=False)
    r = _rs(["train", "--model", model_toml, "--dataset", ds_toml], two, tmp)
    assert r.returncode != 0
    assert "lovasz_per_image = false needs one sort over the global batch" in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(os.path.join(ckdir, "checkpoint-00001-of-00001.pth"))


def test_rs_train_rejects_a_bad_lovasz_classes(tmp_path):
    tmp = str(tmp_path)
    model_toml, ds_toml, ckdir = _setup(tmp, lovasz_classes="some")
    r = _rs(["train", "--model", model_toml, "--dataset", ds_toml], {"ROBOSAT_GPUS": "1"}, tmp)
    assert r.returncode != 0
    assert "Error: [opt] lovasz_classes must be" in r.stderr, r.stdout + r.stderr
