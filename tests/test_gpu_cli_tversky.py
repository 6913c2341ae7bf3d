"""``[opt] loss = "Tversky"`` end to end on the MI355X, on the small synthetic dataset of tests/test_gpu_cli_hard_pixels.py: one epoch of
``rs train`` runs, logs the ``Tversky:`` line and writes a finite checkpoint; once as a captured graph; the fused loss is the sum of its
two terms; and a bad key ends the tool with ``Error: [opt] ...``.

How "the sum of its two terms" is shown: with ``lr = 0`` the optimizer leaves every weight where it is, and the BatchNorm statistics
depend on the seeded batches alone, so runs with different losses end on the same network, bit for bit (asserted on the
checkpoints).  The per-batch losses add linearly -- Tversky with ``tversky_ce = 1`` is Tversky with ``tversky_ce = 0`` plus CrossEntropy on every
batch -- so the logged epoch means add too, up to the three roundings to 4 decimals of the log: 1.5e-4."""

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
    return synth.make_dataset(str(tmp_path_factory.mktemp("tversky") / "ds"), n_train=8, n_val=4, size=SIZE)


def test_rs_train_one_epoch(root, tmp_path):
    log, values, _ = _train(root, str(tmp_path / "t"), "Tversky", {"tversky_alpha": 0.3, "tversky_beta": 0.7, "tversky_gamma": 0.75,
                                                                  "tversky_ce": 0.5})
    line = "Tversky:\t alpha = 0.3, beta = 0.7, gamma = 0.75, smooth = 1.0, per image, classes present, + 0.5 x cross-entropy"
    assert [l for l in log.splitlines() if l.startswith("Tversky:")] == [line], log
    assert "Loss function:\t Tversky" in log
    assert 0.0 < float(values["Train"]) and 0.0 < float(values["Valid"])


def test_rs_train_as_a_captured_graph(root, tmp_path):
    log, values, _ = _train(root, str(tmp_path / "g"), "Tversky", {"tversky_per_image": False, "tversky_classes": "all", "tversky_ce": 1.0},
                            graph=True)
    assert "over the batch, classes all, + 1.0 x cross-entropy" in log
    assert 0.0 < float(values["Train"]) and 0.0 < float(values["Valid"])


def test_the_fused_loss_is_the_sum_of_its_terms(root, tmp_path):
    """``lr = 0``: the three runs end on the same network, and the third run's logged losses are the sums of the other two."""

    _, region, state_a = _train(root, str(tmp_path / "a"), "Tversky", {"tversky_ce": 0.0}, lr=0.0)
    plain_log, pixel, state_b = _train(root, str(tmp_path / "b"), "CrossEntropy", {}, lr=0.0)
    _, fused, state_c = _train(root, str(tmp_path / "c"), "Tversky", {"tversky_ce": 1.0}, lr=0.0)
    assert "Tversky:" not in plain_log
    assert _same_network(state_a, state_b) and _same_network(state_a, state_c)
    for key in ("Train", "Valid"):
        print(key, region[key], pixel[key], fused[key])
        assert abs(float(fused[key]) - (float(region[key]) + float(pixel[key]))) <= 1.5e-4, (key, region, pixel, fused)
        assert float(region[key]) > 1e-3 and float(pixel[key]) > 1e-3  # (both terms are there to be added)


@pytest.mark.parametrize("loss, opt, key", [
    ("Tversky", {"tversky_alpha": -1}, "tversky_alpha"),
    ("CrossEntropy", {"tversky_gamma": 0.75}, "tversky_gamma"),
    ("Tversky", {"boundary_weight": 4.0}, "boundary_weight"),
], ids=["a-bad-value", "a-key-with-another-loss", "the-boundary-weight-with-tversky"])
def test_a_bad_key_ends_rs_train(root, tmp_path, loss, opt, key):
    from robosat_amd.tools import train as train_tool

    args, ckdir = _configs(str(tmp_path), root, loss, opt)
    with pytest.raises(SystemExit) as err:
        train_tool.main(args)
    assert str(err.value).startswith("Error: [opt] " + key), str(err.value)
    assert not os.path.exists(ckdir)
