"""The dataset config's ``[common] ignore = 255`` end to end on the MI355X: ``rs train`` (every loss, the default loaders and the
decoded-tile cache with a zoom table, once as a captured graph), ``rs weights`` and ``rs evaluate`` on a synthetic dataset whose
labels are 255 in their left third, one of them everywhere."""

import argparse
import csv
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import synth
from robosat_amd.config import load_config, save_config
from robosat_amd.tiles import tiles_from_slippy_map

pytestmark = pytest.mark.gpu
IGNORE = 255
SIZE = 256
LOSSES = ["CrossEntropy", "Focal", "mIoU", "Lovasz", "LovaszSoftmax"]


def _label_paths(root, split):
    return sorted(path for _, path in tiles_from_slippy_map(os.path.join(root, split, "labels")))


def _read(path):
    with Image.open(path) as image:
        return np.array(image, dtype=np.uint8)


def _write_label(path, array):
    image = Image.fromarray(array, mode="P")
    image.putpalette([0, 0, 0, 250, 0, 0] + [0] * (254 * 3))
    image.save(path)


def _dataset(tmp):
    """``synth.make_dataset`` (8 train, 4 val, 256 x 256) with the left third of every label set to 255 and the first label of each
    split set to 255 everywhere.  Returns (root, {split: [the labels as written]}, {split: [the labels before]})."""

    root = synth.make_dataset(os.path.join(tmp, "ds"), n_train=8, n_val=4, size=SIZE)
    after, before = {}, {}
    for split in ("training", "validation"):
        after[split], before[split] = [], []
        for k, path in enumerate(_label_paths(root, split)):
            label = _read(path)
            before[split].append(label.copy())
            label[:, : SIZE // 3] = IGNORE
            if k == 0:
                label[:] = IGNORE
            _write_label(path, label)
            assert (_read(path) == label).all()
            after[split].append(label)
    return root, after, before


def _configs(tmp, root, loss, ignore=True, device_augment=False, zoom=False, graph=False):
    ckdir = os.path.join(tmp, "pth-{}".format(loss))
    model_toml, ds_toml = synth.write_configs(tmp, root, ckdir, loss=loss, batch_size=2, image_size=SIZE, epochs=1)
    cfg = load_config(model_toml)
    if device_augment:
        cfg.setdefault("model", {})["device_augment"] = True
    if graph:
        cfg.setdefault("model", {})["graph"] = True
    if zoom:
        cfg["augment"] = {"zoom": 1.5}
    save_config(cfg, model_toml)
    ds = load_config(ds_toml)
    if ignore:
        ds["common"]["ignore"] = IGNORE
    save_config(ds, ds_toml)
    return argparse.Namespace(model=model_toml, dataset=ds_toml, checkpoint=None, resume=False, workers=0), ckdir


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("ignore"))
    root, after, before = _dataset(tmp)
    return {"tmp": tmp, "root": root, "after": after, "before": before}


def _train(data, tmp, loss, **kw):
    from robosat_amd.tools import train as train_tool

    args, ckdir = _configs(tmp, data["root"], loss, **kw)
    train_tool.main(args)
    log = open(os.path.join(ckdir, "log")).read()
    assert "Train    loss:" in log and "Validate loss:" in log
    assert [l for l in log.splitlines() if l.startswith("Ignore label:")] == ["Ignore label:\t 255"], log
    for line in log.splitlines():
        if line.startswith(("Train    loss:", "Validate loss:")):
            value = float(line.split("loss:")[1].split(",")[0])
            assert np.isfinite(value) and value >= 0.0, line
    ck = torch.load(os.path.join(ckdir, "checkpoint-00001-of-00001.pth"), map_location="cpu")
    assert int(ck["state_dict"]["module.resnet.bn1.num_batches_tracked"]) == 4
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values() if v.is_floating_point())
    return log


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("feed", ["default-loaders", "device-augment-zoom"])
def test_rs_train_one_epoch(data, tmp_path, loss, feed):
    _train(data, str(tmp_path), loss, device_augment=feed == "device-augment-zoom", zoom=feed == "device-augment-zoom")


def test_rs_train_as_a_captured_graph(data, tmp_path):
    """``[model] graph = true``: the step with the ignore label is captured after two eager batches and replayed (no host sync in
    the loss)."""

    _train(data, str(tmp_path), "LovaszSoftmax", graph=True)


def test_rs_train_without_the_key_logs_no_ignore_line(data, tmp_path):
    """Without the key nothing is said or passed: the criterion has no ignore index (the run itself is what the existing tests cover)."""

    from robosat_amd.config import ignore_label

    args, _ = _configs(str(tmp_path), data["root"], "Lovasz", ignore=False)
    assert ignore_label(load_config(args.dataset)) is None


@pytest.mark.parametrize("feed", ["default-loaders", "device-augment", "device-augment-zoom"])
def test_the_loaders_carry_the_byte_through_as_int64_255(data, tmp_path, feed):
    """The training feeds as they are (not changed for this): flips and quarter turns move the ignored pixels and keep their
    number; a zoom crop samples labels by nearest neighbour, so it invents no value between a class and 255."""

    from robosat_amd.tools import train as train_tool

    args, _ = _configs(str(tmp_path), data["root"], "Lovasz", device_augment=feed != "default-loaders", zoom=feed.endswith("zoom"))
    model, dataset = load_config(args.model), load_config(args.dataset)
    device = torch.device("cuda", 0)
    if feed == "default-loaders":
        train_loader, val_loader = train_tool.get_split_loaders(model, dataset, 0, device)
    else:
        train_loader, val_loader = train_tool.get_device_loaders(model, dataset, device)
    train_loader.batch_sampler.set_epoch(0)
    for loader, split in ((train_loader, "training"), (val_loader, "validation")):
        ignored = pixels = 0
        for _, masks, _ in loader:
            assert masks.dtype == torch.int64 and tuple(masks.shape[1:]) == (SIZE, SIZE)
            values = set(torch.unique(masks).tolist())
            assert values <= {0, 1, IGNORE}, values
            ignored += int((masks == IGNORE).sum())
            pixels += masks.numel()
        want = int(sum((label == IGNORE).sum() for label in data["after"][split]))
        assert pixels == len(data["after"][split]) * SIZE * SIZE
        if split == "validation" or not feed.endswith("zoom"):
            assert ignored == want, (split, ignored, want)
        else:
            assert 0 < ignored < pixels  # (a crop holds more or less of the ignored third; the wholly ignored tile stays so)


def test_rs_weights_counts_the_valid_pixels(data, tmp_path, capsys):
    from robosat_amd.tools import weights as weights_tool

    args, _ = _configs(str(tmp_path), data["root"], "Lovasz")
    capsys.readouterr()
    weights_tool.main(argparse.Namespace(dataset=args.dataset))
    printed = capsys.readouterr().out.strip().splitlines()[-1]
    labels = np.stack(data["after"]["training"])
    valid = labels[labels != IGNORE]
    assert 0 < valid.size < labels.size
    want = (1 / np.log(1.02 + np.bincount(valid, minlength=2) / valid.size)).round(6).tolist()
    assert json.loads(printed) == want, (printed, want)
    # without the key the 255 byte is outside the classes, as it was
    plain, _ = _configs(str(tmp_path), data["root"], "Lovasz", ignore=False)
    with pytest.raises(ValueError, match=r"labels outside \[0, 2\)"):
        weights_tool.main(argparse.Namespace(dataset=plain.dataset))


def _evaluate(dataset, masks, labels, out, tiles=None, kind=None):
    from robosat_amd.tools import evaluate as evaluate_tool

    evaluate_tool.main(argparse.Namespace(masks=masks, labels=labels, dataset=dataset, out=out, type=kind, boundary=0, match=None,
                                          min_area=None, stitch=False, tiles=tiles, batch_size=3))


def test_rs_evaluate_counts_ignored_pixels_apart(data, tmp_path):
    tmp = str(tmp_path)
    args, _ = _configs(tmp, data["root"], "Lovasz")
    labels_dir = os.path.join(data["root"], "validation", "labels")
    masks_dir = os.path.join(tmp, "masks")
    rng = np.random.default_rng(7)
    masks = {}
    for (tile, path), before in zip(sorted(tiles_from_slippy_map(labels_dir), key=lambda e: e[1]), data["before"]["validation"]):
        mask = np.where(rng.random(before.shape) < 0.1, 1 - before, before).astype(np.uint8)  # the labels as they were, 10 % wrong
        os.makedirs(os.path.join(masks_dir, str(tile.z), str(tile.x)), exist_ok=True)
        _write_label(os.path.join(masks_dir, str(tile.z), str(tile.x), "{}.png".format(tile.y)), mask)
        masks[(tile.z, tile.x, tile.y)] = (mask, _read(path))
    out, rows_csv = os.path.join(tmp, "report.json"), os.path.join(tmp, "tiles.csv")
    _evaluate(args.dataset, masks_dir, labels_dir, out, tiles=rows_csv)
    with open(out) as fp:
        report = json.load(fp)
    want = np.zeros((2, 2), dtype=np.int64)
    ignored = 0
    for mask, label in masks.values():
        valid = label != IGNORE
        np.add.at(want, (label[valid], mask[valid]), 1)
        ignored += int((~valid).sum())
    assert ignored > 4 * SIZE * SIZE // 3  # (a third of three tiles and a whole one)
    assert report["ignore"] == IGNORE and report["ignored"] == ignored and report["confusion"] == want.tolist()
    assert report["pixels"] == int(want.sum()) == 4 * SIZE * SIZE - ignored and report["tiles"] == 4
    with open(rows_csv, newline="") as fp:
        rows = list(csv.DictReader(fp))
    assert len(rows) == 4
    for row in rows:
        mask, label = masks[(int(row["z"]), int(row["x"]), int(row["y"]))]
        assert int(row["ignored"]) == int((label == IGNORE).sum()) and int(row["pixels"]) == int((label != IGNORE).sum())
    assert rows[-1]["miou"] == "" and int(rows[-1]["pixels"]) == 0  # the wholly ignored tile: no score, last
    # --type: boundaries and objects next to ignored pixels are not defined yet: the run ends and names a tile
    with pytest.raises(SystemExit) as err:
        _evaluate(args.dataset, masks_dir, labels_dir, os.path.join(tmp, "typed.json"), kind="parking")
    message = str(err.value)
    assert message.startswith("Error: the label of tile 18/") and "ignore value 255" in message and "--type" in message
    assert any("{}/{}/{}".format(*key) in message for key in masks) and not os.path.exists(os.path.join(tmp, "typed.json"))
    # a mask byte that is no class still ends the run, ignore label or not
    wrong_dir = os.path.join(tmp, "wrong")
    for (z, x, y), (mask, _) in masks.items():
        os.makedirs(os.path.join(wrong_dir, str(z), str(x)), exist_ok=True)
        bad = mask.copy()
        bad[3, SIZE - 4] = 5
        _write_label(os.path.join(wrong_dir, str(z), str(x), "{}.png".format(y)), bad)
    with pytest.raises(SystemExit) as err:
        _evaluate(args.dataset, wrong_dir, labels_dir, os.path.join(tmp, "wrong.json"))
    assert "none of the dataset's 2 classes" in str(err.value)
    # and without the key the 255 byte of a label ends the run as it did
    plain, _ = _configs(tmp, data["root"], "Lovasz", ignore=False)
    with pytest.raises(SystemExit) as err:
        _evaluate(plain.dataset, masks_dir, labels_dir, os.path.join(tmp, "plain.json"))
    assert "none of the dataset's 2 classes" in str(err.value) and not os.path.exists(os.path.join(tmp, "plain.json"))
