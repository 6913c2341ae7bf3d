"""The ignore label without a GPU: the compaction reference (tests/ignore_ref.py) against the oracle and against torch's own
``ignore_index``, the dataset config key, ``rs weights``' arithmetic with an ignore count, the new entry points, and the shape of
``rs evaluate``'s report and tile list."""

import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ignore_ref as I  # noqa: E402
import losses_ref as L  # noqa: E402
import lovasz_softmax_ref as LS  # noqa: E402
from oracle import robosat_ref as R  # noqa: E402

from robosat_amd import evaluate as H  # noqa: E402
from robosat_amd.config import ignore_label  # noqa: E402
from robosat_amd.tiles import Tile  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [s for s in I.SHAPES if s != (1, 2, 96, 96)]  # (the CPU checks need no sort tiles)


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", L.CRITERIA)
def test_with_no_pixel_ignored_the_reference_is_the_oracle(shape, name):
    logits, targets, mask, weight = I.random_inputs(shape, "none", confident=(name == "mIoU"))
    assert not mask.any()
    for w in (None, weight):
        want_loss, want_grad = L.ref64(name, logits, targets, w)
        got_loss, got_grad, _ = I.loss64(name, logits, targets, weight=w)
        # (the same sums taken image by image: equal to rounding in float64, far below any bar of the kernels' tests)
        assert abs(got_loss - want_loss) <= 1e-12 * max(1.0, abs(want_loss)), (got_loss, want_loss)
        assert float((got_grad - want_grad).abs().max()) <= 1e-12 * max(1e-6, float(want_grad.abs().max()))


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_with_no_pixel_ignored_the_lovasz_references_are_the_oracle(shape):
    logits, targets, mask, _ = I.random_inputs(shape, "none")
    x = logits.double().requires_grad_(True)
    with I._float64_default():
        want = R.lovasz2d(x, targets)
    want.backward()
    got_loss, got_grad, _ = I.loss64("Lovasz", logits, targets)
    assert abs(got_loss - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    assert float((got_grad - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    logits, targets, mask = I.separated_softmax_inputs(shape, "none")
    for per_image in (True, False):
        for classes in ("present", "all"):
            x = logits.double().requires_grad_(True)
            want = LS.lovasz_softmax(torch.softmax(x, 1), targets, per_image=per_image, classes=classes)
            want.backward()
            got_loss, got_grad, _ = I.loss64("LovaszSoftmax", logits, targets, per_image=per_image, classes=classes)
            assert abs(got_loss - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
            assert float((got_grad - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


def test_the_soft_iou_term_is_the_helper_the_oracle_pins():
    logits, targets, _, weight = I.random_inputs((3, 4, 16, 16), "none", confident=True)
    miou, _, _ = L.miou_terms64(logits, targets, weight)
    _, _, extras = I.loss64("mIoU", logits, targets, weight=weight)
    assert abs(extras["miou"] - float(miou.detach())) <= 1e-12


@pytest.mark.parametrize("case", [c for c in I.cases() if c[0] in SMALL], ids=I.case_id)
def test_the_cross_entropy_reference_is_torchs_ignore_index(case):
    shape, pattern = case
    logits, targets, mask, weight = I.random_inputs(shape, pattern)
    for w in (None, weight):
        got_loss, got_grad, _ = I.loss64("CrossEntropy", logits, targets, weight=w)
        x = logits.double().requires_grad_(True)
        want = F.cross_entropy(x, targets, None if w is None else w.double(), ignore_index=I.IGNORE)
        if bool(mask.all()):
            assert torch.isnan(want) and got_loss == 0.0 and not got_grad.any()  # (torch's 0 / 0; the definition here says 0)
            continue
        want.backward()
        want = want.detach()
        assert abs(got_loss - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
        assert float((got_grad - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
        assert not got_grad.permute(0, 2, 3, 1)[mask].any()


@pytest.mark.parametrize("case", [c for c in I.cases() if c[0] in SMALL], ids=I.case_id)
def test_the_reference_has_no_gradient_at_and_no_use_for_ignored_pixels(case):
    shape, pattern = case
    logits, targets, mask, weight = I.random_inputs(shape, pattern, confident=True)
    other = I.other_logits_at(logits, mask)
    for name in L.CRITERIA + ("Lovasz",):
        loss, grad, _ = I.loss64(name, logits, targets, weight=weight if name in L.CRITERIA else None)
        assert not grad.permute(0, 2, 3, 1)[mask].any() and bool(torch.isfinite(grad).all())
        loss2, grad2, _ = I.loss64(name, other, targets, weight=weight if name in L.CRITERIA else None)
        assert loss2 == loss and torch.equal(grad2, grad)
        if pattern == "all":
            assert loss == 0.0 and not grad.any()


# ---- the dataset config key -----------------------------------------------------------------------------------------------------
def _dataset(ignore, classes=("background", "parking")):
    common = {"dataset": "/nowhere", "classes": list(classes), "colors": ["denim", "orange"]}
    if ignore is not None:
        common["ignore"] = ignore
    return {"common": common}


def test_the_config_key():
    assert ignore_label(_dataset(None)) is None
    assert ignore_label(_dataset(255)) == 255 and ignore_label(_dataset(2)) == 2
    assert ignore_label(_dataset(3, classes=("a", "b", "c"))) == 3
    for bad in (1, 0, -1, 256, True, False, 255.0, "255", [255]):
        with pytest.raises(ValueError, match=r"\[common\] ignore"):
            ignore_label(_dataset(bad))
    with pytest.raises(ValueError):
        ignore_label(_dataset(2, classes=("a", "b", "c")))


def test_the_config_key_from_a_toml_file(tmp_path):
    from robosat_amd.config import load_config

    for text, ok in (("ignore = 255", True), ("ignore = 1", False), ("ignore = 256", False), ("ignore = true", False)):
        path = tmp_path / "dataset.toml"
        path.write_text('[common]\ndataset = "/nowhere"\nclasses = ["background", "parking"]\ncolors = ["denim", "orange"]\n' + text + "\n")
        if ok:
            assert ignore_label(load_config(str(path))) == 255
        else:
            with pytest.raises(ValueError):
                ignore_label(load_config(str(path)))


@pytest.mark.parametrize("tool", ["train", "weights", "evaluate"])
def test_the_tools_end_on_a_bad_key_before_any_work(tmp_path, tool):
    """``ignore = 1`` with two classes: every tool that reads the key says so and stops -- before it asks for a device."""

    import argparse

    from robosat_amd.config import save_config
    from robosat_amd.tools import evaluate as evaluate_tool, train as train_tool, weights as weights_tool

    ds = str(tmp_path / "dataset.toml")
    save_config({"common": {"dataset": str(tmp_path), "classes": ["background", "parking"], "colors": ["denim", "orange"], "ignore": 1},
                 "weights": {"values": [1.0, 2.0]}}, ds)
    ck = str(tmp_path / "pth")
    model = str(tmp_path / "model.toml")
    save_config({"common": {"cuda": True, "batch_size": 2, "image_size": 64, "checkpoint": ck},
                 "opt": {"epochs": 1, "lr": 1e-4, "loss": "Lovasz"}, "model": {"pretrained": False}}, model)
    os.makedirs(str(tmp_path / "masks"))
    os.makedirs(str(tmp_path / "labels"))
    calls = {
        "train": lambda: train_tool.main(argparse.Namespace(model=model, dataset=ds, checkpoint=None, resume=False, workers=0)),
        "weights": lambda: weights_tool.main(argparse.Namespace(dataset=ds)),
        "evaluate": lambda: evaluate_tool.main(argparse.Namespace(
            masks=str(tmp_path / "masks"), labels=str(tmp_path / "labels"), dataset=ds, out=str(tmp_path / "r.json"), type=None,
            boundary=0, match=None, min_area=None, stitch=False, tiles=None, batch_size=16)),
    }
    with pytest.raises(SystemExit) as err:
        calls[tool]()
    assert str(err.value).startswith("Error: [common] ignore must be an integer in 2..255"), str(err.value)
    assert not os.path.exists(ck) and not os.path.exists(str(tmp_path / "r.json"))


# ---- rs weights -----------------------------------------------------------------------------------------------------------------
def test_rs_weights_leaves_the_ignored_pixels_out_of_counts_and_n():
    from robosat_amd.tools.weights import valid_counts, weights_from_counts

    rng = np.random.default_rng(0)
    labels = rng.integers(0, 3, size=5000).astype(np.uint8)
    labels[rng.random(5000) < 0.25] = 255
    hist = np.bincount(labels, minlength=256)
    n, counts = valid_counts(labels.size, hist, 3, 255, "here")
    valid = labels[labels != 255]
    assert n == valid.size and counts.tolist() == np.bincount(valid, minlength=3).tolist() and counts.dtype == np.int64
    want = (1 / np.log(1.02 + np.bincount(valid, minlength=3) / valid.size)).round(6).tolist()
    assert weights_from_counts(n, counts) == want
    assert want != weights_from_counts(labels.size, counts)  # (n matters: the ignored pixels are no share of anything)
    # without the key the byte is out of range, as before; with it, any OTHER byte out of range still is
    with pytest.raises(ValueError, match=r"labels outside \[0, 3\)"):
        valid_counts(labels.size, hist, 3, None, "here")
    hist[7] = 1
    with pytest.raises(ValueError, match=r"labels outside \[0, 3\)"):
        valid_counts(labels.size + 1, hist, 3, 255, "here")
    # and without ignored pixels nothing changes
    clean = np.bincount(valid, minlength=256)
    assert valid_counts(valid.size, clean, 3, None, "x")[0] == valid_counts(valid.size, clean, 3, 255, "x")[0] == valid.size


# ---- the entry points -------------------------------------------------------------------------------------------------------------
NEW = {"rs_nll_loss_fwd_ig": "rs_nll_loss_fwd", "rs_nll_loss_bwd_ig": "rs_nll_loss_bwd", "rs_miou_loss_fwd_ig": "rs_miou_loss_fwd",
       "rs_miou_loss_bwd_ig": "rs_miou_loss_bwd", "rs_lovasz_fwd_ig": "rs_lovasz_fwd", "rs_lovasz_softmax_fwd_ig": "rs_lovasz_softmax_fwd"}


def test_the_new_symbols_are_declared_bound_and_the_abi_version_stays():
    from ctypes import c_int

    from robosat_amd import _lib

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    for name, base in NEW.items():
        assert re.search(r"\bint {}\([^;]*rs_stream_t stream, int ignore\);".format(name), header), name
        ret, args = _lib.SIGNATURES[name]
        assert (ret, args) == (_lib.SIGNATURES[base][0], _lib.SIGNATURES[base][1] + [c_int])  # the base signature plus `int ignore`
    assert re.search(r"\bint rs_eval_confusion_ig\(const uint8_t\* predicted, const uint8_t\* actual, int64_t\* counts, int64_t\* bad, "
                     r"int64_t\* ignored, long pixels,\s+long group, int C, rs_stream_t stream, int ignore\);", header)
    assert len(_lib.SIGNATURES["rs_eval_confusion_ig"][1]) == len(_lib.SIGNATURES["rs_eval_confusion"][1]) + 2
    assert _lib.ABI_VERSION == 24  # (new symbols, no old one changed)
    assert "exactly +0.0f in every class plane of an ignored pixel" in header
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        assert lib.rs_abi_version() == 24
        for name in list(NEW) + ["rs_eval_confusion_ig"]:
            assert hasattr(lib, name)


def test_the_modules_take_ignore_index_and_validate_it_in_forward():
    from robosat_amd import losses

    for cls in (losses.CrossEntropyLoss2d, losses.FocalLoss2d, losses.mIoULoss2d, losses.LovaszLoss2d, losses.LovaszSoftmax2d):
        assert cls().ignore_index is None and cls(ignore_index=255).ignore_index == 255
    x = torch.zeros(1, 3, 4, 4)
    assert losses._check_ignore(None, x) is None and losses._check_ignore(3, x) == 3 and losses._check_ignore(255, x) == 255
    for bad in (2, 0, -100, 256, True, 3.5):
        with pytest.raises(ValueError, match="ignore_index"):
            losses._check_ignore(bad, x)


def test_metrics_says_what_it_does_with_labels_outside_the_classes():
    from robosat_amd.metrics import Metrics

    assert "outside the classes" in Metrics.add_batch.__doc__ and "not counted" in Metrics.add_batch.__doc__


# ---- rs evaluate's report -----------------------------------------------------------------------------------------------------------
def test_the_report_and_the_tile_rows_carry_the_ignored_counts(tmp_path):
    classes = ["background", "parking"]
    matrices = [[[10, 2], [3, 5]], [[0, 0], [0, 0]], [[7, 0], [0, 9]]]
    ignored = [4, 36, 0]
    tiles = [Tile(1000, 2000, 18), Tile(1000, 2001, 18), Tile(1001, 2000, 18)]
    total = np.sum(matrices, axis=0).tolist()
    plain = H.build_report(classes, total, 3, 0)
    report = H.build_report(classes, total, 3, 0, ignore=255, ignored=sum(ignored))
    assert "ignored" not in plain and "ignore" not in plain  # (without the key the report is what it was)
    assert report["ignore"] == 255 and report["ignored"] == 40 and report["pixels"] == 36 == sum(map(sum, total))
    assert {k: v for k, v in report.items() if k not in ("ignore", "ignored")} == plain
    rows = H.tile_rows(tiles, matrices, classes, ignored=ignored)
    by_tile = {(r["x"], r["y"]): r for r in rows}
    assert by_tile[(1000, 2000)]["pixels"] == 20 and by_tile[(1000, 2000)]["ignored"] == 4
    assert by_tile[(1000, 2001)]["pixels"] == 0 and by_tile[(1000, 2001)]["ignored"] == 36 and by_tile[(1000, 2001)]["miou"] is None
    assert rows[-1]["ignored"] == 36  # (a wholly ignored tile has no score: it sorts last)
    assert all("ignored" not in r for r in H.tile_rows(tiles, matrices, classes))
    assert H.tile_columns(classes, ignored=True) == ["z", "x", "y", "pixels", "ignored", "iou_background", "iou_parking", "miou",
                                                    "predicted_share", "actual_share"]
    assert "ignored" not in H.tile_columns(classes)
    path = str(tmp_path / "tiles.csv")
    H.write_tile_rows(path, rows, classes, ignored=True)
    lines = open(path).read().splitlines()
    assert lines[0].split(",")[4] == "ignored" and len(lines) == 4
    assert sorted(int(l.split(",")[4]) for l in lines[1:]) == [0, 4, 36]
