"""CPU checks of the clDice topology loss (no kernel is launched): the explicit per-pixel tie rules of tests/cldice_ref.py against
torch's autograd, the shared-erosion form against the paper's, the gradient coefficients of the scalar stage against autograd, the
config keys with their refusals, the module's constructor and the declared entry points."""

import argparse
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cldice_ref as R  # noqa: E402

from robosat_amd import ops  # noqa: E402
from robosat_amd.config import cldice_options, load_config, save_config  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (2, 1, 7), (2, 5, 1), (1, 3, 3), (2, 9, 11)]


def _plateaus(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 3, shape, generator=g).float() / 2, torch.randint(-3, 4, shape, generator=g).float()


# ---- the references -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_tie_rules_are_what_autograd_does(shape, iters):
    """Planes of {0, 1/2, 1} are nothing but plateaus; with integer gradients every number is a small dyadic, so fp32, fp64 and any
    order of summation give the same bits."""

    x, g = _plateaus(shape, 7 * iters + len(shape) + shape[-1])
    _, d32 = R.skeleton_autograd(x, iters, g, torch.float32)
    _, d64 = R.skeleton_autograd(x, iters, g, torch.float64)
    assert torch.equal(d32.double(), d64)
    assert np.array_equal(R.skeleton_bwd_numpy(x.numpy(), iters, g.numpy()), d32.numpy())


def test_the_half_shares_of_a_tie_may_land_on_one_cell():
    """A flat plane: v == h everywhere.  The corner cell is the first minimum of its own column and of its own row, so both halves
    of its own gradient come back to it, plus one half from the cell below and one from the cell to its right; the total gradient
    is conserved through an erosion."""

    x = torch.full((1, 4, 5), 0.5, requires_grad=True)
    g = torch.arange(20.0).reshape(1, 4, 5)
    (dx,) = torch.autograd.grad(R.erode(x), x, g)
    assert float(dx.sum()) == float(g.sum())
    assert float(dx[0, 0, 0]) == float(g[0, 0, 0]) + 0.5 * float(g[0, 1, 0]) + 0.5 * float(g[0, 0, 1])  # both halves of its own, one of each neighbour


@pytest.mark.parametrize("iters", [3, 10])
def test_the_shared_erosions_are_the_papers_form(iters):
    g = torch.Generator().manual_seed(iters)
    for x in (torch.rand((2, 23, 31), generator=g), torch.randint(0, 3, (2, 23, 31), generator=g).float() / 2):
        assert torch.equal(R.soft_skeleton(x, iters), R.soft_skeleton_paper(x, iters))


def test_the_coefficients_of_the_scalar_stage():
    """d term / d S_P = alpha Y + beta and d term / d P (through Tsens) = gamma S_Y, the formulas of rs_cldice_finalize, against
    autograd on the sums."""

    g = torch.Generator().manual_seed(3)
    sp, y, sy, p = (torch.rand((3, 6, 7), generator=g, dtype=torch.float64) for _ in range(4))
    y = (y > 0.5).double()
    sp.requires_grad_(True)
    p.requires_grad_(True)
    s = 1.0
    A, B, Cc, Dd = (sp * y).sum((1, 2)), sp.sum((1, 2)), (sy * p).sum((1, 2)), sy.sum((1, 2))
    tp, ts = (A + s) / (B + s), (Cc + s) / (Dd + s)
    loss = (1 - 2 * tp * ts / (tp + ts)).mean()
    dsp, dp = torch.autograd.grad(loss, (sp, p))
    scale = 1.0 / 3
    dtp, dts = -2 * ts ** 2 / (tp + ts) ** 2, -2 * tp ** 2 / (tp + ts) ** 2
    alpha, beta, gamma = scale * dtp / (B + s), -scale * dtp * (A + s) / (B + s) ** 2, scale * dts / (Dd + s)
    alpha, beta, gamma = alpha.detach(), beta.detach(), gamma.detach()
    assert float((dsp - (alpha[:, None, None] * y + beta[:, None, None])).abs().max()) <= 1e-15
    assert float((dp - gamma[:, None, None] * sy).abs().max()) <= 1e-15


def test_the_term_is_a_mean_over_equal_shards():
    """The divisor depends on the batch size alone: the term of a batch is the mean of the terms of its halves."""

    g = torch.Generator().manual_seed(5)
    logits = torch.randn((4, 3, 12, 14), generator=g, dtype=torch.float64)
    targets = torch.randint(0, 3, (4, 12, 14), generator=g)
    whole = R.cldice_term(logits, targets, 3, dtype=torch.float64)
    halves = [R.cldice_term(logits[i:i + 2], targets[i:i + 2], 3, dtype=torch.float64) for i in (0, 2)]
    assert abs(float(whole) - 0.5 * (float(halves[0]) + float(halves[1]))) <= 1e-15


# ---- the config keys ----------------------------------------------------------------------------------------------------------------
DATASET = {"common": {"dataset": "/tmp", "classes": ["background", "road", "building"], "colors": ["denim", "orange", "white"]}}


def _model(loss="CrossEntropy", **opt):
    return {"common": {"cuda": True, "batch_size": 2, "image_size": 64, "checkpoint": "/tmp/pth"},
            "opt": dict({"epochs": 1, "lr": 1e-4, "loss": loss}, **opt)}


def test_the_keys_are_read():
    assert cldice_options(_model(), DATASET) is None
    assert cldice_options(_model(cldice=0.3), DATASET) == {"weight": 0.3, "iters": 10, "smooth": 1.0, "classes": None}
    got = cldice_options(_model("Lovasz", cldice=0.5, cldice_iters=3, cldice_smooth=0, cldice_classes=["road"]), DATASET)
    assert got == {"weight": 0.5, "iters": 3, "smooth": 0.0, "classes": (1,)}
    assert cldice_options(_model(cldice=0.5, cldice_classes=["building", "road"]), DATASET)["classes"] == (1, 2)
    for loss in ("CrossEntropy", "Focal", "mIoU", "Lovasz", "LovaszSoftmax", "Tversky"):
        assert cldice_options(_model(loss, cldice=0.25, cldice_iters=64), DATASET)["iters"] == 64


REFUSALS = [
    ({"cldice": 0}, "cldice must be a number with 0 < a < 1"), ({"cldice": 1}, "cldice must be"), ({"cldice": 1.5}, "cldice must be"),
    ({"cldice": -0.1}, "cldice must be"), ({"cldice": True}, "cldice must be"), ({"cldice": "0.3"}, "cldice must be"),
    ({"cldice": float("nan")}, "cldice must be"),
    ({"cldice": 0.3, "cldice_iters": 0}, r"cldice_iters must be an integer in 1\.\.64"), ({"cldice": 0.3, "cldice_iters": 65}, "cldice_iters"),
    ({"cldice": 0.3, "cldice_iters": 3.0}, "cldice_iters"), ({"cldice": 0.3, "cldice_iters": True}, "cldice_iters"),
    ({"cldice": 0.3, "cldice_smooth": -1}, "cldice_smooth must be a finite number >= 0"),
    ({"cldice": 0.3, "cldice_smooth": float("inf")}, "cldice_smooth"),
    ({"cldice": 0.3, "cldice_classes": ["river"]}, "cldice_classes: 'river' is no non-background class"),
    ({"cldice": 0.3, "cldice_classes": ["background"]}, "cldice_classes: 'background' is no non-background class"),
    ({"cldice": 0.3, "cldice_classes": []}, "cldice_classes must be a non-empty list"),
    ({"cldice": 0.3, "cldice_classes": "road"}, "cldice_classes must be a non-empty list"),
    ({"cldice": 0.3, "cldice_classes": ["road", "road"]}, "cldice_classes names a class twice"),
    ({"cldice_iters": 3}, r"cldice_iters needs \[opt\] cldice"), ({"cldice_smooth": 1.0}, r"cldice_smooth needs \[opt\] cldice"),
    ({"cldice_classes": ["road"]}, r"cldice_classes needs \[opt\] cldice"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_a_bad_key_is_refused(case):
    opt, message = REFUSALS[case]
    with pytest.raises(ValueError, match=r"\[opt\] " + message):
        cldice_options(_model(**opt), DATASET)


def test_a_dataset_without_an_object_class_is_refused():
    with pytest.raises(ValueError, match=r"\[opt\] cldice needs a non-background class"):
        cldice_options(_model(cldice=0.3), {"common": {"classes": ["background"]}})


CLI_REFUSALS = [REFUSALS[i] for i in (0, 7, 11, 13, 18)]


@pytest.mark.parametrize("case", range(len(CLI_REFUSALS)))
def test_rs_train_ends_on_a_bad_key_before_any_work(tmp_path, case):
    """Every refusal is an ``Error: [opt] cldice...`` exit of ``rs train`` itself, before it asks for a device or makes the checkpoint
    directory."""

    from robosat_amd.tools import train as train_tool

    opt, _ = CLI_REFUSALS[case]
    ds = str(tmp_path / "dataset.toml")
    save_config(dict(DATASET, common=dict(DATASET["common"], dataset=str(tmp_path))), ds)
    ck = str(tmp_path / "pth")
    cfg = _model(**opt)
    cfg["common"]["checkpoint"] = ck
    cfg["model"] = {"pretrained": False}
    model = str(tmp_path / "model.toml")
    save_config(cfg, model)
    assert load_config(model)["opt"].keys() == cfg["opt"].keys()
    with pytest.raises(SystemExit) as err:
        train_tool.main(argparse.Namespace(model=model, dataset=ds, checkpoint=None, resume=False, workers=0))
    assert str(err.value).startswith("Error: [opt] cldice"), str(err.value)
    assert not os.path.exists(ck)


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def test_the_module_validates_its_arguments():
    from robosat_amd import losses

    base = losses.CrossEntropyLoss2d(hard=0.25)
    crit = losses.ClDiceLoss2d(base, 0.3)
    assert (crit.cldice_weight, crit.iters, crit.smooth, crit.classes, crit.ignore_index) == (0.3, 10, 1.0, None, None)
    assert crit.base is base and crit.hard == base.hard and losses.ClDiceLoss2d(losses.mIoULoss2d(), 0.3).hard is None
    crit.eval()
    assert not base.training  # (hard-pixel mining follows the mode)
    crit.train()
    assert base.training
    crit = losses.ClDiceLoss2d(base, weight=0.5, iters=0, smooth=0, classes=[2, 1], ignore_index=255)
    assert (crit.iters, crit.smooth, crit.classes, crit.ignore_index) == (0, 0.0, (2, 1), 255)
    for bad in (dict(weight=0), dict(weight=1), dict(weight=True), dict(weight="0.3"), dict(weight=0.3, iters=-1),
                dict(weight=0.3, iters=65), dict(weight=0.3, iters=2.0), dict(weight=0.3, smooth=-1), dict(weight=0.3, smooth=float("nan")),
                dict(weight=0.3, classes=[]), dict(weight=0.3, classes=[0]), dict(weight=0.3, classes=[1, 1])):
        with pytest.raises(ValueError):
            losses.ClDiceLoss2d(base, **bad)
    with pytest.raises(ValueError):
        losses.ClDiceLoss2d("CrossEntropy", 0.3)
    assert ops.cldice_class_mask(None, 3) == (0b110, 2) and ops.cldice_class_mask((2,), 3) == (0b100, 1)
    for bad in ((3,), (0,), (1, 1), ()):
        with pytest.raises(ValueError):
            ops.cldice_class_mask(bad, 3)
    with pytest.raises(RuntimeError, match="no CPU"):
        crit.term(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.soft_skeleton(torch.zeros(1, 4, 4), 3)
    with pytest.raises(ValueError):
        ops.soft_skeleton(torch.zeros(4, 4), 3)
    with pytest.raises(ValueError):
        ops.soft_skeleton(torch.zeros(1, 4, 4), 65)


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_bound_and_the_abi_version_stays():
    from ctypes import c_float, c_int, c_long

    from robosat_amd import _lib
    from robosat_amd._lib import P

    header = open(os.path.join(ROOT, "include", "robosat_hip.h")).read()
    want = {
        "rs_soft_skeleton_state_floats": (c_long, [c_int] * 5),
        "rs_soft_skeleton_fwd": (c_int, [P] * 3 + [c_int] * 5 + [P]),
        "rs_soft_skeleton_bwd_workspace_bytes": (c_long, [c_int] * 4),
        "rs_soft_skeleton_bwd": (c_int, [P] * 4 + [c_int] * 4 + [P, P]),
        "rs_cldice_planes": (c_int, [P] * 4 + [c_int] * 6 + [P]),
        "rs_cldice_workspace_bytes": (c_long, [c_int]),
        "rs_cldice_sums": (c_int, [P] * 5 + [c_int] * 3 + [P, P]),
        "rs_cldice_finalize": (c_int, [P] * 3 + [c_int, c_float, P]),
        "rs_cldice_skel_grad": (c_int, [P] * 3 + [c_int] * 3 + [P]),
        "rs_cldice_bwd": (c_int, [P] * 7 + [c_int] * 6 + [P]),
    }
    for name, signature in want.items():
        assert name + "(" in header and _lib.SIGNATURES[name] == signature, name
    assert _lib.ABI_VERSION == 24  # (new symbols, no old one changed)
    lib = _lib.lib()  # (resolves every symbol of the built library)
    assert lib.rs_soft_skeleton_state_floats(2, 5, 7, 10, 1) == 21 * 70 and lib.rs_soft_skeleton_state_floats(2, 5, 7, 10, 0) == 5 * 70
    assert lib.rs_soft_skeleton_bwd_workspace_bytes(2, 5, 7, 10) == 13 * 70 * 4
    assert lib.rs_soft_skeleton_state_floats(2, 5, 7, 65, 1) < 0 and lib.rs_cldice_workspace_bytes(0) < 0
    for line in ("S_k = S_{k-1} + relu(D_k - S_{k-1}*D_k)", "half through each, even when both halves land on the same cell",
                 "relu'(0) = 0", "2*iters + 1 planes", "an absent class is not skipped"):
        assert line in header, line
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7j" in design and "clDice" in design
