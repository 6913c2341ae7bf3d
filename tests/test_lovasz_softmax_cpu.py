"""Lovasz-Softmax without a GPU: the float64 restatement the GPU tests compare with is pinned here (its value at hard
predictions is the Jaccard loss, its gradient is the derivative of its value), and the host-side contract of
``LovaszSoftmax2d`` / ``rs train``'s option keys is checked."""

import pytest
import torch

import lovasz_softmax_ref as ref
from robosat_amd.losses import LovaszSoftmax2d


@pytest.mark.parametrize("c", [2, 3, 5])
@pytest.mark.parametrize("per_image", [True, False])
def test_restatement_equals_one_minus_mean_iou_at_hard_predictions(c, per_image):
    """Errors in {0, 1}: the Lovasz extension agrees with the Jaccard loss on the cube's vertices, whatever the tie order."""

    g = torch.Generator().manual_seed(c)
    n, h, w = 3, 9, 11
    y = torch.randint(0, c, (n, h, w), generator=g)
    y[0][y[0] == c - 1] = 0  # a class absent from one image
    pred = torch.where(torch.rand(n, h, w, generator=g) < 0.6, y, torch.randint(0, c, (n, h, w), generator=g))
    p = torch.nn.functional.one_hot(pred, c).permute(0, 3, 1, 2).double()
    got = float(ref.lovasz_softmax(p, y, per_image=per_image))
    assert got == pytest.approx(ref.mean_iou_loss(pred, y, c, per_image=per_image), abs=1e-12)


@pytest.mark.parametrize("per_image,classes", [(True, "present"), (False, "present"), (True, "all"), (False, "all")])
def test_restatement_gradient_matches_central_differences(per_image, classes):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64)
    y = torch.randint(0, 3, (2, 3, 3), generator=g)
    y[0][y[0] == 2] = 1
    assert ref.min_error_gap(torch.softmax(x, 1), y, per_image) > 1e-4  # tie-free: the order holds within +-h

    def f(t):
        return ref.lovasz_softmax(torch.softmax(t, 1), y, per_image=per_image, classes=classes)

    xa = x.clone().requires_grad_(True)
    f(xa).backward()
    h = 1e-6
    num = torch.zeros_like(x)
    for i in range(x.numel()):
        d = torch.zeros(x.numel(), dtype=torch.float64)
        d[i] = h
        d = d.view_as(x)
        num.view(-1)[i] = (f(x + d) - f(x - d)) / (2 * h)
    assert float((xa.grad - num).abs().max()) <= 1e-7 * max(1.0, float(num.abs().max()))


def test_separated_inputs_have_the_promised_gap():
    for c, shape in ((2, (3, 64, 64)), (3, (3, 32, 32)), (5, (3, 24, 24))):
        x, y = ref.separated_inputs(shape[0], c, shape[1], shape[2], seed=c)
        p = torch.softmax(x, 1)
        for per_image in (True, False):
            assert ref.min_error_gap(p, y, per_image) >= 1e-5
        assert not (y[0] == c - 1).any() and (y[1:] == c - 1).any()


def test_module_contract_on_the_host():
    with pytest.raises(ValueError):
        LovaszSoftmax2d(classes="some")
    crit = LovaszSoftmax2d()
    assert crit.per_image and crit.classes == "present"
    with pytest.raises(RuntimeError, match="MI355X only"):
        crit(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))


def test_rs_train_option_keys():
    from robosat_amd.tools.train import lovasz_softmax_options

    assert lovasz_softmax_options({"opt": {"loss": "LovaszSoftmax"}}, 1) == (True, "present")
    assert lovasz_softmax_options({"opt": {"lovasz_per_image": False, "lovasz_classes": "all"}}, 1) == (False, "all")
    assert lovasz_softmax_options({"opt": {"lovasz_per_image": True}}, 4) == (True, "present")
    for opt, world, msg in (({"lovasz_classes": "some"}, 1, "lovasz_classes"), ({"lovasz_per_image": "yes"}, 1, "lovasz_per_image"),
                            ({"lovasz_per_image": False}, 2, "global batch")):
        with pytest.raises(SystemExit) as e:
            lovasz_softmax_options({"opt": opt}, world)
        assert str(e.value).startswith("Error: ") and msg in str(e.value)
