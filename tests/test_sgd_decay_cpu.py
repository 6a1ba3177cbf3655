"""CPU tests of FusedSGD's weight decay and Nesterov momentum: two steps
against torch.optim.SGD on float64 copies, within the bounds derived in
tests/xent_bounds.py, and the two refused settings."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xent_bounds as xb  # noqa: E402

from dist_tuto_pth_amd.optim import FusedSGD  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("which", list(xb.DECAY_LISTS))
def test_fused_sgd_decay_bounds(which, nesterov, zero_grad):
    xb.decay_case(which, nesterov, zero_grad, DEV)


@pytest.mark.parametrize("zero_grad", [False, True])
def test_weight_decay_without_momentum(zero_grad):
    xb.decay_no_momentum_case(zero_grad, DEV)


def test_refuses_nesterov_without_momentum():
    p = torch.zeros(4, requires_grad=True)
    with pytest.raises(ValueError, match="FusedSGD"):
        FusedSGD([p], lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="FusedSGD"):
        FusedSGD([p], lr=0.1, nesterov=True)


def test_refuses_negative_weight_decay():
    p = torch.zeros(4, requires_grad=True)
    with pytest.raises(ValueError, match="FusedSGD"):
        FusedSGD([p], lr=0.1, momentum=0.5, weight_decay=-1e-4)


def test_defaults_keep_the_plain_rule():
    """weight_decay=0 and nesterov=False are today's update, bit for bit."""
    g = torch.Generator().manual_seed(3)
    a = torch.randn(257, generator=g)
    grad = torch.randn(257, generator=g)
    pa = a.clone().requires_grad_(True)
    pb = a.clone().requires_grad_(True)
    oa = FusedSGD([pa], lr=0.1, momentum=0.9)
    ob = FusedSGD([pb], lr=0.1, momentum=0.9, weight_decay=0.0,
                  nesterov=False)
    for _ in range(2):
        pa.grad, pb.grad = grad.clone(), grad.clone()
        oa.step()
        ob.step()
    assert torch.equal(pa.detach(), pb.detach())
