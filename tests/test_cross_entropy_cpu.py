"""CPU tests of ops.cross_entropy (K21): the plain-torch fp32 path, which
is the golden model of the contract, against F.cross_entropy in float64
within the derived bounds of tests/xent_bounds.py (its docstring has the
derivation); the inputs the wrapper refuses; and agreement with
ops.log_softmax_nll where the two ops overlap."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_bounds as fb  # noqa: E402
import xent_bounds as xb  # noqa: E402

from dist_tuto_pth_amd import ops  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("regime", xb.XENT_REGIMES)
@pytest.mark.parametrize("shape", xb.XENT_SHAPES, ids=str)
def test_cross_entropy_bounds(shape, regime):
    assert xb.xent_case(shape, regime, DEV) <= 1.0


@pytest.mark.parametrize("case", xb.xent_validation_cases(gpu=False),
                         ids=lambda c: c[0])
def test_cross_entropy_refuses(case):
    name, exc, call = case
    with pytest.raises(exc, match=r"ops\.cross_entropy"):
        call(DEV)


@pytest.mark.parametrize("N", xb.NAN_N)
def test_nan_logits_reach_the_loss(N):
    xb.nan_case(N, DEV)


def test_bf16_logits_give_fp32_loss_and_bf16_gradient():
    x, tgt, gvec = xb.xent_inputs((3, 65), "randn")
    xh = x.to(torch.bfloat16)
    loss, gx = xb.xent_run(xh, tgt, gvec, 0.125, -100, "mean", DEV)
    ref_loss, ref_gx = xb.xent_run(xh.float(), tgt, gvec, 0.125, -100,
                                   "mean", DEV)
    assert gx.dtype == torch.bfloat16
    assert torch.equal(loss, ref_loss)
    assert torch.equal(gx, ref_gx.to(torch.bfloat16))


@pytest.mark.parametrize("regime", fb.REGIMES)
@pytest.mark.parametrize("shape", [(3, 1000), (257, 10), (1, 1)], ids=str)
def test_matches_log_softmax_nll(shape, regime):
    """eps = 0, default ignore_index, "mean": the loss of
    ops.log_softmax_nll, to within the sum of the two ops' bounds (each is
    within its own bound of the same float64 value)."""
    ref = fb.softmax_reference(shape, regime)
    x, tgt = ref["x"], ref["tgt"]
    a = ops.cross_entropy(x, tgt)
    b = ops.log_softmax_nll(x, tgt)
    gvec = torch.zeros(shape[0])
    mine = xb.xent_reference(x, tgt, gvec, 0.0, -100, "mean")
    bound = float(mine["Bloss"]) + float(ref["Bloss"]) + 2 * fb.TINY
    assert abs(float(a) - float(b)) <= bound
    assert abs(float(mine["loss"]) - float(ref["loss"])) <= 1e-12 * max(
        1.0, abs(float(ref["loss"])))


def test_zz_report_ratios():
    """Prints the largest error/bound ratio per quantity of this run."""
    xb.xent_report()
