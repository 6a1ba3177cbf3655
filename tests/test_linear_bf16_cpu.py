"""CPU tests of the mixed-precision linear contract (ops.linear_bf16), the
bf16 mode of MLP and bf16 dropout.  The CPU path implements the same
contract as the HIP kernels: bf16 operands, fp32 accumulation, one rounding.

Bounds (derived, elementwise, against a float64 reference of the same
bf16-representable inputs): the half-ulp of bf16 is <= 2^-8 relative; an
fp32 sum of L terms is within L * 2^-24 * sum|terms|; the factor 2 covers
the summation order."""

import pytest
import torch

from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.models import MLP
from dist_tuto_pth_amd.optim import FusedSGD

SHAPES = [(1, 1, 1), (17, 33, 15), (64, 784, 10)]
U32 = 2.0 ** -24
HALF_ULP_BF16 = 2.0 ** -8


def _inputs(B, K, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(N, generator=g)
    gy = torch.randn(B, N, generator=g).bfloat16()
    return x, w, b, gy


def _within(got, ref, bound):
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), \
        f"worst error/bound ratio {(err / bound.clamp_min(1e-300)).max():.3f}"


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("fuse_relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16])
def test_linear_bf16_cpu(shape, fuse_relu, out_dtype, x_dtype):
    B, K, N = shape
    xb, wb, b, gy = _inputs(B, K, N)
    # master weight fp32; its value is bf16-representable, so the float64
    # reference of the same numbers is exact
    x = xb.to(x_dtype).requires_grad_(True)
    w = wb.float().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    out = ops.linear_bf16(x, w, b, fuse_relu=fuse_relu, out_dtype=out_dtype)
    assert out.dtype == out_dtype and out.shape == (B, N)
    out.backward(gy.to(out_dtype))
    assert w.grad.dtype == torch.float32 and w.grad.shape == (N, K)
    assert b.grad.dtype == torch.float32 and b.grad.shape == (N,)
    assert x.grad.dtype == x_dtype and x.grad.shape == (B, K)

    xd, wd, bd, gd = xb.double(), wb.double(), b.detach().double(), \
        gy.double()
    ref = xd @ wd.t() + bd
    if fuse_relu:
        ref = ref.relu()
    S = xd.abs() @ wd.abs().t() + bd.abs()
    bound = 2 * K * U32 * S
    if out_dtype == torch.bfloat16:
        bound = bound + HALF_ULP_BF16 * ref.abs()
    _within(out.detach(), ref, bound)

    # the live-unit mask comes from the op's own output
    if fuse_relu:
        gd = gd * (out.detach() > 0)
    bound = 2 * N * U32 * (gd.abs() @ wd.abs())
    ref_gx = gd @ wd
    if x_dtype == torch.bfloat16:
        bound = bound + HALF_ULP_BF16 * ref_gx.abs()
    _within(x.grad, ref_gx, bound)
    _within(w.grad, gd.t() @ xd, 2 * B * U32 * (gd.abs().t() @ xd.abs()))
    _within(b.grad, gd.sum(0), 2 * B * U32 * gd.abs().sum(0))


def test_linear_bf16_cpu_rounds_fp32_operands():
    torch.manual_seed(1)
    x, w, b = torch.randn(9, 20), torch.randn(7, 20), torch.randn(7)
    a = ops.linear_bf16(x, w, b)
    c = ops.linear_bf16(x.bfloat16(), w.bfloat16(), b)
    assert torch.equal(a, c)


def test_linear_bf16_cpu_bf16_weight_grad_dtype():
    x, w, b, gy = _inputs(17, 33, 15)
    w = w.clone().requires_grad_(True)
    ops.linear_bf16(x, w, b).backward(gy)
    assert w.grad.dtype == torch.bfloat16


def test_linear_bf16_rejects_bad_arguments():
    x, w, b, _ = _inputs(4, 8, 3)
    with pytest.raises(TypeError):
        ops.linear_bf16(x, w, b, out_dtype=torch.float16)
    with pytest.raises(TypeError):
        ops.linear_bf16(x.half(), w, b)
    with pytest.raises(TypeError):
        ops.linear_bf16(x, w, b.bfloat16())
    with pytest.raises(ValueError):
        ops.linear_bf16(x, w[:, :4], b)


def _train(model, steps=30):
    g = torch.Generator().manual_seed(7)
    dev = next(model.parameters()).device
    x = torch.randn(64, 784, generator=g).to(dev)
    tgt = torch.randint(0, 10, (64,), generator=g).to(dev)
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.5)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = ops.log_softmax_nll(model.forward_logits(x), tgt)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    return losses


def test_mlp_bf16_cpu_fp32_master_and_learns():
    torch.manual_seed(0)
    model = MLP((784, 64, 10), dropout=0.0, compute_dtype=torch.bfloat16)
    losses = _train(model)
    for p in model.parameters():
        assert p.dtype == torch.float32
        assert p.grad is not None and p.grad.dtype == torch.float32
    assert losses[-1] < 0.5 * losses[0], losses


def test_mlp_compute_dtype_none_is_todays_path():
    torch.manual_seed(0)
    a = MLP((784, 64, 10), dropout=0.0)
    b = MLP((784, 64, 10), dropout=0.0, compute_dtype=None)
    b.load_state_dict(a.state_dict())
    x = torch.randn(32, 784)
    assert torch.equal(a(x), b(x))


def test_mlp_rejects_other_compute_dtypes():
    with pytest.raises(ValueError):
        MLP((8, 4, 2), compute_dtype=torch.float16)


def test_dropout_bf16_cpu():
    torch.manual_seed(0)
    x = torch.randn(1000).bfloat16()
    assert torch.equal(ops.dropout(x, p=0.0, training=True), x)
    assert torch.equal(ops.dropout(x, p=0.3, training=False), x)
    xr = x.clone().requires_grad_(True)
    y = ops.dropout(xr, p=0.25, training=True)
    assert y.dtype == torch.bfloat16
    dropped = y == 0
    assert 0 < int(dropped.sum()) < x.numel()
    kept = ~dropped
    assert torch.equal(y[kept], (x.float() * (1 / 0.75)).bfloat16()[kept])
    y.backward(torch.ones_like(y))
    assert xr.grad.dtype == torch.bfloat16
    assert torch.equal(xr.grad == 0, dropped)
