"""CPU tests of ops.maxpool2d and ops.global_avgpool2d: the plain-torch
golden paths against torch autograd and float64, on the cases and bounds of
tests/pool_cases.py (shared with tests/test_pool_gpu.py), the argument
checks, and ResNet's bf16 mode on top of them."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_cases as pc  # noqa: E402

from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.models.resnet import ResNet  # noqa: E402


@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("case", pc.MAXPOOL_CASES, ids=pc.case_id)
def test_maxpool2d_equals_torch(case, dtype):
    x, gx = pc.check_maxpool_exact(ops, case, dtype)
    if case[0] == (2, 2, 5, 5):
        # 2x2/2 windows never reach the last row and column
        assert (gx[:, :, 4, :] == 0).all() and (gx[:, :, :, 4] == 0).all()


def test_maxpool2d_equals_torch_at_the_large_case():
    pc.check_maxpool_exact(ops, pc.BIG_CASE, torch.bfloat16)


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_maxpool2d_random_gy(dtype):
    pc.check_maxpool_random_gy(ops, dtype)


@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("shape", pc.AVG_SHAPES)
def test_global_avgpool2d_bounds(shape, dtype):
    pc.check_avg(ops, shape, dtype)


def test_stride_defaults_to_kernel_size():
    x = pc.maxpool_input((2, 2, 9, 9), torch.float32)
    assert torch.equal(ops.maxpool2d(x, 3), ops.maxpool2d(x, 3, 3, 0))
    assert ops.maxpool2d(x, (3, 2)).shape == (2, 2, 3, 4)


def test_non_contiguous_input():
    x = pc.maxpool_input((2, 3, 7, 9), torch.float32)
    xn = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not xn.is_contiguous()
    assert torch.equal(ops.maxpool2d(xn, 3, 2, 1), ops.maxpool2d(x, 3, 2, 1))
    assert torch.equal(ops.global_avgpool2d(xn), ops.global_avgpool2d(x))


def test_maxpool2d_argument_checks():
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(TypeError, match="maxpool2d"):
        ops.maxpool2d(x.half(), 3)
    with pytest.raises(ValueError, match=r"maxpool2d.*\[B,C,H,W\]"):
        ops.maxpool2d(x[0], 3)
    with pytest.raises(ValueError, match="maxpool2d.*>= 1"):
        ops.maxpool2d(x[:, :, :0], 3)
    with pytest.raises(ValueError, match="maxpool2d: kernel_size"):
        ops.maxpool2d(x, 0)
    with pytest.raises(ValueError, match="maxpool2d: kernel_size"):
        ops.maxpool2d(x, (3, 3, 3))
    with pytest.raises(ValueError, match="maxpool2d: kernel_size"):
        ops.maxpool2d(x, 2.0)
    with pytest.raises(ValueError, match="maxpool2d: stride"):
        ops.maxpool2d(x, 3, 0)
    with pytest.raises(ValueError, match="maxpool2d: padding"):
        ops.maxpool2d(x, 3, 2, -1)
    with pytest.raises(ValueError, match="maxpool2d: padding.*half"):
        ops.maxpool2d(x, 3, 2, 2)
    with pytest.raises(ValueError, match="maxpool2d: padding.*half"):
        ops.maxpool2d(x, (3, 2), 2, (1, 2))
    with pytest.raises(ValueError, match="maxpool2d.*256"):
        ops.maxpool2d(torch.zeros(1, 1, 20, 20), 17)
    with pytest.raises(ValueError, match="maxpool2d.*does not fit"):
        ops.maxpool2d(x, 11, 1, 1)
    # 16x16 = 256 positions is the largest window
    assert ops.maxpool2d(torch.zeros(1, 1, 20, 20), 16, 1).shape == \
        (1, 1, 5, 5)


def test_global_avgpool2d_argument_checks():
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(TypeError, match="global_avgpool2d"):
        ops.global_avgpool2d(x.double())
    with pytest.raises(ValueError, match=r"global_avgpool2d.*\[B,C,H,W\]"):
        ops.global_avgpool2d(x[0])
    with pytest.raises(ValueError, match="global_avgpool2d.*>= 1"):
        ops.global_avgpool2d(x[:, :0])


def test_conv_pair_messages_are_unchanged():
    x, w = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 3, 3)
    with pytest.raises(ValueError, match="^conv2d_bf16: stride must be >= 1"):
        ops.conv2d_bf16(x, w, stride=0)
    with pytest.raises(ValueError,
                       match="^conv2d_bf16: padding must be an int or"):
        ops.conv2d_bf16(x, w, padding=True)


def test_tiny_resnet_bf16_runs_on_the_pool_ops():
    torch.manual_seed(0)
    model = ResNet((1, 1, 1, 1), num_classes=10,
                   compute_dtype=torch.bfloat16)
    calls = []
    real_max, real_avg = ops.maxpool2d, ops.global_avgpool2d

    def spy_max(x, *a, **kw):
        calls.append(("max", tuple(x.shape), a))
        return real_max(x, *a, **kw)

    def spy_avg(x):
        calls.append(("avg", tuple(x.shape)))
        return real_avg(x)

    ops.maxpool2d, ops.global_avgpool2d = spy_max, spy_avg
    try:
        out = model(torch.randn(2, 3, 32, 32))
        out.sum().backward()
    finally:
        ops.maxpool2d, ops.global_avgpool2d = real_max, real_avg
    assert calls == [("max", (2, 64, 16, 16), (3, 2, 1)),
                     ("avg", (2, 2048, 1, 1))]
    assert out.dtype == torch.float32 and out.shape == (2, 10)
    names = dict(model.named_parameters())
    assert "maxpool" in dict(model.named_children())
    assert "avgpool" in dict(model.named_children())
    for n, p in names.items():
        assert p.grad is not None and p.grad.dtype == torch.float32, n
        assert torch.isfinite(p.grad).all(), n
