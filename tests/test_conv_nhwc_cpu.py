"""CPU tests of ops.conv2d_bf16(memory_format=torch.channels_last): the
plain-torch form of the contract csrc/conv_nhwc_bf16.hip implements gives
the default call's values, in channels-last storage."""

import pytest
import torch

from dist_tuto_pth_amd import ops


def _run(shape, **kw):
    B, C, H, W, K, R, S, stride, padding = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g).requires_grad_(True)
    w = (torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5) \
        .requires_grad_(True)
    b = torch.randn(K, generator=g).requires_grad_(True)
    out = ops.conv2d_bf16(x, w, b, stride=stride, padding=padding, **kw)
    # autograd.grad, not .grad: accumulation would restride gx like x
    gy = torch.randn(out.shape, generator=g).bfloat16()
    return (out.detach(),) + torch.autograd.grad(out, (x, w, b), gy)


@pytest.mark.parametrize("shape", [
    (2, 3, 11, 10, 5, 7, 7, 2, 3),     # the stem in small
    (2, 8, 8, 8, 6, 1, 1, 2, 0),       # 1x1 stride 2
])
def test_channels_last_gives_the_default_values(shape):
    ref = _run(shape)
    got = _run(shape, memory_format=torch.channels_last)
    for r, g in zip(ref, got):
        assert g.dtype == r.dtype and g.shape == r.shape
        assert torch.equal(g, r)
    out, gx, gw, _ = got
    assert out.permute(0, 2, 3, 1).is_contiguous()
    assert gx.permute(0, 2, 3, 1).is_contiguous()
    assert gw.is_contiguous()
