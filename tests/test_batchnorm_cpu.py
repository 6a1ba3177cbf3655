"""CPU tests of ops.batchnorm2d (the plain-torch form of the contract the
HIP kernels in csrc/batchnorm.hip implement) and of the bf16 mode of
models.resnet.  The bounds and their derivation are in tests/bn_bounds.py;
they are elementwise and derived, not tuned."""

import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn_bounds as bb  # noqa: E402
from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.models.resnet import (Bottleneck, ResNet,  # noqa: E402
                                              resnet50)

SHAPES = [(2, 3, 5, 7), (2, 5, 1, 1), (2, 3, 2, 3), (3, 70, 4, 4),
          (4, 8, 6, 6), (2, 16, 14, 14), (5, 4, 7, 7), (64, 2, 20, 20)]
OFFSET_SHAPES = [(2, 3, 5, 7), (4, 8, 6, 6), (3, 70, 4, 4)]
MODES = [(False, False), (False, True), (True, True)]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("residual,relu", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_path_meets_bounds(shape, dtype, residual, relu):
    bb.train_case(shape, dtype, residual, relu)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", OFFSET_SHAPES)
def test_cpu_path_meets_bounds_on_offset_inputs(shape, dtype):
    # a variance from E[x^2]-E[x]^2 misses Bv here by one to two orders
    bb.train_case(shape, dtype, True, True,
                offset=100.0 if dtype == torch.float32 else 16.0)


@pytest.mark.parametrize("residual,relu", MODES)
@pytest.mark.parametrize("training", [True, False])
def test_formulas_agree_with_torch_autograd_in_float64(training, residual,
                                                       relu):
    shape = (4, 8, 6, 6)
    x, gamma, beta, res, gy = bb.make_case(shape, torch.float32, residual)
    C = shape[1]
    g = torch.Generator().manual_seed(3)
    rm0 = torch.randn(C, generator=g)
    rv0 = 0.5 + torch.rand(C, generator=g)

    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
    rt = res.clone().requires_grad_(True) if residual else None
    y = ops.batchnorm2d(*leaves, rm0.clone(), rv0.clone(), training=training,
                        momentum=0.1, eps=bb.EPS, residual=rt,
                        fuse_relu=relu)
    y.backward(gy)

    dl = [t.double().clone().requires_grad_(True) for t in (x, gamma, beta)]
    rd = res.double().clone().requires_grad_(True) if residual else None
    yd = F.batch_norm(dl[0], rm0.double(), rv0.double(), dl[1], dl[2],
                      training, 0.1, bb.EPS)
    if residual:
        yd = yd + rd
    if relu:
        yd = F.relu(yd)
    yd.backward(gy.double())

    if training:
        By = bb.forward_reference(x, gamma, beta, res, relu)["By"]
    else:
        _, By = bb.eval_forward_reference(x, gamma, beta, rm0, rv0, res,
                                          relu)
    bb.within("y", y, yd.detach(), By)
    pairs = [("gx", leaves[0].grad, dl[0].grad),
             ("gweight", leaves[1].grad, dl[1].grad),
             ("gbias", leaves[2].grad, dl[2].grad)]
    if residual:
        pairs.append(("gres", rt.grad, rd.grad))
    for name, got, want in pairs:
        tol = 1e-4 * float(want.abs().max())
        assert float((got.double() - want).abs().max()) <= tol, name


def test_running_statistics_match_nn_batchnorm2d():
    x, gamma, beta, _, _ = bb.make_case((4, 8, 6, 6), torch.float32, False)
    bn = nn.BatchNorm2d(8, momentum=0.3)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(8, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(8, generator=g))
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    for step in range(2):
        xs = x + step
        want = bn(xs)
        got = ops.batchnorm2d(xs, gamma, beta, rm, rv, training=True,
                              momentum=0.3, eps=bn.eps)
        torch.testing.assert_close(got, want.detach(), rtol=1e-5, atol=1e-5)
        # includes the unbiased n/(n-1) factor
        torch.testing.assert_close(rm, bn.running_mean, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(rv, bn.running_var, rtol=1e-6, atol=1e-6)
    # no running buffers: nothing to update, same output
    got2 = ops.batchnorm2d(x + 1, gamma, beta, training=True)
    assert torch.equal(got2, got)


@pytest.mark.parametrize("residual,relu", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_mode(dtype, residual, relu):
    bb.eval_case((3, 70, 4, 4), dtype, residual, relu, "cpu")


def test_argument_checks():
    x = torch.randn(2, 3, 4, 4)
    w, b = torch.ones(3), torch.zeros(3)
    rm, rv = torch.zeros(3), torch.ones(3)
    with pytest.raises(TypeError, match="batchnorm2d"):
        ops.batchnorm2d(x.half(), w, b)
    with pytest.raises(TypeError, match="batchnorm2d"):
        ops.batchnorm2d(x.double(), w, b)
    with pytest.raises(ValueError, match="B,C,H,W"):
        ops.batchnorm2d(x[0], w, b)
    with pytest.raises(TypeError, match="weight"):
        ops.batchnorm2d(x, w.bfloat16(), b)
    with pytest.raises(TypeError, match="bias"):
        ops.batchnorm2d(x, w, b.double())
    with pytest.raises(ValueError, match="weight"):
        ops.batchnorm2d(x, torch.ones(4), b)
    with pytest.raises(ValueError, match="bias"):
        ops.batchnorm2d(x, w, torch.zeros(3, 1))
    with pytest.raises(ValueError, match="both"):
        ops.batchnorm2d(x, w, b, rm, None)
    with pytest.raises(ValueError, match="both"):
        ops.batchnorm2d(x, w, b, None, rv)
    with pytest.raises(TypeError, match="running_mean"):
        ops.batchnorm2d(x, w, b, rm.double(), rv)
    with pytest.raises(ValueError, match="running_var"):
        ops.batchnorm2d(x, w, b, rm, torch.ones(2))
    with pytest.raises(TypeError, match="residual"):
        ops.batchnorm2d(x, w, b, residual=x.bfloat16())
    with pytest.raises(ValueError, match="residual"):
        ops.batchnorm2d(x, w, b, residual=x[:, :, :2])
    with pytest.raises(ValueError, match="more than one value"):
        ops.batchnorm2d(torch.randn(1, 3, 1, 1), w, b, training=True)
    # ... which eval mode accepts
    ops.batchnorm2d(torch.randn(1, 3, 1, 1), w, b, rm, rv, training=False)
    with pytest.raises(ValueError, match="training=False"):
        ops.batchnorm2d(x, w, b, training=False)
    with pytest.raises(ValueError, match="not supported"):
        ops.batchnorm2d(x, w, b, rm, rv, momentum=None)
    for bad in (-0.1, 1.5, "0.1", True):
        with pytest.raises(ValueError, match="momentum"):
            ops.batchnorm2d(x, w, b, rm, rv, momentum=bad)


# ---------------------------------------------------------------------------
# models.resnet in bf16 mode
# ---------------------------------------------------------------------------
def test_compute_dtype_is_checked():
    with pytest.raises(ValueError, match="compute_dtype"):
        resnet50(compute_dtype=torch.float16)
    with pytest.raises(ValueError, match="compute_dtype"):
        ResNet((1, 1, 1, 1), compute_dtype=torch.float32)
    with pytest.raises(ValueError, match="compute_dtype"):
        Bottleneck(64, 16, compute_dtype=torch.float16)


def test_state_dict_round_trips_between_modes():
    torch.manual_seed(0)
    a = ResNet((1, 1, 1, 1), num_classes=10)
    b = ResNet((1, 1, 1, 1), num_classes=10, compute_dtype=torch.bfloat16)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype
               for k in sa)
    b.load_state_dict(sa)
    assert all(torch.equal(v, sa[k]) for k, v in b.state_dict().items())
    a.load_state_dict(b.state_dict())


def test_tiny_resnet_bf16_forward_backward():
    torch.manual_seed(0)
    net = ResNet((1, 1, 1, 1), num_classes=10, compute_dtype=torch.bfloat16)
    net.train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 32, 32, generator=g)
    tracked = net.bn1.num_batches_tracked.clone()
    rm0 = net.bn1.running_mean.clone()
    out = net(x)
    assert out.dtype == torch.float32 and out.shape == (2, 10)
    F.cross_entropy(out, torch.tensor([1, 7])).backward()
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        assert p.grad.dtype == torch.float32, name
        assert bool(torch.isfinite(p.grad).all()), name
    assert not torch.equal(net.bn1.running_mean, rm0)
    assert torch.equal(net.bn1.num_batches_tracked, tracked)
    net.eval()
    rm1 = net.bn1.running_mean.clone()
    with torch.no_grad():
        assert net(x).dtype == torch.float32
    assert torch.equal(net.bn1.running_mean, rm1)


def test_tiny_resnet_bf16_converges_like_fp32():
    bb.check_tiny_resnet_convergence("cpu")
