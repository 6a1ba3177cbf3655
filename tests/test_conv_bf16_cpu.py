"""CPU tests of ops.conv2d_bf16 (the plain-torch form of the contract the
HIP kernels in csrc/conv_bf16.hip implement) and of
Net(compute_dtype=torch.bfloat16).

Bounds are the ones tests/test_linear_bf16_gpu.py derives: an fp32 sum of
L terms is within L * 2^-24 * sum|terms|, doubled for summation order; a
bf16 result adds its half-ulp, 2^-8 relative."""

import pytest
import torch
import torch.nn.functional as F

from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.models import Net
from dist_tuto_pth_amd.optim import FusedSGD

U32 = 2.0 ** -24
HALF_ULP_BF16 = 2.0 ** -8

SHAPES = [
    (2, 1, 28, 28, 10, 5, 5, 1, 0),
    (3, 10, 12, 12, 20, 5, 5, 1, 0),
    (2, 3, 9, 7, 5, 3, 3, 1, 1),
    (2, 4, 11, 10, 6, 3, 2, 2, 1),
    (2, 8, 9, 6, 4, 3, 3, (2, 1), (0, 2)),
    (2, 4, 8, 8, 6, 1, 1, 2, 0),
]


def _inputs(shape, seed=0):
    B, C, H, W, K, R, S, stride, padding = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g).bfloat16()
    w = (torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5).bfloat16()
    b = torch.randn(K, generator=g)
    out = F.conv2d(x.float(), w.float(), b, stride, padding)
    gy = torch.randn(out.shape, generator=g).bfloat16()
    return x, w, b, gy


def _within(name, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: worst error/bound = {ratio:.3f}")
    assert bool((err <= bound).all()), f"{name}: ratio {ratio:.3f}"


def _run(x, w, b, gy, stride, padding, out_dtype):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    b = b.detach().clone().requires_grad_(True)
    out = ops.conv2d_bf16(x, w, b, stride=stride, padding=padding,
                          out_dtype=out_dtype)
    out.backward(gy.to(out_dtype))
    return out.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_path_meets_bounds(shape, out_dtype):
    B, C, H, W, K, R, S, stride, padding = shape
    x, w, b, gy = _inputs(shape)
    out, gx, gw, gb = _run(x, w.float(), b, gy, stride, padding, out_dtype)
    xd, wd, bd, gd = x.double(), w.double(), b.double(), gy.double()
    ref = F.conv2d(xd, wd, bd, stride, padding)
    assert out.dtype == out_dtype and out.shape == ref.shape
    assert gx.dtype == torch.bfloat16 and gx.shape == x.shape
    assert gw.dtype == torch.float32 and gw.shape == w.shape
    assert gb.dtype == torch.float32 and gb.shape == (K,)

    Sabs = F.conv2d(xd.abs(), wd.abs(), bd.abs(), stride, padding)
    bound = 2 * (C * R * S) * U32 * Sabs
    if out_dtype == torch.bfloat16:
        bound = bound + HALF_ULP_BF16 * ref.abs()
    _within("out", out, ref, bound)

    ref_gx = torch.nn.grad.conv2d_input(x.shape, wd, gd, stride, padding)
    S_gx = torch.nn.grad.conv2d_input(x.shape, wd.abs(), gd.abs(), stride,
                                      padding)
    _within("gx", gx, ref_gx,
            HALF_ULP_BF16 * ref_gx.abs() + 2 * (K * R * S) * U32 * S_gx)
    assert bool((gx[S_gx == 0] == 0).all())
    L = B * out.shape[2] * out.shape[3]
    ref_gw = torch.nn.grad.conv2d_weight(xd, w.shape, gd, stride, padding)
    S_gw = torch.nn.grad.conv2d_weight(xd.abs(), w.shape, gd.abs(), stride,
                                       padding)
    _within("gw", gw, ref_gw, 2 * L * U32 * S_gw)
    _within("gb", gb, gd.sum((0, 2, 3)),
            2 * L * U32 * gd.abs().sum((0, 2, 3)))


def test_fp32_inputs_round_like_bf16_inputs():
    shape = (2, 4, 11, 10, 6, 3, 2, 2, 1)
    B, C, H, W, K, R, S, stride, padding = shape
    g = torch.Generator().manual_seed(5)
    x32 = torch.randn(B, C, H, W, generator=g)
    w32 = torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5
    b = torch.randn(K, generator=g)
    gy = torch.randn(B, K, 6, 6, generator=g).bfloat16()
    o1, gx1, gw1, gb1 = _run(x32, w32, b, gy, stride, padding,
                             torch.bfloat16)
    o2, gx2, gw2, gb2 = _run(x32.bfloat16(), w32.bfloat16(), b, gy, stride,
                             padding, torch.bfloat16)
    assert torch.equal(o1, o2)
    assert gx1.dtype == torch.float32 and gx2.dtype == torch.bfloat16
    assert gw1.dtype == torch.float32 and gw2.dtype == torch.bfloat16
    assert gb1.dtype == torch.float32 and gb2.dtype == torch.float32
    assert torch.equal(gx1.bfloat16(), gx2)
    assert torch.equal(gw1.bfloat16(), gw2)
    assert torch.equal(gb1, gb2)


def test_x_without_grad_and_no_bias():
    x, w, b, gy = _inputs(SHAPES[2])
    w = w.float().requires_grad_(True)
    out = ops.conv2d_bf16(x, w, None, padding=1)
    out.backward(gy)
    assert x.grad is None and w.grad is not None


def test_validation_errors():
    x = torch.zeros(2, 3, 8, 8)
    w = torch.zeros(4, 3, 3, 3)
    b = torch.zeros(4)
    with pytest.raises(TypeError, match="conv2d_bf16"):
        ops.conv2d_bf16(x.half(), w)
    with pytest.raises(TypeError, match="conv2d_bf16"):
        ops.conv2d_bf16(x, w.double())
    with pytest.raises(TypeError, match="conv2d_bf16"):
        ops.conv2d_bf16(x, w, b.bfloat16())
    with pytest.raises(TypeError, match="conv2d_bf16"):
        ops.conv2d_bf16(x, w, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="conv2d_bf16"):
        ops.conv2d_bf16(x[0], w)                       # rank
    with pytest.raises(ValueError, match="conv2d_bf16"):
        ops.conv2d_bf16(x, w[0])
    with pytest.raises(ValueError, match="channels"):
        ops.conv2d_bf16(x, torch.zeros(4, 2, 3, 3))    # C mismatch
    with pytest.raises(ValueError, match="shape"):
        ops.conv2d_bf16(x, w, torch.zeros(5))          # bias shape
    with pytest.raises(ValueError, match="does not fit"):
        ops.conv2d_bf16(x, torch.zeros(4, 3, 9, 3))    # OH < 1
    with pytest.raises(ValueError, match="does not fit"):
        ops.conv2d_bf16(x, torch.zeros(4, 3, 3, 11), padding=(0, 1))
    with pytest.raises(ValueError, match="stride"):
        ops.conv2d_bf16(x, w, stride=0)
    with pytest.raises(ValueError, match="stride"):
        ops.conv2d_bf16(x, w, stride=(1, 0))
    with pytest.raises(ValueError, match="stride"):
        ops.conv2d_bf16(x, w, stride=(1, 1, 1))
    with pytest.raises(ValueError, match="padding"):
        ops.conv2d_bf16(x, w, padding=-1)
    with pytest.raises(ValueError, match="padding"):
        ops.conv2d_bf16(x, w, padding=1.5)


def test_dimensions_past_the_index_type_raise():
    # expanded views: huge shapes, no memory; nothing may be touched
    w = torch.zeros(1, 1, 1, 1)
    x = torch.zeros(1, 1, 1, 1).expand(2 ** 16, 1, 2 ** 8, 2 ** 8)
    with pytest.raises(ValueError, match="32-bit"):
        ops.conv2d_bf16(x, w)                          # B*H*W = 2^32
    x = torch.zeros(1, 1, 1, 1).expand(2 ** 15, 1, 2 ** 8, 2 ** 8)
    with pytest.raises(ValueError, match="32-bit"):
        ops.conv2d_bf16(x, w)                          # exactly 2^31
    x = torch.zeros(1, 1, 1, 1).expand(1, 2 ** 27, 4, 4)
    w = torch.zeros(1, 1, 1, 1).expand(1, 2 ** 27, 4, 4)
    with pytest.raises(ValueError, match="32-bit"):
        ops.conv2d_bf16(x, w)                          # C*R*S = 2^31


# ---------------------------------------------------------------------------
# Net(compute_dtype=torch.bfloat16)
# ---------------------------------------------------------------------------
def learnable_batch(seed=0, B=64):
    """x = T[tgt] + 0.5*randn over ten random 28x28 templates."""
    g = torch.Generator().manual_seed(seed)
    T = torch.randn(10, 1, 28, 28, generator=g)
    tgt = torch.randint(0, 10, (B,), generator=g)
    x = T[tgt] + 0.5 * torch.randn(B, 1, 28, 28, generator=g)
    return x, tgt


def test_net_compute_dtype_argument():
    assert Net().compute_dtype is None
    assert Net(compute_dtype=None).compute_dtype is None
    with pytest.raises(ValueError, match="compute_dtype"):
        Net(compute_dtype=torch.float16)
    with pytest.raises(ValueError, match="compute_dtype"):
        Net(compute_dtype=torch.float32)
    assert list(Net(compute_dtype=torch.bfloat16).state_dict().keys()) == \
        list(Net().state_dict().keys())


def test_net_default_is_unchanged():
    torch.manual_seed(0)
    a = Net()
    b = Net(compute_dtype=None)
    b.load_state_dict(a.state_dict())
    a.eval(), b.eval()
    x, _ = learnable_batch(1, 8)
    want = F.log_softmax(a.fc2(F.relu(a.fc1(F.relu(F.max_pool2d(
        a.conv2(F.relu(F.max_pool2d(a.conv1(x), 2))), 2)).reshape(-1, 320)))),
        dim=1)
    assert torch.equal(a(x), b(x))
    assert torch.allclose(a(x), want, atol=1e-6)


def test_net_bf16_dtypes_and_forward():
    torch.manual_seed(0)
    net = Net(compute_dtype=torch.bfloat16)
    x, tgt = learnable_batch(2, 8)
    logits = net.forward_logits(x)
    assert logits.dtype == torch.float32 and logits.shape == (8, 10)
    ops.log_softmax_nll(logits, tgt).backward()
    for p in net.parameters():
        assert p.dtype == torch.float32
        assert p.grad.dtype == torch.float32
        assert bool(torch.isfinite(p.grad).all())
    net.eval()
    assert torch.equal(net(x), ops.log_softmax(net.forward_logits(x)))
    # close to the fp32 net, but not the fp32 net
    ref = Net()
    ref.load_state_dict(net.state_dict())
    ref.eval()
    with torch.no_grad():
        d = (net.forward_logits(x) - ref.forward_logits(x)).abs().max()
    assert 0 < float(d) < 0.05


def test_net_bf16_converges_cpu():
    torch.manual_seed(0)
    net = Net(compute_dtype=torch.bfloat16)
    net.train()
    x, tgt = learnable_batch(0, 64)
    opt = FusedSGD(net.parameters(), lr=0.05, momentum=0.5)
    losses = []
    for _ in range(61):
        opt.zero_grad()
        loss = ops.log_softmax_nll(net.forward_logits(x), tgt)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    print("losses", losses[0], losses[-1])
    assert losses[-1] < 0.5 * losses[0], losses


def test_fused_entry_points_reject_bf16_net():
    from dist_tuto_pth_amd.ops import fused
    net = Net(compute_dtype=torch.bfloat16)
    x, tgt = learnable_batch(0, 4)
    for fn in (fused.net_fused_step, fused.net_fused_step_fb,
               fused.net_fused_train_step, fused.net_fused_loss):
        with pytest.raises(TypeError, match="compute_dtype"):
            fn(net, x, tgt)
    with pytest.raises(TypeError, match="compute_dtype"):
        fused.net_fused_step_opt(net, x, tgt, None)
