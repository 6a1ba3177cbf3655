"""GPU tests of the bf16 MFMA convolution (csrc/conv_bf16.hip), the bf16
forms of maxpool2d_relu and dropout2d, and Net(compute_dtype=bfloat16).

Inputs are bf16-representable, so the reference is the float64 convolution
of the same values.  The bounds are derived, not measured, and elementwise,
by the rule tests/test_linear_bf16_gpu.py states: the half-ulp of bf16 is
<= 2^-8 relative; an fp32 sum of L terms is within L * 2^-24 * sum|terms|
under RNE; the factor 2 covers the matrix core's internal summation order
and rounding."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dist_tuto_pth_amd import ops
    from dist_tuto_pth_amd.models import Net
    from dist_tuto_pth_amd.optim import FusedSGD
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
U32 = 2.0 ** -24
HALF_ULP_BF16 = 2.0 ** -8

SPLIT_SHAPE = (64, 2, 20, 20, 3, 3, 3, 1, 0)
SHAPES = [
    # (B, C, H, W, K, R, S, stride, padding)
    (1, 1, 5, 5, 1, 5, 5, 1, 0),       # 1x1 output, everything is tail
    (2, 1, 28, 28, 10, 5, 5, 1, 0),    # Net conv1: reduction 25 < a k-step
    (3, 10, 12, 12, 20, 5, 5, 1, 0),   # Net conv2: 250 = 3 tiles + tail
    (2, 3, 9, 7, 5, 3, 3, 1, 1),       # padding, odd widths
    (2, 4, 11, 10, 6, 3, 2, 2, 1),     # stride 2, non-square filter
    (2, 8, 9, 6, 4, 3, 3, (2, 1), (0, 2)),  # pairs, padding > filter reach
    (2, 4, 8, 8, 6, 1, 1, 2, 0),       # 1x1 stride 2: gx holes, unused edge
    (5, 16, 8, 8, 70, 1, 1, 1, 0),     # N > 64, M = 320: several tiles
    SPLIT_SHAPE,                       # M = 20736: gw splits > 1
]


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """bf16 inputs (CPU) and the float64 references, built once per shape
    and shared by every test of that shape; never modified."""
    B, C, H, W, K, R, S, stride, padding = shape
    g = torch.Generator().manual_seed(sum(_pair(stride)) + 7 * B + 11 * C
                                      + 13 * H + 17 * K + 19 * R)
    x = torch.randn(B, C, H, W, generator=g).bfloat16()
    w = (torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5).bfloat16()
    b = torch.randn(K, generator=g)
    xd, wd, bd = x.double(), w.double(), b.double()
    ref = F.conv2d(xd, wd, bd, stride, padding)
    gy = torch.randn(ref.shape, generator=g).bfloat16()
    gd = gy.double()
    cin = torch.nn.grad.conv2d_input
    cw = torch.nn.grad.conv2d_weight
    refs = {
        "out": (ref, F.conv2d(xd.abs(), wd.abs(), bd.abs(), stride, padding)),
        "gx": (cin(x.shape, wd, gd, stride, padding),
               cin(x.shape, wd.abs(), gd.abs(), stride, padding)),
        "gw": (cw(xd, w.shape, gd, stride, padding),
               cw(xd.abs(), w.shape, gd.abs(), stride, padding)),
        "gb": (gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3))),
    }
    return x, w, b, gy, refs


def _within(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: worst error/bound = {ratio:.3f}")
    assert bool((err <= bound).all()), \
        f"{name}: worst error/bound ratio {ratio:.3f}"


def _run(x, w, b, gy, stride, padding, out_dtype):
    x = x.detach().to(DEV).requires_grad_(True)
    w = w.detach().to(DEV).requires_grad_(True)
    b = b.detach().to(DEV).requires_grad_(True)
    out = ops.conv2d_bf16(x, w, b, stride=stride, padding=padding,
                          out_dtype=out_dtype)
    out.backward(gy.to(DEV).to(out_dtype))
    return out.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_conv2d_bf16_bounds(shape, out_dtype):
    B, C, H, W, K, R, S, stride, padding = shape
    x, w, b, gy, refs = _case(shape)
    if shape == SPLIT_SHAPE:
        assert load_native("_kernels").conv2d_bf16_gw_splits(
            B, C, H, W, K, R, S, *_pair(stride), *_pair(padding)) > 1
    # bf16 activations, fp32 master weight (bf16-representable values)
    out, gx, gw, gb = _run(x, w.float(), b, gy, stride, padding, out_dtype)
    ref, Sabs = refs["out"]
    assert out.dtype == out_dtype and out.shape == ref.shape
    assert gx.dtype == torch.bfloat16 and gx.shape == x.shape
    assert gw.dtype == torch.float32 and gw.shape == w.shape
    assert gb.dtype == torch.float32 and gb.shape == (K,)

    bound = 2 * (C * R * S) * U32 * Sabs
    if out_dtype == torch.bfloat16:
        bound = bound + HALF_ULP_BF16 * ref.abs()
    _within("out", out, ref, bound)

    ref_gx, S_gx = refs["gx"]
    _within("gx", gx, ref_gx,
            HALF_ULP_BF16 * ref_gx.abs() + 2 * (K * R * S) * U32 * S_gx)
    # inputs no output reads get an exact zero
    assert bool((gx.cpu()[S_gx == 0] == 0).all())
    L = B * ref.shape[2] * ref.shape[3]
    _within("gw", gw, refs["gw"][0], 2 * L * U32 * refs["gw"][1])
    _within("gb", gb, refs["gb"][0], 2 * L * U32 * refs["gb"][1])


def test_stride_holes_exist_in_the_1x1_case():
    # the exact-zero check above is not vacuous for the shape meant for it
    _, _, _, _, refs = _case((2, 4, 8, 8, 6, 1, 1, 2, 0))
    holes = refs["gx"][1] == 0
    assert bool(holes[:, :, 1::2].all()) and bool(holes[:, :, :, 7].all())


def test_fp32_inputs_are_rounded_like_torch():
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
    # one rounding each: fp32 -> bf16 of the fp32 result is the bf16 result
    assert torch.equal(gx1.bfloat16(), gx2)
    assert torch.equal(gw1.bfloat16(), gw2)
    assert torch.equal(gb1, gb2)


def test_split_shape_is_bitwise_deterministic():
    B, C, H, W, K, R, S, stride, padding = SPLIT_SHAPE
    x, w, b, gy, _ = _case(SPLIT_SHAPE)
    r1 = _run(x, w.float(), b, gy, stride, padding, torch.bfloat16)
    r2 = _run(x, w.float(), b, gy, stride, padding, torch.bfloat16)
    for a, c in zip(r1, r2):
        assert torch.equal(a, c)


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
def test_non_contiguous_x(x_dtype):
    x, w, b, _, _ = _case((2, 3, 9, 7, 5, 3, 3, 1, 1))
    xt = x.to(x_dtype).to(DEV).permute(0, 1, 3, 2).contiguous()
    xn = xt.permute(0, 1, 3, 2)
    assert not xn.is_contiguous()
    w, b = w.float().to(DEV), b.to(DEV)
    a = ops.conv2d_bf16(xn, w, b, padding=1)
    c = ops.conv2d_bf16(xn.contiguous(), w, b, padding=1)
    assert torch.equal(a, c)


def test_x_without_grad_skips_gx():
    x, w, b, gy, _ = _case((2, 3, 9, 7, 5, 3, 3, 1, 1))
    x = x.to(DEV)
    w = w.float().to(DEV).requires_grad_(True)
    out = ops.conv2d_bf16(x, w, b.to(DEV), padding=1)
    out.backward(gy.to(DEV))
    assert x.grad is None and w.grad is not None


def test_gpu_dtype_guards():
    x = torch.randn(2, 3, 8, 8, device=DEV)
    with pytest.raises(TypeError, match="conv2d_bf16"):
        ops.conv2d_bf16(x.half(), torch.randn(4, 3, 3, 3, device=DEV))
    with pytest.raises(TypeError, match="maxpool2d_relu"):
        ops.maxpool2d_relu(x.half())
    with pytest.raises(TypeError, match="dropout2d"):
        ops.dropout2d(x.half())
    with pytest.raises(ValueError, match="even"):
        ops.maxpool2d_relu(x.bfloat16()[:, :, :7])
    with pytest.raises(ValueError, match="even"):
        ops.maxpool2d_relu(x.bfloat16()[:, :, :, :5])


def test_maxpool2d_relu_bf16_matches_fp32():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(3, 5, 12, 8, generator=g).bfloat16()
    x[0, 1] = -x[0, 1].abs() - 1         # planes that are all negative
    x[2, 4] = -x[2, 4].abs() - 1
    gy = torch.randn(3, 5, 6, 4, generator=g).bfloat16()
    gy[gy == 0] = 1.0
    xb = x.to(DEV).requires_grad_(True)
    xf = x.float().to(DEV).requires_grad_(True)
    yb = ops.maxpool2d_relu(xb)
    yf = ops.maxpool2d_relu(xf)
    assert yb.dtype == torch.bfloat16
    assert torch.equal(yb.detach(), yf.detach().bfloat16())
    assert torch.equal(yb.detach().float(), yf.detach())
    assert bool((yb[0, 1] == 0).all()) and bool((yb[2, 4] == 0).all())
    yb.backward(gy.to(DEV))
    yf.backward(gy.float().to(DEV))
    assert xb.grad.dtype == torch.bfloat16
    assert torch.equal(xb.grad, xf.grad.bfloat16())
    assert torch.equal(xb.grad.float(), xf.grad)


def test_dropout2d_bf16_matches_fp32_mask():
    B, C, H, W, p = 37, 29, 6, 5, 0.3
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, C, H, W, generator=g).bfloat16()
    x[x == 0] = 1.0
    x = x.to(DEV)
    ops._seed_ptr(torch.device(DEV))    # make sure the seed buffer exists
    seed = ops._seed_bufs[0]

    seed.fill_(12345)
    y32 = ops.dropout2d(x.float(), p=p, training=True)
    seed_after_fp32 = int(seed.item())
    seed.fill_(12345)
    xb = x.clone().requires_grad_(True)
    y = ops.dropout2d(xb, p=p, training=True)
    assert int(seed.item()) == seed_after_fp32 != 12345
    assert y.dtype == torch.bfloat16
    keep = y32 != 0
    planes = keep.flatten(2).all(2) | ~keep.flatten(2).any(2)
    assert bool(planes.all())            # whole channels
    assert 0.63 < float(keep.float().mean()) < 0.77
    assert torch.equal(y != 0, keep)
    # the forward scales by 1/(1-p) evaluated in fp32, as the fp32 op does
    scale = float(1.0 / (1.0 - torch.tensor(p, dtype=torch.float32)))
    want = torch.where(keep, (x.float() * scale).bfloat16(),
                       torch.zeros_like(x))
    assert torch.equal(y.detach(), want)

    gy = torch.randn(B, C, H, W, generator=g).bfloat16().to(DEV)
    gy[gy == 0] = 1.0
    y.backward(gy)
    assert xb.grad.dtype == torch.bfloat16
    # the backward by the double 1/(1-p) rounded to fp32, likewise
    want = torch.where(keep, (gy.float() * (1.0 / (1.0 - p))).bfloat16(),
                       torch.zeros_like(gy))
    assert torch.equal(xb.grad, want)


# ---------------------------------------------------------------------------
# Net(compute_dtype=torch.bfloat16)
# ---------------------------------------------------------------------------
def _learnable_batch(seed=0, B=64):
    g = torch.Generator().manual_seed(seed)
    T = torch.randn(10, 1, 28, 28, generator=g)
    tgt = torch.randint(0, 10, (B,), generator=g)
    x = T[tgt] + 0.5 * torch.randn(B, 1, 28, 28, generator=g)
    return x.to(DEV), tgt.to(DEV)


def test_net_bf16_eval_is_the_ops_chained_by_hand():
    torch.manual_seed(0)
    net = Net(compute_dtype=torch.bfloat16).cuda().eval()
    x, _ = _learnable_batch(3, 9)
    bf16 = torch.bfloat16
    h = ops.conv2d_bf16(x, net.conv1.weight, net.conv1.bias)
    assert h.dtype == bf16
    h = ops.maxpool2d_relu(h)
    h = ops.conv2d_bf16(h, net.conv2.weight, net.conv2.bias)
    h = ops.maxpool2d_relu(h)
    assert h.dtype == bf16 and h.shape == (9, 20, 4, 4)
    h = ops.linear_bf16(h.reshape(-1, 320), net.fc1.weight, net.fc1.bias,
                        fuse_relu=True)
    assert h.dtype == bf16
    want = ops.linear_bf16(h, net.fc2.weight, net.fc2.bias,
                           out_dtype=torch.float32)
    got = net.forward_logits(x)
    assert got.dtype == torch.float32 and got.shape == (9, 10)
    assert torch.equal(got, want)
    assert torch.equal(net(x), ops.log_softmax(want))


def test_net_bf16_converges_gpu():
    torch.manual_seed(0)
    net = Net(compute_dtype=torch.bfloat16).cuda()
    net.train()
    x, tgt = _learnable_batch(0, 64)
    opt = FusedSGD(net.parameters(), lr=0.05, momentum=0.5)
    losses = []
    for step in range(61):
        opt.zero_grad()
        loss = ops.log_softmax_nll(net.forward_logits(x), tgt)
        loss.backward()
        if step == 0:
            for p in net.parameters():
                assert p.dtype == torch.float32
                assert p.grad.dtype == torch.float32
                assert bool(torch.isfinite(p.grad).all())
        losses.append(float(loss.detach()))
        opt.step()
    print("losses", losses[0], losses[-1])
    assert losses[-1] < 0.5 * losses[0], losses


def test_fused_step_rejects_bf16_net():
    from dist_tuto_pth_amd.ops.fused import net_fused_step
    net = Net(compute_dtype=torch.bfloat16).cuda()
    x, tgt = _learnable_batch(0, 4)
    with pytest.raises(TypeError, match="compute_dtype"):
        net_fused_step(net, x, tgt)
