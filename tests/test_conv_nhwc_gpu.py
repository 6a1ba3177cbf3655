"""GPU tests of the channels-last bf16 MFMA convolution
(csrc/conv_nhwc_bf16.hip) behind ops.conv2d_bf16(memory_format=
torch.channels_last).

Inputs are bf16-representable, so the reference is the float64 convolution
of the same values.  The bounds are the derived, elementwise ones of
tests/test_conv_bf16_gpu.py: the half-ulp of bf16 is <= 2^-8 relative; an
fp32 sum of L terms is within L * 2^-24 * sum|terms| under RNE; the factor 2
covers the matrix core's internal summation order and rounding."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dist_tuto_pth_amd import ops
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
U32 = 2.0 ** -24
HALF_ULP_BF16 = 2.0 ** -8
CL = torch.channels_last

SPLIT_SHAPE = (64, 8, 20, 20, 3, 3, 3, 1, 0)
HOLES_SHAPE = (2, 8, 8, 8, 6, 1, 1, 2, 0)
SHAPES = [
    # (B, C, H, W, K, R, S, stride, padding)
    (1, 8, 3, 3, 8, 3, 3, 1, 1),        # one tile, all tail, all padding
    (2, 16, 9, 7, 24, 3, 3, 1, 1),      # vector path, odd widths, padding
    (2, 3, 11, 10, 5, 7, 7, 2, 3),      # the stem: chunks straddle taps
    (2, 12, 8, 6, 6, 3, 2, (2, 1), (0, 2)),  # C % 8 != 0, pairs, far padding
    HOLES_SHAPE,                        # 1x1 stride 2: gx holes, unused edge
    (5, 72, 8, 8, 70, 1, 1, 1, 0),      # plain GEMM: M 320, N 70, k 64 + 8
    (3, 40, 6, 6, 130, 3, 3, 1, 1),     # taps change inside K tiles, 3 n tiles
    SPLIT_SHAPE,                        # L = 20736: gw splits > 1
]


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
    assert bool((err <= bound).all()), \
        f"{name}: worst error/bound ratio {ratio:.3f}"


def _run(x, w, b, gy, stride, padding, out_dtype, memory_format=CL):
    x = x.detach().to(DEV).requires_grad_(True)
    w = w.detach().to(DEV).requires_grad_(True)
    b = b.detach().to(DEV).requires_grad_(True)
    out = ops.conv2d_bf16(x, w, b, stride=stride, padding=padding,
                          out_dtype=out_dtype, memory_format=memory_format)
    # autograd.grad, not .grad: accumulation would restride gx like x
    gx, gw, gb = torch.autograd.grad(out, (x, w, b),
                                     gy.to(DEV).to(out_dtype))
    return out.detach(), gx, gw, gb


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_conv2d_nhwc_bounds(shape, out_dtype):
    B, C, H, W, K, R, S, stride, padding = shape
    x, w, b, gy, refs = _case(shape)
    if shape == SPLIT_SHAPE:
        assert load_native("_kernels").conv2d_nhwc_bf16_gw_splits(
            B, C, H, W, K, R, S, *_pair(stride), *_pair(padding)) > 1
    # bf16 activations, fp32 master weight (bf16-representable values)
    out, gx, gw, gb = _run(x, w.float(), b, gy, stride, padding, out_dtype)
    ref, Sabs = refs["out"]
    assert out.dtype == out_dtype and out.shape == ref.shape
    assert gx.dtype == torch.bfloat16 and gx.shape == x.shape
    assert gw.dtype == torch.float32 and gw.shape == w.shape
    assert gb.dtype == torch.float32 and gb.shape == (K,)
    assert out.permute(0, 2, 3, 1).is_contiguous()
    assert gx.permute(0, 2, 3, 1).is_contiguous()
    assert gw.is_contiguous()

    bound = 2 * (C * R * S) * U32 * Sabs
    if out_dtype == torch.bfloat16:
        bound = bound + HALF_ULP_BF16 * ref.abs()
    _within("out", out, ref, bound)

    ref_gx, S_gx = refs["gx"]
    _within("gx", gx, ref_gx,
            HALF_ULP_BF16 * ref_gx.abs() + 2 * (K * R * S) * U32 * S_gx)
    # inputs no output reads get an exact zero
    if shape == HOLES_SHAPE:
        assert bool((S_gx[:, :, 1::2] == 0).all())
        assert bool((S_gx[:, :, :, 7] == 0).all())
    assert bool((gx.cpu()[S_gx == 0] == 0).all())
    L = B * ref.shape[2] * ref.shape[3]
    _within("gw", gw, refs["gw"][0], 2 * L * U32 * refs["gw"][1])
    _within("gb", gb, refs["gb"][0], 2 * L * U32 * refs["gb"][1])


def test_split_shape_is_bitwise_deterministic():
    B, C, H, W, K, R, S, stride, padding = SPLIT_SHAPE
    x, w, b, gy, _ = _case(SPLIT_SHAPE)
    r1 = _run(x, w.float(), b, gy, stride, padding, torch.bfloat16)
    r2 = _run(x, w.float(), b, gy, stride, padding, torch.bfloat16)
    for a, c in zip(r1, r2):
        assert torch.equal(a, c)


def test_fp32_inputs_are_rounded_like_torch():
    shape = (2, 12, 8, 6, 6, 3, 2, (2, 1), (0, 2))
    B, C, H, W, K, R, S, stride, padding = shape
    g = torch.Generator().manual_seed(5)
    x32 = torch.randn(B, C, H, W, generator=g)
    w32 = torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5
    b = torch.randn(K, generator=g)
    gy = torch.randn(_case(shape)[3].shape, generator=g).bfloat16()
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


def test_storage_of_x_does_not_matter_and_format_is_checked():
    x, w, b, _, _ = _case((2, 16, 9, 7, 24, 3, 3, 1, 1))
    x, w, b = x.to(DEV), w.float().to(DEV), b.to(DEV)
    xc = x.contiguous(memory_format=CL)
    assert x.is_contiguous() and not xc.is_contiguous()
    a = ops.conv2d_bf16(x, w, b, padding=1, memory_format=CL)
    c = ops.conv2d_bf16(xc, w, b, padding=1, memory_format=CL)
    assert torch.equal(a, c)
    with pytest.raises(ValueError, match="conv2d_bf16: memory_format"):
        ops.conv2d_bf16(x, w, b, padding=1,
                        memory_format=torch.preserve_format)
