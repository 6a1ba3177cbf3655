"""CPU tests of the fp8 linear contract (ops.quantize_fp8, ops.linear_fp8):
the power-of-two scale rule at its edges, and the torch fallback against
the float64 product of its own dequantised operands."""

import math

import pytest
import torch

from dist_tuto_pth_amd import ops

U32 = 2.0 ** -24
FORMATS = [(torch.float8_e4m3fn, 8), (torch.float8_e5m2, 15)]


def _above(v):
    return float(torch.nextafter(torch.tensor(v), torch.tensor(math.inf)))


# (amax, e of amax = f * 2^e, f > 1.75)
EDGES = [(1.75 * 2.0 ** e, e, False) for e in (-130, -20, 0, 9, 120)] \
    + [(_above(1.75 * 2.0 ** e), e, True) for e in (-20, 0, 9)] \
    + [(2.0 ** e, e, False) for e in (-126, -3, 0, 127)]


@pytest.mark.parametrize("dtype,E", FORMATS)
@pytest.mark.parametrize("amax,e,over", EDGES)
def test_scale_rule_edges(dtype, E, amax, e, over):
    fmax = 1.75 * 2.0 ** E
    q, s = ops.quantize_fp8(torch.tensor([amax / 3, -amax]), dtype)
    k = E - e - (1 if over else 0)
    assert s.dtype == torch.float32 and s.dim() == 0
    assert float(s) == 2.0 ** min(126, max(-126, k))
    assert amax * float(s) <= fmax
    if -126 <= k <= 126:     # the largest such power of two
        assert amax * 2 * float(s) > fmax
    assert bool(torch.isfinite(q.float()).all())


@pytest.mark.parametrize("dtype,E", FORMATS)
def test_scale_rule_subnormal_and_zero(dtype, E):
    _, s = ops.quantize_fp8(torch.tensor([1e-40, -3e-41]), dtype)
    assert float(s) == 2.0 ** 126
    q, s = ops.quantize_fp8(torch.zeros(3), dtype)
    assert float(s) == 1.0 and q.dtype == dtype
    assert bool((q.view(torch.uint8) == 0).all())


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("fuse_relu", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1), (17, 129, 15), (64, 784, 10)])
def test_cpu_fallback_against_float64(shape, fuse_relu, out_dtype):
    """Bound: an fp32 sum of L exact products is within L * 2^-24 *
    sum|terms| in any order (the factor 2 covers the bias add), plus the
    half-ulp of the one output rounding."""
    B, K, N = shape
    g = torch.Generator().manual_seed(100 * B + N)
    x = torch.randn(B, K, generator=g).bfloat16().requires_grad_(True)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).requires_grad_(True)
    b = torch.randn(N, generator=g).requires_grad_(True)
    gy = torch.randn(B, N, generator=g).to(out_dtype)
    out = ops.linear_fp8(x, w, b, fuse_relu=fuse_relu, out_dtype=out_dtype)
    out.backward(gy)
    assert out.dtype == out_dtype and x.grad.dtype == torch.bfloat16
    assert w.grad.dtype == torch.float32 and b.grad.dtype == torch.float32

    half = {torch.bfloat16: 2.0 ** -8, torch.float32: U32}
    e4m3, e5m2 = torch.float8_e4m3fn, torch.float8_e5m2
    (xq, sx), (wq, sw) = ops.quantize_fp8(x, e4m3), ops.quantize_fp8(w, e4m3)
    xd, wd = xq.double() / sx.double(), wq.double() / sw.double()
    ref = xd @ wd.t() + b.detach().double()
    S = xd.abs() @ wd.abs().t() + b.detach().abs().double()
    if fuse_relu:
        ref = ref.relu()

    def within(got, want, bound):
        assert bool(((got.detach().double() - want).abs() <= bound).all())

    within(out, ref, 2 * K * U32 * S + half[out_dtype] * ref.abs())
    gm = gy.float()
    if fuse_relu:
        gm = torch.where(out.detach() > 0, gm, torch.zeros_like(gm))
    gq, sg = ops.quantize_fp8(gm, e5m2)
    gd = gq.double() / sg.double()
    ref_gx = gd @ wd
    within(x.grad, ref_gx, 2 * N * U32 * (gd.abs() @ wd.abs())
           + half[torch.bfloat16] * ref_gx.abs())
    ref_gw = gd.t() @ xd
    within(w.grad, ref_gw, 2 * B * U32 * (gd.abs().t() @ xd.abs())
           + U32 * ref_gw.abs())
    within(b.grad, gm.double().sum(0), 2 * B * U32 * gm.double().abs().sum(0))


def test_argument_checks_and_mlp_mode():
    from dist_tuto_pth_amd.models import MLP
    with pytest.raises(TypeError, match="quantize_fp8"):
        ops.quantize_fp8(torch.ones(3), torch.bfloat16)
    with pytest.raises(ValueError, match="linear_fp8"):
        ops.linear_fp8(torch.ones(2, 3), torch.ones(4, 5))
    with pytest.raises(TypeError, match="linear_fp8"):
        ops.linear_fp8(torch.ones(2, 3).half(), torch.ones(4, 3))
    with pytest.raises(ValueError, match="compute_dtype"):
        MLP((8, 4, 2), compute_dtype=torch.float16)
    torch.manual_seed(0)
    model = MLP((8, 4, 2), dropout=0.0, compute_dtype=torch.float8_e4m3fn)
    model.load_state_dict(MLP((8, 4, 2)).state_dict())
    model(torch.randn(5, 8)).sum().backward()
    assert all(p.grad.dtype == torch.float32 for p in model.parameters())
