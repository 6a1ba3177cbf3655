"""CPU tests of the MXFP8 contract (ops.quantize_fp8(block=32),
ops.linear_fp8(scaling="mx")): the per-block scale rule recomputed in
float64, and the torch fallback against the float64 product of its own
dequantised operands."""

import math

import pytest
import torch

from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.models import MLP

U32 = 2.0 ** -24
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
FORMATS = [(E4M3, 8), (E5M2, 15)]


@pytest.mark.parametrize("dtype,E", FORMATS)
@pytest.mark.parametrize("shape", [(1, 1), (3, 33), (5, 127)])
def test_block_quantiser_against_the_rule(shape, dtype, E):
    R, C = shape
    g = torch.Generator().manual_seed(R + C)
    t = torch.randn(R, C, generator=g)
    # neighbouring blocks of very different size, and one all-zero block
    nb = -(-C // 32)
    j = torch.randint(-6, 7, (R, nb), generator=g)
    t = t * torch.ldexp(torch.ones(()), j).repeat_interleave(32, 1)[:, :C]
    if nb > 1:
        t[0, :32] = 0
    q, sc = ops.quantize_fp8(t, dtype, block=32)
    assert q.dtype == dtype and q.shape == (R, C)
    assert sc.dtype == torch.uint8 and sc.shape == (R, nb)
    assert nb == 1 or int(sc[0, 0]) == 127
    assert int(sc.min()) >= 1 and int(sc.max()) <= 253
    assert float(q.float().abs().max()) <= 1.75 * 2.0 ** E
    for r in range(R):
        for c in range(0, C, 32):
            blk = t[r, c:c + 32]
            amax = float(blk.abs().max())
            k = 0
            if amax > 0:
                e = math.floor(math.log2(amax))
                k = E - e - (1 if amax / 2.0 ** e > 1.75 else 0)
                k = min(126, max(-126, k))
            assert int(sc[r, c // 32]) == 127 - k
            want = (blk * 2.0 ** k).to(dtype)
            assert torch.equal(q[r, c:c + 32].view(torch.uint8),
                               want.view(torch.uint8))


def test_cpu_mx_linear_against_float64():
    """An fp32 sum of L products is within L * 2^-24 * sum|terms| (factor 2
    for the bias add), plus the half-ulp of the one output rounding."""
    B, K, N = 17, 129, 15
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, K, generator=g).requires_grad_(True)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).requires_grad_(True)
    b = torch.randn(N, generator=g).requires_grad_(True)
    gy = torch.randn(B, N, generator=g)
    out = ops.linear_fp8(x, w, b, fuse_relu=True, out_dtype=torch.float32,
                         scaling="mx")
    out.backward(gy)

    def dq(t, dtype):   # float64 dequantised copy, blocks along the last dim
        q, sc = ops.quantize_fp8(t, dtype, block=32)
        f = torch.ldexp(torch.ones((), dtype=torch.float64),
                        sc.to(torch.int32) - 127)
        return q.double() * f.repeat_interleave(32, -1)[..., :t.shape[-1]]

    def within(got, want, bound, half_ulp=U32):
        assert bool(((got.detach().double() - want).abs()
                     <= bound + half_ulp * want.abs()).all())

    xd, wd = dq(x.detach(), E4M3), dq(w.detach(), E4M3)
    within(out, (xd @ wd.t() + b.detach().double()).relu(),
           2 * K * U32 * (xd.abs() @ wd.abs().t() + b.detach().abs().double()))
    gm = torch.where(out.detach() > 0, gy, torch.zeros(()))
    gd, wTd = dq(gm, E5M2), dq(w.detach().t(), E4M3)
    within(x.grad, gd @ wTd.t(), 2 * N * U32 * (gd.abs() @ wTd.abs().t()))
    gTd, xTd = dq(gm.t(), E5M2), dq(x.detach().t(), E4M3)
    within(w.grad, gTd @ xTd.t(), 2 * B * U32 * (gTd.abs() @ xTd.abs().t()))
    within(b.grad, gm.double().sum(0), 2 * B * U32 * gm.double().abs().sum(0),
           half_ulp=0)


def test_argument_errors():
    with pytest.raises(ValueError, match="block"):
        ops.quantize_fp8(torch.ones(3), E4M3, block=16)
    with pytest.raises(ValueError, match="scaling"):
        ops.linear_fp8(torch.ones(2, 3), torch.ones(4, 3), scaling="block")
    with pytest.raises(ValueError, match="fp8_scaling"):
        MLP((8, 4, 2), compute_dtype=torch.bfloat16, fp8_scaling="mx")
    with pytest.raises(ValueError, match="fp8_scaling"):
        MLP((8, 4, 2), compute_dtype=E4M3, fp8_scaling="ocp")
    torch.manual_seed(0)
    model = MLP((8, 4, 2), dropout=0.0, compute_dtype=E4M3, fp8_scaling="mx")
    model.load_state_dict(MLP((8, 4, 2)).state_dict())
    model(torch.randn(5, 8)).sum().backward()
    assert all(p.grad.dtype == torch.float32 for p in model.parameters())
