"""GPU tests of the MXFP8 path (K23, csrc/linear_fp8.hip) against the CPU
contract and float64, with test_linear_fp8_gpu.py's bound unchanged.  Inputs
carry a 2^j jitter per 32x32 square, j in [-6, 6].  Measured error/bound
ratios: profiles/linear_mxfp8_numbers.md."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dist_tuto_pth_amd import ops
    from dist_tuto_pth_amd.models import MLP
    from dist_tuto_pth_amd.optim import FusedSGD
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
U32 = 2.0 ** -24
MFMA_FACTOR = 512
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float32: U32}
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


def _jittered(R, C, g):
    j = torch.randint(-6, 7, (-(-R // 32), -(-C // 32)), generator=g)
    f = torch.ldexp(torch.ones(()), j)
    return torch.randn(R, C, generator=g) \
        * f.repeat_interleave(32, 0)[:R].repeat_interleave(32, 1)[:, :C]


def _dq(t, dtype):
    """float64 of the CPU-quantised ``t``, blocks along the last dimension"""
    return ops._mxfp8_dequantize(
        *ops.quantize_fp8(t, dtype, block=32)).double()


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dtype", [E4M3, E5M2])
@pytest.mark.parametrize("shape", [(1, 1), (17, 129), (130, 127), (64, 784)])
def test_quantiser_bits(shape, dtype, src_dtype, misaligned):
    R, C = shape
    nr, nc = -(-R // 32), -(-C // 32)
    g = torch.Generator().manual_seed(R + C)
    t = (_jittered(R, C, g) * 3e-3).to(src_dtype)
    want, want_s = ops.quantize_fp8(t, dtype, block=32)
    wantT, wantT_s = ops.quantize_fp8(t.t().contiguous(), dtype, block=32)
    off = 1 if misaligned else 0
    tg = torch.empty(R * C + 1, dtype=src_dtype,
                     device=DEV)[off:off + R * C].view(R, C)
    tg.copy_(t)
    assert tg.data_ptr() % 16 == off * t.element_size()
    q, s = ops.quantize_fp8(tg, dtype, block=32)
    assert q.dtype == dtype and q.shape == (R, C)
    assert s.dtype == torch.uint8 and s.shape == (R, nc)
    assert torch.equal(q.cpu().view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(s.cpu(), want_s)
    # both storages with their scales, and the padding of each
    qs, sq, qT, sqT, _ = ops._mxfp8_quantize_gpu(tg, dtype, want_qT=True)
    assert qs.shape[1] % 128 == 0 and qT.shape[1] % 128 == 0
    assert torch.equal(qs[:, :C].cpu(), want.view(torch.uint8))
    assert torch.equal(sq[:, :nc].cpu(), want_s)
    assert torch.equal(qT[:, :R].cpu(), wantT.view(torch.uint8))
    assert torch.equal(sqT[:, :nr].cpu(), wantT_s)
    assert not qs[:, C:].any() and not qT[:, R:].any()
    assert bool((sq[:, nc:] == 127).all()) and bool((sqT[:, nr:] == 127).all())


@pytest.mark.parametrize("product", ["out", "gx", "gw"])
def test_exact_scale_mapping(product):
    """Both operands are [16][128], +-2^j per (row, 32-block), j in {0..3}:
    every quantised element is +-2^8, the scale bytes carry the rest, and all
    products are within 2^6 of the largest, where the instruction is exact.
    So the result must EQUAL float64, or a scale went to the wrong values."""
    g = torch.Generator().manual_seed(23)
    a, b = (torch.ldexp(torch.randint(0, 2, (16, 128), generator=g) * 2. - 1,
                        torch.randint(0, 4, (16, 4), generator=g)
                        .repeat_interleave(32, 1)) for _ in range(2))
    ref = (a.double() @ b.double().t()).float()
    if product == "out":            # (B, K, N) = (16, 128, 16)
        got = ops.linear_fp8(a.to(DEV), b.to(DEV), out_dtype=torch.float32,
                             scaling="mx")
    elif product == "gx":           # (16, 16, 128): a = gy, b = w^T
        x = torch.ones(16, 16, device=DEV, requires_grad=True)
        ops.linear_fp8(x, b.t().contiguous().to(DEV), scaling="mx",
                       out_dtype=torch.float32).backward(a.to(DEV))
        got = x.grad
    else:                           # (128, 16, 16): a = gy^T, b = x^T
        w = torch.ones(16, 16, device=DEV, requires_grad=True)
        ops.linear_fp8(b.t().contiguous().to(DEV), w, scaling="mx",
                       out_dtype=torch.float32).backward(
                           a.t().contiguous().to(DEV))
        got = w.grad
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), ref)


@functools.lru_cache(maxsize=None)
def _case(B, K, N):
    """fp32 inputs (CPU), built once per shape; never modified."""
    g = torch.Generator().manual_seed(1000 * B + 10 * K + N)
    return (_jittered(B, K, g), _jittered(N, K, g) / K ** 0.5,
            torch.randn(N, generator=g), _jittered(B, N, g))


@functools.lru_cache(maxsize=None)
def _operands(B, K, N, x_dtype, w_dtype):
    """float64 dequantised x, w (blocks along K), w^T (N) and x^T (B)"""
    x, w, _, _ = _case(B, K, N)
    x, w = x.to(x_dtype), w.to(w_dtype)
    return (_dq(x, E4M3), _dq(w, E4M3), _dq(w.t().contiguous(), E4M3),
            _dq(x.t().contiguous(), E4M3))


def _within(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: worst error/bound = {ratio:.3f}")
    assert bool((err <= bound).all()), \
        f"{name}: worst error/bound ratio {ratio:.3f}"


def _run(x, w, b, gy, fuse_relu, out_dtype):
    x = x.detach().to(DEV).requires_grad_(True)
    w = w.detach().to(DEV).requires_grad_(True)
    b = b.detach().to(DEV).requires_grad_(True)
    out = ops.linear_fp8(x, w, b, fuse_relu=fuse_relu, out_dtype=out_dtype,
                         scaling="mx")
    out.backward(gy.to(DEV))
    return out.detach(), x.grad, w.grad, b.grad


def _check_grads(out, gx, gw, gb, gy, fuse_relu, wTd, xTd, B, N, hx, hw):
    # the mask comes from the kernel's own saved output
    gm = gy.float()
    if fuse_relu:
        gm = torch.where(out.cpu() > 0, gm, torch.zeros_like(gm))
    gd, gTd = _dq(gm, E5M2), _dq(gm.t().contiguous(), E5M2)
    ref_gw = gTd @ xTd.t()
    if gx is not None:
        ref_gx = gd @ wTd.t()
        _within("gx", gx, ref_gx, MFMA_FACTOR * N * U32
                * (gd.abs() @ wTd.abs().t()) + hx * ref_gx.abs())
    _within("gw", gw, ref_gw, MFMA_FACTOR * B * U32
            * (gTd.abs() @ xTd.abs().t()) + hw * ref_gw.abs())
    if gb is not None:
        _within("gb", gb, gm.double().sum(0),
                2 * B * U32 * gm.double().abs().sum(0))


@pytest.mark.parametrize("x_dtype,w_dtype", [
    (torch.bfloat16, torch.float32),    # hidden layer, fp32 master weight
    (torch.float32, torch.bfloat16)])   # fp32 input, bf16 weight
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("fuse_relu", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1), (17, 129, 15), (5, 127, 3),
                                   (130, 264, 70), (16, 1024, 256)])
def test_linear_mxfp8_bounds(shape, fuse_relu, out_dtype, x_dtype, w_dtype):
    B, K, N = shape
    x, w, b, gy = _case(B, K, N)
    gy = gy.to(out_dtype)
    out, gx, gw, gb = _run(x.to(x_dtype), w.to(w_dtype), b, gy, fuse_relu,
                           out_dtype)
    assert out.dtype == out_dtype and out.shape == (B, N)
    assert gx.dtype == x_dtype and gx.shape == (B, K)
    assert gw.dtype == w_dtype and gw.shape == (N, K)
    assert gb.dtype == torch.float32 and gb.shape == (N,)
    xd, wd, wTd, xTd = _operands(B, K, N, x_dtype, w_dtype)
    ref = xd @ wd.t() + b.double()
    S = xd.abs() @ wd.abs().t() + b.double().abs()
    if fuse_relu:
        ref = ref.relu()
    _within("out", out, ref,
            MFMA_FACTOR * K * U32 * S + HALF_ULP[out_dtype] * ref.abs())
    _check_grads(out, gx, gw, gb, gy, fuse_relu, wTd, xTd, B, N,
                 HALF_ULP[x_dtype], HALF_ULP[w_dtype])


@pytest.mark.parametrize("shape", [(130, 264, 70), (4096, 33, 15)])
def test_bitwise_reproducible(shape):
    # (4096, 33, 15) splits the weight gradient's reduction
    B, K, N = shape
    if B >= 4096:
        assert load_native("_kernels").linear_fp8_gw_splits(B, K, N) > 1
    g = torch.Generator().manual_seed(11)
    x = _jittered(B, K, g).bfloat16()
    w = _jittered(N, K, g) / K ** 0.5
    b = torch.randn(N, generator=g)
    gy = _jittered(B, N, g).bfloat16()
    r1 = _run(x, w, b, gy, True, torch.bfloat16)
    r2 = _run(x, w, b, gy, True, torch.bfloat16)
    for a, c in zip(r1, r2):
        assert torch.equal(a, c)
    # and the split result is right, not just repeatable
    _check_grads(r1[0], None, r1[2], None, gy, True, None,
                 _dq(x.t().contiguous(), E4M3), B, N, 0.0, U32)


def test_mlp_mxfp8_gpu():
    torch.manual_seed(0)
    model = MLP((784, 200, 10), compute_dtype=E4M3, fp8_scaling="mx").cuda()
    model.load_state_dict(MLP((784, 200, 10)).state_dict())
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, 784, generator=g).to(DEV)
    tgt = torch.randint(0, 10, (64,), generator=g).to(DEV)
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.5)
    losses = []
    for step in range(21):
        opt.zero_grad()
        loss = ops.log_softmax_nll(model.forward_logits(x), tgt)
        loss.backward()
        if step == 0:
            for p in model.parameters():
                assert p.dtype == torch.float32
                assert p.grad.dtype == torch.float32
                assert bool(torch.isfinite(p.grad).all())
        losses.append(float(loss.detach()))
        opt.step()
    assert losses[-1] < losses[0], losses
