"""GPU tests of the fp8 linear kernels (csrc/linear_fp8.hip) and the fp8
mode of MLP.

The quantiser is checked bit for bit against the CPU fallback.  The GEMMs
are checked elementwise against the float64 product of the dequantised
operands, with the structure of test_linear_bf16_gpu.py's bound: an fp32
sum of L exact products is within L * 2^-24 * sum|terms|, times a factor
for the matrix core's internal summation, plus the output's half-ulp for
its one rounding.

That factor is 2 in the bf16 test.  The 128-deep fp8 instruction does not
stay inside it: it drops what lies 2^-14 or more below the largest product
it adds it to (profiles/linear_fp8_numbers.md has the probe).  With factor
2 the worst error/bound ratios measured on an MI355X were, per shape in
SHAPES order, out 0.48 0.88 0.56 0.87 0.95 0.81, gx 0 29.1 201.5 90.6 3.2
0.95, gw 0 26.4 162.9 (n/a) 0.97 60.7.  MFMA_FACTOR is the next power of
two above twice the worst of them (2 * 201.5 -> 512).  gb is a plain fp32
sum and keeps the factor 2."""

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

SHAPES = [
    (1, 1, 1),          # everything is tail and padding
    (17, 129, 15),      # K one past a 128 tile
    (5, 127, 3),        # K one short of it
    (64, 784, 10),      # the MLP's own K and N
    (130, 264, 70),     # several blocks in every dimension, B past a tile
    (16, 1024, 256),    # long K, N two tiles
]


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dtype", [E4M3, E5M2])
@pytest.mark.parametrize("shape", [(1, 1), (17, 129), (130, 127), (64, 784)])
def test_quantiser_bits(shape, dtype, src_dtype, misaligned):
    R, C = shape
    g = torch.Generator().manual_seed(R + C)
    flat = (torch.randn(R * C + 1, generator=g) * 3e-3).to(src_dtype)
    t = flat[1:].view(R, C) if misaligned else flat[:-1].view(R, C)
    want, want_s = ops.quantize_fp8(t, dtype)
    tg = flat.to(DEV)[1:].view(R, C) if misaligned \
        else flat.to(DEV)[:-1].view(R, C)
    assert tg.data_ptr() % 16 == (flat.element_size() if misaligned else 0)
    q, s = ops.quantize_fp8(tg, dtype)
    assert q.dtype == dtype and q.shape == (R, C) and s.dim() == 0
    assert torch.equal(s.cpu().view(torch.int32), want_s.view(torch.int32))
    assert torch.equal(q.cpu().view(torch.uint8), want.view(torch.uint8))
    # both storages: the transposed copy and the zero padding of each
    qs, qT, _, _ = ops._fp8_quantize_gpu(tg, dtype, want_qT=True)
    assert qs.shape[1] % 128 == 0 and qT.shape[1] % 128 == 0
    assert torch.equal(qs[:, :C].cpu(), want.view(torch.uint8))
    assert torch.equal(qT[:, :R].cpu(), want.view(torch.uint8).t())
    assert not qs[:, C:].any() and not qT[:, R:].any()


@functools.lru_cache(maxsize=None)
def _case(B, K, N):
    """fp32 inputs (CPU), built once per shape; never modified."""
    g = torch.Generator().manual_seed(1000 * B + 10 * K + N)
    x = torch.randn(B, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    gy = torch.randn(B, N, generator=g)
    return x, w, b, gy


@functools.lru_cache(maxsize=None)
def _forward_ref(B, K, N, x_dtype, w_dtype):
    """float64 forward reference from the CPU-quantised operands."""
    x, w, b, _ = _case(B, K, N)
    (xq, sx) = ops.quantize_fp8(x.to(x_dtype), E4M3)
    (wq, sw) = ops.quantize_fp8(w.to(w_dtype), E4M3)
    xd, wd = xq.double() / sx.double(), wq.double() / sw.double()
    ref = xd @ wd.t() + b.double()
    S = xd.abs() @ wd.abs().t() + b.double().abs()
    return xd, wd, ref, S


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
    out = ops.linear_fp8(x, w, b, fuse_relu=fuse_relu, out_dtype=out_dtype)
    out.backward(gy.to(DEV))
    return out.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("x_dtype,w_dtype", [
    (torch.bfloat16, torch.float32),    # hidden layer, fp32 master weight
    (torch.float32, torch.bfloat16)])   # fp32 input, bf16 weight
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("fuse_relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_linear_fp8_bounds(shape, fuse_relu, out_dtype, x_dtype, w_dtype):
    B, K, N = shape
    x, w, b, gy = _case(B, K, N)
    gy = gy.to(out_dtype)
    out, gx, gw, gb = _run(x.to(x_dtype), w.to(w_dtype), b, gy, fuse_relu,
                           out_dtype)
    assert out.dtype == out_dtype and out.shape == (B, N)
    assert gx.dtype == x_dtype and gx.shape == (B, K)
    assert gw.dtype == w_dtype and gw.shape == (N, K)
    assert gb.dtype == torch.float32 and gb.shape == (N,)

    xd, wd, ref, S = _forward_ref(B, K, N, x_dtype, w_dtype)
    if fuse_relu:
        ref = ref.relu()
    _within("out", out, ref,
            MFMA_FACTOR * K * U32 * S + HALF_ULP[out_dtype] * ref.abs())

    # the mask comes from the kernel's own saved output, so the reference
    # and the kernel agree on which units are live
    gm = gy.float()
    if fuse_relu:
        gm = torch.where(out.cpu() > 0, gm, torch.zeros_like(gm))
    gq, sg = ops.quantize_fp8(gm, E5M2)
    gd = gq.double() / sg.double()
    ref_gx, ref_gw = gd @ wd, gd.t() @ xd
    _within("gx", gx, ref_gx, MFMA_FACTOR * N * U32 * (gd.abs() @ wd.abs())
            + HALF_ULP[x_dtype] * ref_gx.abs())
    _within("gw", gw, ref_gw,
            MFMA_FACTOR * B * U32 * (gd.abs().t() @ xd.abs())
            + HALF_ULP[w_dtype] * ref_gw.abs())
    _within("gb", gb, gm.double().sum(0),
            2 * B * U32 * gm.double().abs().sum(0))


@pytest.mark.parametrize("shape", [(130, 264, 70), (4096, 33, 15)])
def test_bitwise_reproducible(shape):
    # (4096, 33, 15) splits the weight gradient's reduction
    B, K, N = shape
    if B >= 4096:
        assert load_native("_kernels").linear_fp8_gw_splits(B, K, N) > 1
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, K, generator=g).bfloat16()
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    gy = torch.randn(B, N, generator=g).bfloat16()
    r1 = _run(x, w, b, gy, True, torch.bfloat16)
    r2 = _run(x, w, b, gy, True, torch.bfloat16)
    for a, c in zip(r1, r2):
        assert torch.equal(a, c)
    # and the split result is right, not just repeatable
    gm = torch.where(r1[0].cpu() > 0, gy.float(), torch.zeros(()))
    gq, sg = ops.quantize_fp8(gm, E5M2)
    xq, sx = ops.quantize_fp8(x, E4M3)
    gd, xd = gq.double() / sg.double(), xq.double() / sx.double()
    _within("gw", r1[2], gd.t() @ xd,
            MFMA_FACTOR * B * U32 * (gd.abs().t() @ xd.abs())
            + U32 * (gd.t() @ xd).abs())


def test_mlp_fp8_gpu():
    with pytest.raises(ValueError, match="compute_dtype"):
        MLP((8, 4, 2), compute_dtype=torch.float16)
    torch.manual_seed(0)
    model = MLP((784, 200, 10), compute_dtype=E4M3).cuda()
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
    print("losses", losses[0], losses[-1])
    assert losses[-1] < losses[0], losses
