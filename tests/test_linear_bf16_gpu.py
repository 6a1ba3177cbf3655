"""GPU tests of the bf16 MFMA linear kernels (csrc/linear_bf16.hip), bf16
dropout and the bf16 mode of MLP.

Inputs are bf16-representable, so the reference is the float64 product of
the same values.  The bounds are derived, not measured, and elementwise:
the half-ulp of bf16 is <= 2^-8 relative; an fp32 sum of L terms is within
L * 2^-24 * sum|terms| under RNE; the factor 2 covers the matrix core's
internal summation order and rounding."""

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
HALF_ULP_BF16 = 2.0 ** -8

SHAPES = [
    (1, 1, 1),          # everything is tail
    (17, 33, 15),       # one past, one past and one short of a tile edge
    (5, 37, 3),         # odd K: bf16 rows are not 4-byte aligned
    (64, 784, 10),      # the MLP's own K and N
    (130, 264, 70),     # several blocks in every dimension, K loop + tail
    (16, 1024, 256),    # long K
]


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


@functools.lru_cache(maxsize=None)
def _case(B, K, N):
    """bf16 inputs (CPU) and the float64 forward reference, built once per
    shape and shared by every test of that shape; never modified."""
    g = torch.Generator().manual_seed(1000 * B + 10 * K + N)
    x = torch.randn(B, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(N, generator=g)
    gy = torch.randn(B, N, generator=g).bfloat16()
    xd, wd, bd = x.double(), w.double(), b.double()
    ref = xd @ wd.t() + bd
    S = xd.abs() @ wd.abs().t() + bd.abs()
    return x, w, b, gy, ref, S


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
    out = ops.linear_bf16(x, w, b, fuse_relu=fuse_relu, out_dtype=out_dtype)
    out.backward(gy.to(DEV).to(out_dtype))
    return out.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("fuse_relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_linear_bf16_bounds(shape, fuse_relu, out_dtype):
    B, K, N = shape
    x, w, b, gy, ref, S = _case(B, K, N)
    # bf16 activations, fp32 master weight (bf16-representable values)
    out, gx, gw, gb = _run(x, w.float(), b, gy, fuse_relu, out_dtype)
    assert out.dtype == out_dtype and out.shape == (B, N)
    assert gx.dtype == torch.bfloat16 and gx.shape == (B, K)
    assert gw.dtype == torch.float32 and gw.shape == (N, K)
    assert gb.dtype == torch.float32 and gb.shape == (N,)

    if fuse_relu:
        ref = ref.relu()
    bound = 2 * K * U32 * S
    if out_dtype == torch.bfloat16:
        bound = bound + HALF_ULP_BF16 * ref.abs()
    _within("out", out, ref, bound)

    # the mask comes from the kernel's own saved output, so the reference
    # and the kernel agree on which units are live
    xd, wd, gd = x.double(), w.double(), gy.double()
    if fuse_relu:
        gd = gd * (out.cpu() > 0)
    ref_gx = gd @ wd
    _within("gx", gx, ref_gx,
            HALF_ULP_BF16 * ref_gx.abs()
            + 2 * N * U32 * (gd.abs() @ wd.abs()))
    _within("gw", gw, gd.t() @ xd, 2 * B * U32 * (gd.abs().t() @ xd.abs()))
    _within("gb", gb, gd.sum(0), 2 * B * U32 * gd.abs().sum(0))


def test_fp32_inputs_are_rounded_like_torch():
    B, K, N = 130, 264, 70
    g = torch.Generator().manual_seed(5)
    x32 = torch.randn(B, K, generator=g)
    w32 = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    gy = torch.randn(B, N, generator=g).bfloat16()
    o1, gx1, gw1, gb1 = _run(x32, w32, b, gy, True, torch.bfloat16)
    o2, gx2, gw2, gb2 = _run(x32.bfloat16(), w32.bfloat16(), b, gy, True,
                             torch.bfloat16)
    assert torch.equal(o1, o2)
    assert gx1.dtype == torch.float32 and gx2.dtype == torch.bfloat16
    assert gw1.dtype == torch.float32 and gw2.dtype == torch.bfloat16
    # one rounding each: fp32 -> bf16 of the fp32 result is the bf16 result
    assert torch.equal(gx1.bfloat16(), gx2)
    assert torch.equal(gw1.bfloat16(), gw2)
    assert torch.equal(gb1, gb2)


def test_cast_kernel_tail_and_unaligned():
    k = load_native("_kernels")
    src = torch.randn(1003, device=DEV)
    for off, n in ((0, 1003), (1, 1001), (4, 7), (0, 8)):
        s = src[off:off + n]
        dst = torch.empty(n + 1, device=DEV, dtype=torch.bfloat16)[1:]
        k.cast_f32_to_bf16(s.data_ptr(), dst.data_ptr(), n,
                           torch.cuda.current_stream().cuda_stream)
        assert torch.equal(dst, s.bfloat16())
        dst = torch.empty(n, device=DEV, dtype=torch.bfloat16)
        k.cast_f32_to_bf16(s.data_ptr(), dst.data_ptr(), n,
                           torch.cuda.current_stream().cuda_stream)
        assert torch.equal(dst, s.bfloat16())


@pytest.mark.parametrize("shape", [(130, 264, 70), (4096, 33, 15)])
def test_bitwise_deterministic(shape):
    # (4096, 33, 15) forces the batch split of the weight gradient
    B, K, N = shape
    if B >= 4096:
        assert load_native("_kernels").linear_bf16_gw_splits(B, K, N) > 1
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
    gd = gy.double() * (r1[0].cpu() > 0)
    _within("gw", r1[2], gd.t() @ x.double(),
            2 * B * U32 * (gd.abs().t() @ x.double().abs()))
    _within("gb", r1[3], gd.sum(0), 2 * B * U32 * gd.abs().sum(0))


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
def test_non_contiguous_x(x_dtype):
    B, K, N = 17, 33, 15
    g = torch.Generator().manual_seed(3)
    xt = torch.randn(K, B, generator=g).to(x_dtype).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    x = xt.t()
    assert not x.is_contiguous()
    a = ops.linear_bf16(x, w, b, fuse_relu=True)
    c = ops.linear_bf16(x.contiguous(), w, b, fuse_relu=True)
    assert torch.equal(a, c)


def test_x_without_grad_skips_gx():
    x, w, b, gy, _, _ = _case(17, 33, 15)
    x = x.to(DEV)
    w = w.float().to(DEV).requires_grad_(True)
    out = ops.linear_bf16(x, w, b.to(DEV))
    out.backward(gy.to(DEV))
    assert x.grad is None and w.grad is not None


def test_linear_fp32_guard_names_linear_bf16():
    x = torch.randn(4, 8, device=DEV).bfloat16()
    w = torch.randn(3, 8, device=DEV)
    with pytest.raises(TypeError, match="linear_bf16"):
        ops.linear(x, w)
    with pytest.raises(TypeError, match="linear_bf16"):
        ops.linear(x.float(), w.bfloat16())


def test_dropout_bf16_matches_fp32_mask():
    n, p = 1_000_003, 0.2
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, generator=g).bfloat16()
    x[x == 0] = 1.0
    x = x.to(DEV)
    ops._seed_ptr(torch.device(DEV))    # make sure the seed buffer exists
    seed = ops._seed_bufs[0]

    seed.fill_(12345)
    y32 = ops.dropout(x.float(), p=p, training=True)
    seed.fill_(12345)
    xb = x.clone().requires_grad_(True)
    y = ops.dropout(xb, p=p, training=True)
    assert y.dtype == torch.bfloat16
    keep = y32 != 0
    assert 0.78 < float(keep.float().mean()) < 0.82
    assert torch.equal(y != 0, keep)
    want = torch.where(keep, (x.float() * 1.25).bfloat16(),
                       torch.zeros_like(x))
    assert torch.equal(y.detach(), want)

    gy = torch.randn(n, generator=g).bfloat16().to(DEV)
    gy[gy == 0] = 1.0
    y.backward(gy)
    assert xb.grad.dtype == torch.bfloat16
    want = torch.where(keep, (gy.float() * 1.25).bfloat16(),
                       torch.zeros_like(gy))
    assert torch.equal(xb.grad, want)


def test_mlp_bf16_gpu():
    torch.manual_seed(0)
    model = MLP((784, 200, 10), compute_dtype=torch.bfloat16).cuda()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, 784, generator=g).to(DEV)
    tgt = torch.randint(0, 10, (64,), generator=g).to(DEV)
    opt = FusedSGD(model.parameters(), lr=0.1, momentum=0.5)
    losses = []
    for step in range(31):
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
    assert losses[-1] < 0.5 * losses[0], losses
