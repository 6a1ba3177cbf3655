"""Cases, inputs, references and bounds shared by tests/test_pool_cpu.py and
tests/test_pool_gpu.py (ops.maxpool2d and ops.global_avgpool2d), so the
kernels answer to exactly what the CPU golden path meets.

Max-pool.  Inputs are ``relu(randn)`` cast to the dtype — about half the
values are tied zeros, as in ResNet's stem — with one -inf element, and in
one case a whole window of -inf.  Max only selects, so ``y`` must equal
torch's bit for bit.  With ``gy`` drawn from the integers in [-8, 8] every
sum of at most 9 terms is an integer of magnitude <= 72, exact in fp32 and
bf16 in any order, so ``gx`` must equal torch's too.  For a random ``gy``
the reference is a float64 scatter of ``gy`` by torch's indices; an fp32
sum of at most ``t = ceil(kh/sh)*ceil(kw/sw)`` terms in any order is within
``t * 2^-24 * A`` of it, ``A`` being the same scatter of ``|gy|``, and the
bf16 rounding adds at most ``2^-8 * |ref|``.

Global average.  The fp32 sum of HW terms in any order is within
``(HW-1) * 2^-24 * sum|x|`` of the exact one; dividing by HW scales that and
adds one rounding, ``2^-24 * |mean|``; a bf16 output adds ``2^-8 * |mean|``.
The backward is one fp32 division (correctly rounded: ``2^-24 * |ref|``)
and, for bf16, one more rounding of that (8 significant bits: ``2^-8``
relative, of a value within ``1 + 2^-24`` of the reference).
"""

import math

import torch
import torch.nn.functional as F

DTYPES = [torch.float32, torch.bfloat16]

# (shape, kernel, stride, padding)
MAXPOOL_CASES = [
    ((2, 3, 7, 9), 3, 2, 1),            # odd extents
    ((1, 2, 8, 8), 3, 2, 1),            # carries the all -inf window
    ((1, 1, 1, 1), 3, 2, 1),            # window mostly padding
    ((2, 2, 5, 5), 2, 2, 0),            # last row/column in no window
    ((1, 3, 6, 7), 3, 1, 1),            # up to 9 windows per input
    ((2, 2, 9, 9), 3, 3, 0),            # disjoint windows
    ((1, 2, 6, 10), (3, 2), (2, 1), (1, 0)),   # rectangular everything
    ((3, 70, 12, 12), 3, 2, 1),         # many planes
]
# more than 4096*256 outputs: the grid-stride loops run more than once
BIG_CASE = ((8, 64, 96, 96), 3, 2, 1)
INF_WINDOW_SHAPE = (1, 2, 8, 8)
RANDOM_GY_CASE = ((1, 3, 6, 7), 3, 1, 1)

AVG_SHAPES = [
    (2, 3, 7, 7),
    (3, 5, 1, 1),
    (2, 4, 14, 14),
    (1, 2, 40, 40),      # more elements than a block has threads
    (70, 33, 3, 5),      # many odd planes
]


def case_id(case):
    shape, k, s, p = case
    return "x".join(map(str, shape)) + f"-k{k}s{s}p{p}".replace(" ", "")


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def windows_per_input(k, s):
    (kh, kw), (sh, sw) = pair(k), pair(s)
    return math.ceil(kh / sh) * math.ceil(kw / sw)


def maxpool_input(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = F.relu(torch.randn(shape, generator=g)).to(dtype)
    x.view(-1)[x.numel() // 2] = float("-inf")
    if tuple(shape) == INF_WINDOW_SHAPE:
        # with k3 s2 p1, output (0, 0) sees rows 0-1 and columns 0-1 only
        x[0, 0, :2, :2] = float("-inf")
    return x


def out_shape(shape, k, s, p):
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(s), pair(p)
    B, C, H, W = shape
    return (B, C, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1)


def integer_gy(shape, dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(dtype)


def random_gy(shape, dtype, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def torch_maxpool(x, k, s, p, gy):
    """torch on the CPU, autograd included: (y, gx)."""
    xt = x.detach().clone().requires_grad_(True)
    y = F.max_pool2d(xt, k, s, p)
    y.backward(gy)
    return y.detach(), xt.grad


def scatter_reference(x, k, s, p, gy):
    """float64 scatter of gy, and of |gy|, by torch's indices: (ref, A)."""
    B, C, H, W = x.shape
    _, idx = F.max_pool2d(x.double(), k, s, p, return_indices=True)
    idx = idx.reshape(B * C, -1)
    g = gy.double().reshape(B * C, -1)
    ref = torch.zeros(B * C, H * W, dtype=torch.float64)
    a = torch.zeros(B * C, H * W, dtype=torch.float64)
    ref.scatter_add_(1, idx, g)
    a.scatter_add_(1, idx, g.abs())
    return ref.view(B, C, H, W), a.view(B, C, H, W)


def maxpool_gx_bound(ref, a, k, s, dtype):
    t = windows_per_input(k, s)
    bound = t * 2.0 ** -24 * a
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    return bound


def run_maxpool(ops, x, k, s, p, gy):
    """ops.maxpool2d forward and backward on x's device: (y, gx)."""
    xt = x.detach().requires_grad_(True)      # keeps x's storage
    y = ops.maxpool2d(xt, k, s, p)
    y.backward(gy)
    return y.detach(), xt.grad


def check_maxpool_exact(ops, case, dtype, dev="cpu"):
    shape, k, s, p = case
    x = maxpool_input(shape, dtype)
    gy = integer_gy(out_shape(shape, k, s, p), dtype)
    want_y, want_gx = torch_maxpool(x, k, s, p, gy)
    y, gx = run_maxpool(ops, x.to(dev), k, s, p, gy.to(dev))
    assert y.dtype == dtype and gx.dtype == dtype
    assert y.shape == want_y.shape and gx.shape == x.shape
    assert torch.equal(y.cpu(), want_y)
    assert torch.equal(gx.cpu(), want_gx)
    return x, gx.cpu()


def check_maxpool_random_gy(ops, dtype, dev="cpu"):
    shape, k, s, p = RANDOM_GY_CASE
    x = maxpool_input(shape, dtype)
    gy = random_gy(out_shape(shape, k, s, p), dtype)
    ref, a = scatter_reference(x, k, s, p, gy)
    _, gx = run_maxpool(ops, x.to(dev), k, s, p, gy.to(dev))
    err = (gx.cpu().double() - ref).abs()
    bound = maxpool_gx_bound(ref, a, k, s, dtype)
    print(f"maxpool gx {dtype}: max err {err.max():.3e}, "
          f"max bound {bound.max():.3e}")
    assert (err <= bound).all()


def avg_input(shape, dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def avg_fwd_bound(x, dtype):
    hw = x.shape[2] * x.shape[3]
    xd = x.double()
    mean = xd.mean(dim=(2, 3))
    bound = (hw - 1) * 2.0 ** -24 * xd.abs().sum(dim=(2, 3)) / hw \
        + 2.0 ** -24 * mean.abs()
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * mean.abs()
    return mean, bound


def avg_bwd_bound(gy, hw, dtype):
    ref = gy.double() / hw
    rel = 2.0 ** -24
    if dtype == torch.bfloat16:
        rel = 2.0 ** -8 * (1 + 2.0 ** -24) + 2.0 ** -24
    return ref, rel * ref.abs()


def run_avg(ops, x, gy):
    xt = x.detach().requires_grad_(True)
    y = ops.global_avgpool2d(xt)
    y.backward(gy)
    return y.detach(), xt.grad


def check_avg(ops, shape, dtype, dev="cpu"):
    B, C, H, W = shape
    x = avg_input(shape, dtype)
    gy = random_gy((B, C), dtype)
    y, gx = run_avg(ops, x.to(dev), gy.to(dev))
    assert y.dtype == dtype and y.shape == (B, C)
    assert gx.dtype == dtype and gx.shape == x.shape
    mean, bound = avg_fwd_bound(x, dtype)
    err = (y.cpu().double() - mean).abs()
    print(f"avg fwd {shape} {dtype}: max err {err.max():.3e}, "
          f"max bound {bound.max():.3e}")
    assert (err <= bound).all()
    ref, bbound = avg_bwd_bound(gy, H * W, dtype)
    berr = (gx.cpu().double() - ref.view(B, C, 1, 1)).abs()
    print(f"avg bwd {shape} {dtype}: max err {berr.max():.3e}, "
          f"max bound {bbound.max():.3e}")
    assert (berr <= bbound.view(B, C, 1, 1)).all()
