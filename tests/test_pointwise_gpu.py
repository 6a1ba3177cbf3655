"""GPU tests of the templated pointwise and pooling kernels
(csrc/pointwise.hip): one kernel template serves fp32 and bf16, so every
property is checked for both dtypes against something that is not the code
under test — torch on the CPU for the pool, a numpy reimplementation of the
documented generator for the dropout masks.  Everything is exact
(``torch.equal``): the pool only selects values, and a kept dropout value
is one fp32 multiply rounded once."""

import functools

import numpy as np
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
DTYPES = [torch.float32, torch.bfloat16]
SEED0 = 12345
SEED_INC = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
GRID_CAP = 4096 * 256           # threads of the largest elementwise grid


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


def _nonzero(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g).to(dtype)
    t[t == 0] = 1.0
    return t


# ---------------------------------------------------------------------------
# maxpool2d_relu, exact against torch on the CPU
# ---------------------------------------------------------------------------
BIG = (8, 33, 128, 128)     # more outputs than GRID_CAP: the loop strides
assert BIG[0] * BIG[1] * (BIG[2] // 2) * (BIG[3] // 2) > GRID_CAP

POOL_CASES = [
    (torch.float32, (2, 3, 5, 7)),    # odd H and W: floor, last row/col unused
    (torch.float32, (1, 1, 2, 2)),
    (torch.float32, (1, 1, 1, 1)),    # no window at all
    (torch.float32, BIG),
    (torch.bfloat16, (1, 1, 2, 2)),
    (torch.bfloat16, (2, 3, 6, 4)),
    (torch.bfloat16, BIG),
]


@functools.lru_cache(maxsize=None)
def _pool_case(dtype, shape):
    """CPU input, upstream gradient without zeros, and torch's forward and
    backward; built once per case and never modified."""
    B, C, H, W = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)) \
        .to(dtype)
    gy = _nonzero((B, C, H // 2, W // 2), dtype, 6)
    if H < 2 or W < 2:      # torch refuses an empty output; it is empty
        return x, gy, gy.clone(), torch.zeros_like(x)
    xr = x.clone().requires_grad_(True)
    y = F.relu(F.max_pool2d(xr, 2))
    y.backward(gy)
    return x, gy, y.detach(), xr.grad


def _pool_check(x_dev, gy, y_ref, gx_ref):
    x_dev.requires_grad_(True)
    y = ops.maxpool2d_relu(x_dev)
    assert y.dtype == y_ref.dtype and y.shape == y_ref.shape
    assert torch.equal(y.detach().cpu(), y_ref)
    y.backward(gy.to(DEV))
    assert x_dev.grad.dtype == gx_ref.dtype
    assert torch.equal(x_dev.grad.cpu(), gx_ref)


@pytest.mark.parametrize("dtype,shape", POOL_CASES)
def test_pool_exact(dtype, shape):
    x, gy, y_ref, gx_ref = _pool_case(dtype, shape)
    _pool_check(x.to(DEV), gy, y_ref, gx_ref)


def test_pool_bf16_odd_element_offset():
    # a contiguous bf16 view that starts 2 bytes past a 4-byte boundary:
    # the pair accesses need the aligned copy ops makes
    x, gy, y_ref, gx_ref = _pool_case(torch.bfloat16, (2, 3, 6, 4))
    base = torch.empty(x.numel() + 1, dtype=torch.bfloat16, device=DEV)
    view = base[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 4 == 2
    _pool_check(view.detach(), gy, y_ref, gx_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_tie_goes_to_slot_0(dtype):
    x = torch.full((1, 2, 4, 4), 1.5, dtype=dtype)
    gy = _nonzero((1, 2, 2, 2), dtype, 7)
    xr = x.clone().requires_grad_(True)
    F.relu(F.max_pool2d(xr, 2)).backward(gy)
    want = torch.zeros_like(x)
    want[:, :, ::2, ::2] = gy
    assert torch.equal(xr.grad, want)       # torch's rule, spelled out
    xd = x.to(DEV).requires_grad_(True)
    y = ops.maxpool2d_relu(xd)
    assert torch.equal(y.detach().cpu(), torch.full((1, 2, 2, 2), 1.5,
                                                    dtype=dtype))
    y.backward(gy.to(DEV))
    assert torch.equal(xd.grad.cpu(), want)


# ---------------------------------------------------------------------------
# the dropout RNG stream, reimplemented from its description
# ---------------------------------------------------------------------------
def _mix32(seed, idx):
    """splitmix64 finalizer of (seed, index), bits 16..47 of the result."""
    z = np.full(idx.shape, seed & M64, dtype=np.uint64)
    z = z + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return ((z ^ (z >> np.uint64(31))) >> np.uint64(16)) \
        & np.uint64(0xFFFFFFFF)


def _keep_mask(n, p, advances=1):
    """keep[i] of the draw that follows `advances` seed bumps from SEED0."""
    seed = (SEED0 + advances * SEED_INC) & M64
    idx = np.arange(n, dtype=np.uint64)
    r = ((_mix32(seed, idx) << np.uint64(16)) & np.uint64(0xFFFFFFFF)) \
        | (_mix32(seed ^ 0xabcd, idx) & np.uint64(0xFFFF))
    thresh = np.uint32(float(np.float32(p)) * 2.0 ** 32)
    return torch.from_numpy(r.astype(np.uint32) >= thresh)


def _seed_buf():
    ops._seed_ptr(torch.device(DEV))    # make sure the seed buffer exists
    return ops._seed_bufs[0]


def _seed_value():
    return int(_seed_buf().item()) & M64


# float32(0.45) != 0.45, and 1/(1-p) evaluated in fp32 differs from the
# double quotient rounded to fp32: the threshold and both scales notice
P = 0.45


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 257, GRID_CAP + 3])
def test_dropout_mask_is_the_documented_stream(n, dtype):
    x = _nonzero((n,), dtype, 8).to(DEV)
    _seed_buf().fill_(SEED0)
    y = ops.dropout(x, p=P, training=True)
    assert y.dtype == dtype
    assert torch.equal((y != 0).cpu(), _keep_mask(n, P))
    assert _seed_value() == (SEED0 + SEED_INC) & M64


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 5, 2, 3), (37, 29, 1, 1)])
def test_dropout2d_mask_is_the_documented_stream(shape, dtype):
    B, C, H, W = shape
    x = _nonzero(shape, dtype, 9).to(DEV)
    _seed_buf().fill_(SEED0)
    y = ops.dropout2d(x, p=P, training=True)
    assert y.dtype == dtype
    keep = _keep_mask(B * C, P).view(B, C, 1, 1).expand(shape)
    assert torch.equal((y != 0).cpu(), keep)
    assert _seed_value() == (SEED0 + SEED_INC) & M64


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ["dropout", "dropout2d"])
def test_seed_advances_once_per_training_call(op, dtype):
    fn = getattr(ops, op)
    x = _nonzero((3, 5, 2, 3), dtype, 10).to(DEV)
    _seed_buf().fill_(SEED0)
    assert torch.equal(fn(x, p=P, training=False), x)
    assert torch.equal(fn(x, p=0.0, training=True), x)
    assert _seed_value() == SEED0
    fn(x, p=P, training=True)
    assert _seed_value() == (SEED0 + SEED_INC) & M64
    y = fn(x, p=P, training=True)
    assert _seed_value() == (SEED0 + 2 * SEED_INC) & M64
    planes = 15 if op == "dropout2d" else x.numel()
    keep = _keep_mask(planes, P, advances=2)
    keep = keep.view(3, 5, 1, 1).expand(x.shape) if op == "dropout2d" \
        else keep.view(x.shape)
    assert torch.equal((y != 0).cpu(), keep)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ["dropout", "dropout2d"])
def test_dropout_values(op, dtype):
    """Kept elements are x*scale for fp32 and bf16(float(x)*scale) for bf16.
    The forward's scale is 1/(1-p) evaluated in fp32, the backward's the
    double 1/(1-p) rounded to fp32 — the two conventions
    test_dropout2d_bf16_matches_fp32_mask spells out."""
    shape = (4, 7, 3, 5)
    x = _nonzero(shape, dtype, 11)
    gy = _nonzero(shape, dtype, 12)
    one = np.float32(1.0)
    s_fwd = torch.tensor(one / (one - np.float32(P)), dtype=torch.float32)
    s_bwd = torch.tensor(1.0 / (1.0 - P), dtype=torch.float32)
    assert float(s_fwd) != float(s_bwd)     # the test tells them apart
    keep = _keep_mask(4 * 7, P).view(4, 7, 1, 1).expand(shape) \
        if op == "dropout2d" else _keep_mask(x.numel(), P).view(shape)
    zero = torch.zeros(shape, dtype=dtype)

    xd = x.to(DEV).requires_grad_(True)
    _seed_buf().fill_(SEED0)
    y = getattr(ops, op)(xd, p=P, training=True)
    want = torch.where(keep, (x.float() * s_fwd).to(dtype), zero)
    assert torch.equal(y.detach().cpu(), want)
    y.backward(gy.to(DEV))
    assert xd.grad.dtype == dtype
    want = torch.where(keep, (gy.float() * s_bwd).to(dtype), zero)
    assert torch.equal(xd.grad.cpu(), want)


# ---------------------------------------------------------------------------
# fp32-only ops refuse other CUDA dtypes before a pointer reaches a kernel
# ---------------------------------------------------------------------------
def _fp32_only_calls():
    g = torch.Generator().manual_seed(13)
    tgt = torch.randint(0, 10, (6,), generator=g).to(DEV)
    w = torch.randn(4, 3, 5, 5, generator=g).to(DEV)
    return [
        ("relu", torch.randn(64, generator=g), lambda t: ops.relu(t)),
        ("conv2d", torch.randn(2, 3, 8, 8, generator=g),
         lambda t: ops.conv2d(t, w)),
        ("log_softmax", torch.randn(6, 10, generator=g),
         lambda t: ops.log_softmax(t)),
        ("nll_loss", torch.randn(6, 10, generator=g),
         lambda t: ops.nll_loss(t, tgt)),
        ("log_softmax_nll", torch.randn(6, 10, generator=g),
         lambda t: ops.log_softmax_nll(t, tgt)),
    ]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
def test_fp32_ops_refuse_other_cuda_dtypes(dtype):
    for name, x, call in _fp32_only_calls():
        xd = x.to(dtype).to(DEV)
        before = xd.clone()
        with pytest.raises(TypeError, match=name):
            call(xd)
        assert torch.equal(xd, before), name
    w = torch.randn(4, 3, 5, 5, device=DEV).to(dtype)
    with pytest.raises(TypeError, match="conv2d"):
        ops.conv2d(torch.randn(2, 3, 8, 8, device=DEV), w)
