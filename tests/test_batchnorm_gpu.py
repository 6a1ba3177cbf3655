"""GPU tests of ops.batchnorm2d (csrc/batchnorm.hip) and of the bf16 mode
of models.resnet.  The float64 references and the derived elementwise
bounds are in tests/bn_bounds.py (its docstring has the derivation); the
case runners there are shared with tests/test_batchnorm_cpu.py, so the kernels
answer to exactly the bounds the CPU golden path meets."""

import os
import sys

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bn_bounds as bb
    from dist_tuto_pth_amd import ops
    from dist_tuto_pth_amd.models.resnet import Bottleneck
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
SPLIT_SHAPE = (64, 2, 20, 20)
SHAPES = [
    (2, 3, 5, 7),        # odd HW = 35: one element per access
    (2, 5, 1, 1),        # n = 2, HW = 1
    (2, 3, 2, 3),        # HW = 6: two elements per access in both dtypes
    (3, 70, 4, 4),       # C > 64, HW = 16
    (4, 8, 6, 6),        # bf16 planes only 8-byte aligned
    (2, 16, 14, 14),     # ResNet's 14x14 planes
    (5, 4, 7, 7),        # ResNet's 7x7 planes
    SPLIT_SHAPE,         # more than one slice per channel
]
OFFSET_SHAPES = [(2, 3, 5, 7), (4, 8, 6, 6), (3, 70, 4, 4)]
MODES = [(False, False), (False, True), (True, True)]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


@pytest.mark.parametrize("residual,relu", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_batchnorm2d_bounds(shape, dtype, residual, relu):
    if shape == SPLIT_SHAPE:
        B, C, H, W = shape
        assert load_native("_kernels").batchnorm2d_splits(B, C, H * W) > 1
    bb.train_case(shape, dtype, residual, relu, dev=DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", OFFSET_SHAPES)
def test_offset_inputs_need_a_centred_variance(shape, dtype):
    bb.train_case(shape, dtype, True, True, dev=DEV,
                  offset=100.0 if dtype == torch.float32 else 16.0)


def test_splits_depend_on_shapes_and_fill_the_chip():
    k = load_native("_kernels")
    # ResNet's stem: few channels, many pixels -> at least 8 blocks per CU
    assert 64 * k.batchnorm2d_splits(32, 64, 112 * 112) >= 2048
    # many channels of 49 pixels are not split to nothing
    assert k.batchnorm2d_splits(32, 2048, 49) == 1
    assert k.batchnorm2d_splits(2, 5, 1) == 1
    for B, C, HW in [(32, 64, 12544), (64, 2, 400), (7, 3, 100000)]:
        s = k.batchnorm2d_splits(B, C, HW)
        assert 1 <= s <= B and s == k.batchnorm2d_splits(B, C, HW)


@pytest.mark.parametrize("residual,relu", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 70, 4, 4), (5, 4, 7, 7)])
def test_eval_mode(shape, dtype, residual, relu):
    bb.eval_case(shape, dtype, residual, relu, DEV)


def _full_run(x, gamma, beta, res, gy, relu, **kw):
    xt = x.detach().requires_grad_(True)      # keeps x's storage
    wt = gamma.detach().clone().requires_grad_(True)
    bt = beta.detach().clone().requires_grad_(True)
    rt = res.detach().requires_grad_(True) if res is not None \
        else None
    C = x.shape[1]
    rm = torch.zeros(C, device=x.device)
    rv = torch.ones(C, device=x.device)
    y = ops.batchnorm2d(xt, wt, bt, rm, rv, residual=rt, fuse_relu=relu,
                        **kw)
    y.backward(gy)
    out = [y.detach(), rm, rv, xt.grad, wt.grad, bt.grad]
    if rt is not None:
        out.append(rt.grad)
    return out


def _dev_case(shape, dtype, residual, offset=0.0):
    return [t.to(DEV) if t is not None else None
            for t in bb.make_case(shape, dtype, residual, offset)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_shape_is_bitwise_deterministic(dtype):
    x, gamma, beta, res, gy = _dev_case(SPLIT_SHAPE, dtype, True)
    r1 = _full_run(x, gamma, beta, res, gy, True)
    r2 = _full_run(x, gamma, beta, res, gy, True)
    assert len(r1) == 7
    for a, c in zip(r1, r2):
        assert torch.equal(a, c)


@pytest.mark.parametrize("shape", [(4, 8, 6, 6), (5, 4, 7, 7), SPLIT_SHAPE])
def test_bf16_is_the_fp32_result_rounded_once(shape):
    # same values, same fp32 arithmetic in the same order: only the final
    # rounding differs, whatever access width each dtype's launch picked
    x, gamma, beta, res, gy = _dev_case(shape, torch.bfloat16, True)
    for r, relu in ((None, False), (res, True)):
        yb = ops.batchnorm2d(x, gamma, beta, residual=r, fuse_relu=relu)
        yf = ops.batchnorm2d(x.float(), gamma, beta,
                             residual=None if r is None else r.float(),
                             fuse_relu=relu)
        assert yb.dtype == torch.bfloat16 and yf.dtype == torch.float32
        assert torch.equal(yb, yf.bfloat16())


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 16, 14, 14)])
def test_fusion_equals_composition(shape):
    x, gamma, beta, res, _ = _dev_case(shape, torch.float32, True)
    fused = ops.batchnorm2d(x, gamma, beta, residual=res, fuse_relu=True)
    chained = ops.relu(ops.batchnorm2d(x, gamma, beta) + res)
    assert torch.equal(fused, chained)


def test_misaligned_batch_slice_equals_its_clone():
    # C*H*W = 3*5*7 is odd: x[1:] starts 2-byte aligned only
    big, gamma, beta, bigres, biggy = _dev_case((3, 3, 5, 7),
                                                torch.bfloat16, True)
    x, res, gy = big[1:], bigres[1:], biggy[1:]
    assert x.is_contiguous() and x.data_ptr() % 4 == 2
    a = _full_run(x, gamma, beta, res, gy, True)
    c = _full_run(x.clone(), gamma, beta, res.clone(), gy.clone(), True)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_contiguous_x(dtype):
    x, gamma, beta, res, gy = _dev_case((2, 16, 14, 14), dtype, True)
    xn = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not xn.is_contiguous() and torch.equal(xn, x)
    a = _full_run(xn, gamma, beta, res, gy, True)
    c = _full_run(x, gamma, beta, res, gy, True)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


def test_x_without_grad_skips_gx():
    x, gamma, beta, res, gy = _dev_case((4, 8, 6, 6), torch.bfloat16, True)
    wt = gamma.clone().requires_grad_(True)
    bt = beta.clone().requires_grad_(True)
    y = ops.batchnorm2d(x, wt, bt, residual=res, fuse_relu=True)
    y.backward(gy)
    assert x.grad is None and res.grad is None
    assert wt.grad is not None and bt.grad is not None
    want = _full_run(x, gamma, beta, res, gy, True, momentum=0.1)
    assert torch.equal(wt.grad, want[4]) and torch.equal(bt.grad, want[5])


def test_gpu_dtype_guards():
    x = torch.randn(2, 3, 4, 4, device=DEV)
    w = torch.ones(3, device=DEV)
    b = torch.zeros(3, device=DEV)
    with pytest.raises(TypeError, match="batchnorm2d"):
        ops.batchnorm2d(x.half(), w, b)
    with pytest.raises(TypeError, match="weight"):
        ops.batchnorm2d(x.bfloat16(), w.bfloat16(), b)
    with pytest.raises(TypeError, match="residual"):
        ops.batchnorm2d(x.bfloat16(), w, b, residual=x)
    with pytest.raises(ValueError, match="training=False"):
        ops.batchnorm2d(x, w, b, training=False)
    with pytest.raises(ValueError, match="more than one value"):
        ops.batchnorm2d(x[:1, :, :1, :1], w, b)
    with pytest.raises(ValueError, match="not supported"):
        ops.batchnorm2d(x, w, b, w.clone(), w.clone(), momentum=None)
    with pytest.raises(ValueError, match="is on"):
        ops.batchnorm2d(x, w.cpu(), b)


# ---------------------------------------------------------------------------
# models.resnet in bf16 mode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
def test_bottleneck_bf16_is_the_ops_chained_by_hand(training):
    torch.manual_seed(0)
    down = nn.Sequential(nn.Conv2d(64, 64, 1, stride=2, bias=False),
                         nn.BatchNorm2d(64))
    blk = Bottleneck(64, 16, stride=2, downsample=down,
                     compute_dtype=torch.bfloat16).to(DEV)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(
                    0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape,
                                                     generator=g))
    blk.train(training)
    x = torch.randn(3, 64, 10, 10, generator=g).bfloat16().to(DEV)
    bf16 = torch.bfloat16

    def bn(m, h, rm, rv, **kw):
        return ops.batchnorm2d(h, m.weight, m.bias, rm, rv,
                               training=training, momentum=m.momentum,
                               eps=m.eps, **kw)

    # by hand, on copies of the running buffers
    bufs = {n: (m.running_mean.clone(), m.running_var.clone())
            for n, m in (("bn1", blk.bn1), ("bn2", blk.bn2),
                         ("bn3", blk.bn3), ("down", down[1]))}
    with torch.no_grad():
        h = ops.conv2d_bf16(x, blk.conv1.weight, None, out_dtype=bf16)
        h = bn(blk.bn1, h, *bufs["bn1"], fuse_relu=True)
        h = ops.conv2d_bf16(h, blk.conv2.weight, None, stride=2, padding=1,
                            out_dtype=bf16)
        h = bn(blk.bn2, h, *bufs["bn2"], fuse_relu=True)
        assert h.dtype == bf16 and h.shape == (3, 16, 5, 5)
        idn = ops.conv2d_bf16(x, down[0].weight, None, stride=2,
                              out_dtype=bf16)
        idn = bn(down[1], idn, *bufs["down"])
        h = ops.conv2d_bf16(h, blk.conv3.weight, None, out_dtype=bf16)
        want = bn(blk.bn3, h, *bufs["bn3"], residual=idn, fuse_relu=True)
        got = blk(x)
    assert got.dtype == bf16 and got.shape == (3, 64, 5, 5)
    assert torch.equal(got, want)
    for n, m in (("bn1", blk.bn1), ("bn2", blk.bn2), ("bn3", blk.bn3),
                 ("down", down[1])):
        assert torch.equal(m.running_mean, bufs[n][0])
        assert torch.equal(m.running_var, bufs[n][1])
        assert int(m.num_batches_tracked) == 0


def test_tiny_resnet_bf16_converges_like_fp32_gpu():
    bb.check_tiny_resnet_convergence(DEV)
