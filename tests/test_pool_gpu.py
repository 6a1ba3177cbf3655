"""GPU tests of ops.maxpool2d and ops.global_avgpool2d (csrc/pool.hip) and
of their use in the bf16 mode of models.resnet.  Cases, references and the
derived bounds are in tests/pool_cases.py (its docstring has the
derivation), shared with tests/test_pool_cpu.py."""

import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pool_cases as pc
    from dist_tuto_pth_amd import ops
    from dist_tuto_pth_amd.models.resnet import ResNet
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
DTYPES = pc.DTYPES


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


# ---------------------------------------------------------------------------
# max-pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", pc.MAXPOOL_CASES, ids=pc.case_id)
def test_maxpool2d_equals_torch(case, dtype):
    x, gx = pc.check_maxpool_exact(ops, case, dtype, DEV)
    if case[0] == (2, 2, 5, 5):
        # 2x2/2 windows never reach the last row and column
        assert (gx[:, :, 4, :] == 0).all() and (gx[:, :, :, 4] == 0).all()


def test_maxpool2d_grid_stride_loops_run_more_than_once():
    shape, k, s, p = pc.BIG_CASE
    assert torch.Size(pc.out_shape(shape, k, s, p)).numel() > 4096 * 256
    pc.check_maxpool_exact(ops, pc.BIG_CASE, torch.bfloat16, DEV)


@pytest.mark.parametrize("dtype", DTYPES)
def test_maxpool2d_random_gy(dtype):
    pc.check_maxpool_random_gy(ops, dtype, DEV)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_propagates_to_every_window_that_contains_it(dtype):
    shape, k, s, p = (2, 3, 7, 9), 3, 2, 1
    x = pc.maxpool_input(shape, dtype)
    x[0, 1, 3, 3] = float("nan")      # odd row and column: four windows
    x[1, 2, 0, 0] = float("nan")      # a corner: one window
    y = ops.maxpool2d(x.to(DEV), k, s, p).cpu()
    has_nan = F.max_pool2d(torch.isnan(x).float(), k, s, p) > 0
    assert int(has_nan.sum()) == 5
    assert torch.equal(torch.isnan(y), has_nan)
    want = F.max_pool2d(x, k, s, p)
    assert torch.equal(y[~has_nan], want[~has_nan])


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (3, 70, 12, 12)])
def test_maxpool2d_bf16_is_the_fp32_op_on_the_same_values(shape):
    x = pc.maxpool_input(shape, torch.bfloat16).to(DEV)
    yb = ops.maxpool2d(x, 3, 2, 1)
    yf = ops.maxpool2d(x.float(), 3, 2, 1)
    assert yb.dtype == torch.bfloat16 and yf.dtype == torch.float32
    assert torch.equal(yb, yf.bfloat16())


# ---------------------------------------------------------------------------
# global average pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", pc.AVG_SHAPES)
def test_global_avgpool2d_bounds(shape, dtype):
    pc.check_avg(ops, shape, dtype, DEV)


@pytest.mark.parametrize("shape", pc.AVG_SHAPES)
def test_global_avgpool2d_bf16_is_the_fp32_result_rounded_once(shape):
    # the order of the sum depends on H*W alone, not on the dtype
    x = pc.avg_input(shape, torch.bfloat16).to(DEV)
    yb = ops.global_avgpool2d(x)
    yf = ops.global_avgpool2d(x.float())
    assert yb.dtype == torch.bfloat16 and yf.dtype == torch.float32
    assert torch.equal(yb, yf.bfloat16())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (3, 5, 1, 1), (2, 3, 7, 7)])
def test_global_avgpool2d_bwd_into_a_misaligned_gx(shape, offset, dtype):
    # ops allocates gx itself, so only the entry point meets a gx that
    # starts off a 16-byte boundary: scalar head, 16-byte body, scalar tail
    k = load_native("_kernels")
    B, C, H, W = shape
    n = B * C * H * W
    gy = pc.random_gy((B, C), dtype).to(DEV)
    buf = torch.full((n + offset + 9,), 7.0, device=DEV, dtype=dtype)
    gx = buf[offset:offset + n]
    assert gx.data_ptr() % 16 == offset * gx.element_size()
    k.global_avgpool2d_bwd(gy.data_ptr(), gx.data_ptr(), B * C, H * W,
                           dtype == torch.bfloat16,
                           torch.cuda.current_stream().cuda_stream)
    want = torch.empty(n, device=DEV, dtype=dtype)
    k.global_avgpool2d_bwd(gy.data_ptr(), want.data_ptr(), B * C, H * W,
                           dtype == torch.bfloat16,
                           torch.cuda.current_stream().cuda_stream)
    assert torch.equal(gx, want)
    _, got = pc.run_avg(ops, pc.avg_input(shape, dtype).to(DEV), gy)
    assert torch.equal(want.view(shape), got)
    # nothing written outside gx
    assert (buf[:offset] == 7).all() and (buf[offset + n:] == 7).all()


# ---------------------------------------------------------------------------
# determinism and alignment, both ops
# ---------------------------------------------------------------------------
def _run_max(x, gy):
    return pc.run_maxpool(ops, x, 3, 2, 1, gy)


def _run_avg(x, gy):
    return pc.run_avg(ops, x, gy)


_BOTH = [
    ("max", _run_max, pc.maxpool_input, (3, 5, 7, 9),
     pc.out_shape((3, 5, 7, 9), 3, 2, 1)),
    ("avg", _run_avg, pc.avg_input, (3, 5, 7, 7), (3, 5)),
    ("avg-block", _run_avg, pc.avg_input, (1, 3, 35, 37), (1, 3)),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,run,make,shape,oshape", _BOTH,
                         ids=[b[0] for b in _BOTH])
def test_two_runs_are_bitwise_equal(name, run, make, shape, oshape, dtype):
    x = make(shape, dtype).to(DEV)
    gy = pc.random_gy(oshape, dtype).to(DEV)
    a, c = run(x, gy), run(x, gy)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,run,make,shape,oshape", _BOTH,
                         ids=[b[0] for b in _BOTH])
def test_view_one_element_into_a_buffer_equals_its_clone(
        name, run, make, shape, oshape, dtype):
    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        return v

    x = shifted(make(shape, dtype).to(DEV))
    gy = shifted(pc.random_gy(oshape, dtype).to(DEV))
    es = x.element_size()
    assert x.is_contiguous() and x.data_ptr() % 16 == es
    assert gy.is_contiguous() and gy.data_ptr() % 16 == es
    a = run(x, gy)
    c = run(x.clone(), gy.clone())
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# ---------------------------------------------------------------------------
# argument errors: raised in Python or in the launcher, before any launch
# ---------------------------------------------------------------------------
def test_argument_errors():
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    with pytest.raises(TypeError, match="maxpool2d"):
        ops.maxpool2d(x.half(), 3, 2, 1)
    with pytest.raises(TypeError, match="global_avgpool2d"):
        ops.global_avgpool2d(x.half())
    with pytest.raises(ValueError, match="maxpool2d"):
        ops.maxpool2d(x[0], 3, 2, 1)
    with pytest.raises(ValueError, match="global_avgpool2d"):
        ops.global_avgpool2d(x[0])
    with pytest.raises(ValueError, match="maxpool2d: padding"):
        ops.maxpool2d(x, 3, 2, 2)
    with pytest.raises(ValueError, match="maxpool2d.*256"):
        ops.maxpool2d(torch.zeros(1, 1, 20, 20, device=DEV), 17)


def test_launcher_argument_errors():
    k = load_native("_kernels")
    x = torch.zeros(1, 1, 20, 20, device=DEV)
    y = torch.zeros(1, 1, 20, 20, device=DEV)
    slot = torch.zeros(1, 1, 20, 20, device=DEV, dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream

    def fwd(*geom):
        k.maxpool2d_fwd(x.data_ptr(), y.data_ptr(), slot.data_ptr(), 1, 1,
                        20, 20, *geom, False, st)

    with pytest.raises(ValueError, match="256"):
        fwd(17, 17, 1, 1, 0, 0)
    with pytest.raises(ValueError, match="padding"):
        fwd(3, 3, 2, 2, 2, 2)
    with pytest.raises(ValueError, match="does not fit"):
        k.maxpool2d_fwd(x.data_ptr(), y.data_ptr(), slot.data_ptr(), 1, 1,
                        4, 4, 9, 9, 1, 1, 1, 1, False, st)
    with pytest.raises(ValueError, match="stride"):
        fwd(3, 3, 0, 1, 1, 1)
    with pytest.raises(ValueError, match="null"):
        k.maxpool2d_bwd(0, slot.data_ptr(), x.data_ptr(), 1, 1, 20, 20,
                        3, 3, 2, 2, 1, 1, False, st)
    with pytest.raises(ValueError, match=">= 1"):
        k.global_avgpool2d_fwd(x.data_ptr(), y.data_ptr(), 0, 400, False, st)
    with pytest.raises(ValueError, match="null"):
        k.global_avgpool2d_bwd(0, y.data_ptr(), 1, 400, False, st)


# ---------------------------------------------------------------------------
# models.resnet in bf16 mode
# ---------------------------------------------------------------------------
def _tiny_resnet():
    torch.manual_seed(0)
    return ResNet((1, 1, 1, 1), num_classes=10,
                  compute_dtype=torch.bfloat16).to(DEV)


def test_resnet_bf16_borrows_no_pooling_from_torch(monkeypatch):
    def borrowed(*a, **kw):
        raise AssertionError("pooling borrowed from torch")

    model = _tiny_resnet()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    monkeypatch.setattr(torch.nn.functional, "max_pool2d", borrowed)
    monkeypatch.setattr(torch.nn.functional, "adaptive_avg_pool2d", borrowed)
    out = model(x.to(DEV))
    out.sum().backward()
    assert out.shape == (2, 10) and out.dtype == torch.float32
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


@pytest.mark.parametrize("training", [True, False])
def test_resnet_bf16_stem_and_head_are_the_ops_chained_by_hand(training):
    model = _tiny_resnet()
    model.train(training)
    x = torch.randn(2, 3, 32, 32,
                    generator=torch.Generator().manual_seed(1)).to(DEV)
    bf16 = torch.bfloat16
    bn1 = model.bn1
    rm, rv = bn1.running_mean.clone(), bn1.running_var.clone()
    with torch.no_grad():
        h = ops.conv2d_bf16(x, model.conv1.weight, None, stride=2, padding=3,
                            out_dtype=bf16)
        h = ops.batchnorm2d(h, bn1.weight, bn1.bias, rm, rv,
                            training=training, momentum=bn1.momentum,
                            eps=bn1.eps, fuse_relu=True)
        h = ops.maxpool2d(h, 3, 2, 1)
        assert h.dtype == bf16 and h.shape == (2, 64, 8, 8)
        # a training-mode block normalizes with the batch statistics, so
        # running it here and again inside the model gives the same output
        h = model.layer4(model.layer3(model.layer2(model.layer1(h))))
        assert h.shape == (2, 2048, 1, 1)
        h = ops.global_avgpool2d(h)
        assert h.dtype == bf16 and h.shape == (2, 2048)
        want = ops.linear_bf16(h, model.fc.weight, model.fc.bias,
                               out_dtype=torch.float32)
        got = model(x)
    assert got.dtype == torch.float32 and got.shape == (2, 10)
    assert torch.equal(got, want)
    assert torch.equal(bn1.running_mean, rm)
    assert torch.equal(bn1.running_var, rv)
    assert isinstance(model.maxpool, nn.MaxPool2d)
    assert isinstance(model.avgpool, nn.AdaptiveAvgPool2d)
