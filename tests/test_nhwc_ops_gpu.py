"""GPU tests of the channels-last kernels behind ops.batchnorm2d,
ops.maxpool2d and ops.global_avgpool2d (csrc/batchnorm_nhwc.hip,
csrc/pool_nhwc.hip) and of models.resnet's channels-last mode.  Inputs,
float64 references and bounds are those of tests/bn_bounds.py and
tests/pool_cases.py, unchanged: the layout changes where the values lie,
not what is asked of them."""

import functools
import os
import sys
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bn_bounds as bb
    import pool_cases as pc
    from dist_tuto_pth_amd import ops
    from dist_tuto_pth_amd.models.resnet import Bottleneck, ResNet
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
CL = torch.channels_last
# 343 rows in 2 slices of 172 and 171 rows: neither a multiple of the 32
# row lanes (test_nhwc_ops_cpu.py checks the rule)
SPLIT_SHAPE = (7, 6, 7, 7)
SHAPES = [
    (2, 3, 5, 7),        # C odd: one element per access
    (2, 6, 2, 3),        # two elements per access
    (1, 5, 1, 2),        # two rows: fewer rows than row lanes
    (3, 12, 3, 3),       # bf16 8-byte only; 27 rows, no multiple of the lanes
    (3, 70, 4, 4),       # ragged last column tile
    (2, 64, 7, 7),       # full width at ResNet's 7x7 maps
    (2, 128, 14, 14),    # full width, 16 column lanes, 14x14 maps
    SPLIT_SHAPE,
]
MODES = [(False, False), (False, True), (True, True)]
DTYPES = [torch.float32, torch.bfloat16]
NHWC_OPS = types.SimpleNamespace(
    maxpool2d=functools.partial(ops.maxpool2d, memory_format=CL),
    global_avgpool2d=functools.partial(ops.global_avgpool2d,
                                       memory_format=CL))


def nhwc(t, grad=False):
    t = t.to(DEV).contiguous(memory_format=CL)
    return t.requires_grad_(True) if grad else t


def is_nhwc(t):
    return t.permute(0, 2, 3, 1).is_contiguous()


def run_bn(case, relu, training, rm=None, rv=None):
    """ops.batchnorm2d forward and backward in channels-last mode on the CPU
    tensors of ``case``: y, the saved statistics, the four gradients and the
    running buffers, the seven outputs of one call."""
    x, gamma, beta, res, gy = case
    C = x.shape[1]
    xt, rt = nhwc(x, True), None if res is None else nhwc(res, True)
    wt = gamma.clone().to(DEV).requires_grad_(True)
    bt = beta.clone().to(DEV).requires_grad_(True)
    rm = torch.full((C,), 3.0, device=DEV) if rm is None else rm.to(DEV)
    rv = torch.full((C,), 7.0, device=DEV) if rv is None else rv.to(DEV)
    kw = dict(training=training, momentum=1.0, eps=bb.EPS, residual=rt,
              fuse_relu=relu, memory_format=CL)
    y = ops.batchnorm2d(xt, wt, bt, rm, rv, **kw)
    with torch.no_grad():
        y2, mean, invstd = ops._batchnorm2d_forward(
            xt.detach(), wt.detach(), bt.detach(), None if training else rm,
            None if training else rv, training, 0.1, bb.EPS,
            None if rt is None else rt.detach(), relu, memory_format=CL)
    assert torch.equal(y2, y.detach())
    y.backward(nhwc(gy))
    for t in (y, xt.grad) + (() if rt is None else (rt.grad,)):
        assert is_nhwc(t) and t.dtype == x.dtype and t.shape == x.shape
    return dict(y=y.detach(), mean=mean, invstd=invstd, gx=xt.grad,
                gw=wt.grad, gb=bt.grad, gres=None if rt is None else rt.grad,
                rm=rm, rv=rv)


def check_train(shape, dtype, residual, relu, offset=0.0):
    case = bb.make_case(shape, dtype, residual, offset)
    x, gamma, beta, res, gy = case
    ref = bb.forward_reference(x, gamma, beta, res, relu)
    n = ref["n"]
    o = run_bn(case, relu, True)
    bb.within("y", o["y"], ref["y"], ref["By"])
    bb.within("mean", o["rm"], ref["mu"], ref["Bm"])
    bb.within("var", o["rv"], ref["v"] * n / (n - 1), ref["Bv"] * n / (n - 1))
    assert torch.equal(o["mean"], o["rm"])
    bref = bb.backward_reference(x, gamma, gy, o["mean"], o["invstd"],
                                 o["y"], relu, True)
    bb.within("gx", o["gx"], bref["gx"], bref["Bgx"])
    bb.within("gweight", o["gw"], bref["dg"], bref["Bdg"])
    bb.within("gbias", o["gb"], bref["db"], bref["Bdb"])
    if residual:    # the masked gy, exactly
        assert torch.equal(o["gres"].double().cpu(), bref["g"])


@pytest.mark.parametrize("residual,relu", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_batchnorm2d_nhwc_bounds(shape, dtype, residual, relu):
    if shape == SPLIT_SHAPE:
        B, C, H, W = shape
        k = load_native("_kernels")
        assert k.batchnorm2d_nhwc_splits(B * H * W, C) == 2
    check_train(shape, dtype, residual, relu)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (3, 70, 4, 4)])
def test_offset_inputs_need_a_centred_variance(shape, dtype):
    check_train(shape, dtype, True, True,
                offset=100.0 if dtype == torch.float32 else 16.0)


@pytest.mark.parametrize("residual,relu", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 70, 4, 4), (2, 64, 7, 7)])
def test_eval_mode(shape, dtype, residual, relu):
    case = bb.make_case(shape, dtype, residual)
    x, gamma, beta, res, gy = case
    g = torch.Generator().manual_seed(5)
    rm = torch.randn(shape[1], generator=g)
    rv = 0.5 + torch.rand(shape[1], generator=g)
    yref, By = bb.eval_forward_reference(x, gamma, beta, rm, rv, res, relu)
    o = run_bn(case, relu, False, rm, rv)
    bb.within("y", o["y"], yref, By)
    assert torch.equal(o["rm"].cpu(), rm) and torch.equal(o["rv"].cpu(), rv)
    inv = 1.0 / torch.sqrt(rv.double() + bb.EPS)
    bref = bb.backward_reference(x, gamma, gy, rm, inv, o["y"], relu, False)
    bb.within("gx", o["gx"], bref["gx"], bref["Bgx"])
    bb.within("gweight", o["gw"], bref["dg"], bref["Bdg"])
    bb.within("gbias", o["gb"], bref["db"], bref["Bdb"])
    if residual:
        assert torch.equal(o["gres"].double().cpu(), bref["g"])


def test_two_runs_are_bitwise_equal():
    case = bb.make_case(SPLIT_SHAPE, torch.float32, True)
    a, b = run_bn(case, True, True), run_bn(case, True, True)
    for name in ("y", "mean", "invstd", "gx", "gw", "gb", "gres"):
        assert torch.equal(a[name], b[name]), name


def test_bf16_y_is_the_fp32_y_rounded_once():
    x, gamma, beta, res, gy = bb.make_case((3, 72, 5, 5), torch.bfloat16,
                                           True)
    lo = run_bn((x, gamma, beta, res, gy), True, True)
    hi = run_bn((x.float(), gamma, beta, res.float(), gy.float()), True, True)
    assert torch.equal(lo["mean"], hi["mean"])
    assert torch.equal(lo["invstd"], hi["invstd"])
    assert torch.equal(lo["y"], hi["y"].bfloat16())


@pytest.mark.parametrize("dtype", DTYPES)
def test_misaligned_views_equal_their_clones(dtype):
    """x, the residual and gy one element off a 16-byte boundary: every
    kernel, forward and backward, runs one element per access and gives the
    bits of the 16-byte run."""
    shape = (3, 72, 5, 5)
    B, C, H, W = shape
    x, gamma, beta, res, gy = bb.make_case(shape, dtype, True)

    def at(t, off):     # t's values in channels-last storage at buf + off
        buf = torch.zeros(t.numel() + 8, dtype=dtype, device=DEV)
        v = buf[off:off + t.numel()].view(B, H, W, C).permute(0, 3, 1, 2)
        v.copy_(t)
        assert v.data_ptr() % 16 == off * t.element_size()
        return v

    out = []
    for off in (0, 1):
        xt = at(x, off).requires_grad_(True)
        rt = at(res, off).requires_grad_(True)
        wt = gamma.clone().to(DEV).requires_grad_(True)
        bt = beta.clone().to(DEV).requires_grad_(True)
        y = ops.batchnorm2d(xt, wt, bt, residual=rt, fuse_relu=True,
                            memory_format=CL)
        y.backward(at(gy, off))
        out.append((y.detach(), xt.grad, rt.grad, wt.grad, bt.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# pools
# ---------------------------------------------------------------------------
MAXPOOL_CASES = pc.MAXPOOL_CASES + [
    ((2, 8, 7, 9), 3, 2, 1),            # 16 bytes of bf16 per access
    ((2, 64, 9, 9), 3, 2, 1),           # ResNet's C, 8-byte slot stores
    ((1, 8, 6, 7), 5, 1, 2),            # run-time window, 25 windows/input
]


@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("case", MAXPOOL_CASES, ids=pc.case_id)
def test_maxpool2d_nhwc_equals_torch(case, dtype):
    pc.check_maxpool_exact(NHWC_OPS, case, dtype, DEV)


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_maxpool2d_nhwc_random_gy(dtype):
    pc.check_maxpool_random_gy(NHWC_OPS, dtype, DEV)


@pytest.mark.parametrize("dtype", pc.DTYPES)
@pytest.mark.parametrize("shape", pc.AVG_SHAPES + [(2, 136, 7, 7)])
def test_global_avgpool2d_nhwc(shape, dtype):
    pc.check_avg(NHWC_OPS, shape, dtype, DEV)


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_maxpool2d_nhwc_is_the_default_layout_bit_for_bit(dtype):
    shape, k, s, p = (2, 24, 9, 11), 3, 2, 1
    x = pc.maxpool_input(shape, dtype).to(DEV)
    gy = pc.random_gy(pc.out_shape(shape, k, s, p), dtype).to(DEV)
    y0, gx0 = pc.run_maxpool(ops, x, k, s, p, gy)
    y1, gx1 = pc.run_maxpool(NHWC_OPS, nhwc(x), k, s, p, nhwc(gy))
    assert is_nhwc(y1) and is_nhwc(gx1)
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)


def test_maxpool2d_nhwc_propagates_nan():
    x = pc.maxpool_input((1, 8, 6, 6), torch.float32)
    x[0, 3, 3, 3] = float("nan")      # in four windows
    y = NHWC_OPS.maxpool2d(x.to(DEV), 3, 2, 1).cpu()
    want = F.max_pool2d(x, 3, 2, 1)
    assert torch.isnan(want).sum() == 4
    assert torch.equal(torch.isnan(y), torch.isnan(want))
    assert torch.equal(y.nan_to_num(7.0), want.nan_to_num(7.0))


# ---------------------------------------------------------------------------
# models.resnet in channels-last mode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
def test_bottleneck_nhwc_is_the_ops_chained_by_hand(training):
    torch.manual_seed(0)
    bf16 = torch.bfloat16
    down = nn.Sequential(nn.Conv2d(64, 64, 1, stride=2, bias=False),
                         nn.BatchNorm2d(64))
    blk = Bottleneck(64, 16, stride=2, downsample=down, compute_dtype=bf16,
                     memory_format=CL).to(DEV)
    g = torch.Generator().manual_seed(4)
    bns = dict(bn1=blk.bn1, bn2=blk.bn2, bn3=blk.bn3, down=down[1])
    with torch.no_grad():
        for m in bns.values():
            m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
            m.bias.copy_(torch.randn(m.bias.shape, generator=g))
            m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    blk.train(training)
    x = torch.randn(3, 64, 10, 10, generator=g).bfloat16().to(DEV)
    conv = functools.partial(ops.conv2d_bf16, out_dtype=bf16,
                             memory_format=CL)

    def bn(name, h, **kw):      # on copies of the running buffers
        m = bns[name]
        return ops.batchnorm2d(h, m.weight, m.bias, *bufs[name],
                               training=training, momentum=m.momentum,
                               eps=m.eps, memory_format=CL, **kw)

    bufs = {n: (m.running_mean.clone(), m.running_var.clone())
            for n, m in bns.items()}
    with torch.no_grad():
        h = bn("bn1", conv(x, blk.conv1.weight, None), fuse_relu=True)
        h = bn("bn2", conv(h, blk.conv2.weight, None, stride=2, padding=1),
               fuse_relu=True)
        idn = bn("down", conv(x, down[0].weight, None, stride=2))
        want = bn("bn3", conv(h, blk.conv3.weight, None), residual=idn,
                  fuse_relu=True)
        got = blk(x)
    assert got.dtype == bf16 and got.shape == (3, 64, 5, 5) and is_nhwc(got)
    assert torch.equal(got, want)
    for n, m in bns.items():
        assert torch.equal(m.running_mean, bufs[n][0])
        assert torch.equal(m.running_var, bufs[n][1])


def test_tiny_resnet_nhwc_converges():
    def losses(**mode):
        torch.manual_seed(0)
        net = ResNet((1, 1, 1, 1), num_classes=10, **mode).to(DEV).train()
        x, tgt = (t.to(DEV) for t in bb.tiny_resnet_batch())
        opt = torch.optim.SGD(net.parameters(), lr=bb.TINY_LR)
        out = []
        for _ in range(bb.TINY_STEPS + 1):
            opt.zero_grad()
            loss = F.cross_entropy(net(x), tgt)
            loss.backward()
            out.append(float(loss.detach()))
            opt.step()
        return out

    ref = losses()
    got = losses(compute_dtype=torch.bfloat16, memory_format=CL)
    l0, l_ref, l_cl = ref[0], ref[-1], got[-1]
    print(f"fp32 {l0:.4f} -> {l_ref:.4f}; "
          f"nhwc bf16 {got[0]:.4f} -> {l_cl:.4f}")
    assert l_ref < 0.5 * l0, ref
    assert l_cl <= l0 - 0.5 * (l0 - l_ref), (ref, got)
