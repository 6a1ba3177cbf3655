"""ops.conv2d_bf16(bn_stats=True), ops.batchnorm2d(batch_stats=) and
models.resnet's fused_bn_stats as far as they show without a GPU, and that
test_conv_bn_stats_gpu.py's bias-100 case separates a centred variance from
E[x^2]-E[x]^2."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_bounds as bb  # noqa: E402
from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.models.resnet import ResNet, resnet50  # noqa: E402

CL = torch.channels_last


def conv_case(bias=None, seed=0):
    # test_conv_bn_stats_gpu.py's M429 case: unit-variance output
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(3, 8, 13, 11, generator=g)
    w = torch.randn(20, 8, 3, 3, generator=g) / 72 ** 0.5
    b = None if bias is None else torch.full((20,), float(bias))
    return x, w, b


def pair(x, w, b, fused, gamma, beta, gy):
    xt, wt = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    o = ops.conv2d_bf16(xt, wt, b, 1, 1, torch.float32, memory_format=CL,
                        bn_stats=fused)
    out, st = o if fused else (o, None)
    rm, rv = torch.zeros(20), torch.ones(20)
    y = ops.batchnorm2d(out, gamma, beta, rm, rv, training=True,
                        momentum=1.0, memory_format=CL, batch_stats=st)
    y.backward(gy)
    return out.detach(), st, (y.detach(), rm, rv, xt.grad, wt.grad)


def test_fused_statistics_need_channels_last():
    x, w, _ = conv_case()
    with pytest.raises(ValueError, match="channels_last"):
        ops.conv2d_bf16(x, w, bn_stats=True)
    with pytest.raises(ValueError, match="fused_bn_stats"):
        resnet50(compute_dtype=torch.bfloat16, fused_bn_stats=True)


@pytest.mark.parametrize("how", ["eval", "default_layout", "other_shape",
                                 "other_tensor"])
def test_batch_stats_is_refused(how):
    x, w, _ = conv_case()
    out, st = ops.conv2d_bf16(x, w, None, 1, 1, memory_format=CL,
                              bn_stats=True)
    assert st.partials is None and st.is_cpu and st.rows == 429 and st.K == 20
    kw = dict(training=how != "eval",
              memory_format=torch.contiguous_format
              if how == "default_layout" else CL)
    t = {"other_shape": out[:, :, :-1], "other_tensor": out.clone()}\
        .get(how, out)
    C = t.shape[1]
    with pytest.raises(ValueError, match="batch_stats"):
        ops.batchnorm2d(t, torch.ones(C), torch.zeros(C), torch.zeros(C),
                        torch.ones(C), batch_stats=st, **kw)


def test_cpu_fused_pair_is_the_unfused_pair():
    x, w, b = conv_case(bias=0.5)
    _, gamma, beta, _, gy = bb.make_case((3, 20, 13, 11), torch.float32,
                                         False)
    out_f, _, got = pair(x, w, b, True, gamma, beta, gy)
    out_p, _, want = pair(x, w, b, False, gamma, beta, gy)
    assert torch.equal(out_f, out_p)
    for a, e in zip(got, want):
        assert torch.equal(a, e)


def test_bias_100_case_separates_centred_from_raw_moment():
    x, w, b = conv_case(bias=100)
    gamma, beta = torch.ones(20), torch.zeros(20)
    out, _, (y, rm, rv, _, _) = pair(x, w, b, True, gamma, beta,
                                     torch.zeros(3, 20, 13, 11))
    ref = bb.forward_reference(out, gamma, beta, None, False)
    n = ref["n"]
    bb.within("var", rv, ref["v"] * n / (n - 1), ref["Bv"] * n / (n - 1))
    raw = (out * out).mean(dim=(0, 2, 3)) - out.mean(dim=(0, 2, 3)) ** 2
    err = (raw.double() - ref["v"]).abs()
    assert bool((err > ref["Bv"]).any())


def test_fused_resnet_has_the_same_state():
    kw = dict(num_classes=10, compute_dtype=torch.bfloat16, memory_format=CL)
    torch.manual_seed(0)
    plain = ResNet((1, 1, 1, 1), **kw)
    torch.manual_seed(0)
    fused = ResNet((1, 1, 1, 1), fused_bn_stats=True, **kw)
    a, b = plain.state_dict(), fused.state_dict()
    assert list(a) == list(b)
    assert all(torch.equal(a[k], b[k]) for k in a)
    x, _ = bb.tiny_resnet_batch(B=2)
    assert torch.equal(plain.train()(x), fused.train()(x))   # CPU: same bits
    assert torch.equal(plain.eval()(x), fused.eval()(x))
