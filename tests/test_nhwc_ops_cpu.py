"""CPU tests of ``memory_format=torch.channels_last`` on ops.batchnorm2d,
ops.maxpool2d, ops.global_avgpool2d and models.resnet: on CPU tensors the
keyword runs the default path's arithmetic and only lays the results out
channels-last, so every value is the default path's, bit for bit."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_bounds as bb  # noqa: E402
from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.models.resnet import ResNet, resnet50  # noqa: E402

CL = torch.channels_last
SHAPE = (3, 6, 5, 4)


def is_nhwc(t):
    return t.permute(0, 2, 3, 1).is_contiguous()


def both_layouts(op, dtype, *args, **kw):
    """(y, gx) of ``op(x, *args, **kw)`` in the default layout and in
    channels-last mode on the same values."""
    x, _, _, _, gy = bb.make_case(SHAPE, dtype, False)
    out = []
    for mf in (torch.contiguous_format, CL):
        # autograd lays a leaf's gradient out like the leaf
        xt = x.contiguous(memory_format=mf).clone().requires_grad_(True)
        y = op(xt, *args, memory_format=mf, **kw)
        y.backward(gy[:, :, :y.shape[2], :y.shape[3]] if y.dim() == 4
                   else gy[:, :, 0, 0])
        out.append((y.detach(), xt.grad))
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("op,args,kw", [
    (ops.batchnorm2d, (torch.rand(6) + 0.5, torch.randn(6)),
     dict(fuse_relu=True)),
    (ops.maxpool2d, (3, 2, 1), {}),
    (ops.global_avgpool2d, (), {}),
], ids=["batchnorm2d", "maxpool2d", "global_avgpool2d"])
def test_channels_last_is_the_default_path_laid_out(op, args, kw, dtype):
    (y0, gx0), (y1, gx1) = both_layouts(op, dtype, *args, **kw)
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    assert is_nhwc(gx1) and (y1.dim() == 2 or is_nhwc(y1))
    with pytest.raises(ValueError, match="memory_format"):
        op(torch.zeros(SHAPE), *args, memory_format=torch.preserve_format,
           **kw)


def test_split_rule():
    from dist_tuto_pth_amd.utils.native import load_native
    splits = load_native("_kernels").batchnorm2d_nhwc_splits
    assert splits(343, 6) == 2              # test_nhwc_ops_gpu's SPLIT_SHAPE
    assert splits(32 * 112 * 112, 64) == 128    # the stem fills the chip
    assert splits(32 * 49, 2048) == 24      # 32 column tiles x 24 slices
    assert splits(2, 5) == 1 and splits(127, 3) == 1


def test_tiny_resnet_is_wired_alike_in_both_layouts():
    x, tgt = bb.tiny_resnet_batch()
    out = []
    for mf in (torch.contiguous_format, CL):
        torch.manual_seed(0)
        net = ResNet((1, 1, 1, 1), num_classes=10,
                     compute_dtype=torch.bfloat16, memory_format=mf).train()
        logits = net(x)
        torch.nn.functional.cross_entropy(logits, tgt).backward()
        out.append([logits.detach()] + [p.grad for p in net.parameters()])
    assert len(out[0]) == len(out[1]) > 1
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_channels_last_needs_the_bf16_mode():
    with pytest.raises(ValueError, match="compute_dtype"):
        resnet50(memory_format=CL)
    with pytest.raises(ValueError, match="memory_format"):
        ResNet((1, 1, 1, 1), compute_dtype=torch.bfloat16,
               memory_format=torch.preserve_format)
