"""ResNet-50 for the bucketed-overlap DP benchmark (BASELINE.md
config 4: "ResNet-50 on synthetic 3x224x224, bucketed grad all-reduce
overlapped with backward, 8 GPUs").

The reference has no model beyond the 21,840-param ConvNet; this is the
standard ResNet-50 architecture (He et al. 2015: conv7x7/2 - maxpool -
[3,4,6,3] bottleneck stages x (1x1,3x3,1x1) with expansion 4 - avgpool
- fc1000, ~25.6M params) written directly against torch.nn — by default
the compute runs on torch-ROCm (MIOpen/rocBLAS) while the DISTRIBUTED path
(bucketed all-reduce overlapped with backward over RCCL/xGMI) is this
package's own DistributedDataParallel, which is what config 4 measures.
torchvision is not available in this environment.

``compute_dtype=torch.bfloat16`` (on ``Bottleneck``, ``ResNet`` and
``resnet50``) is the mixed-precision form on this package's own HIP ops,
in the contract of ``Net`` and ``MLP``: parameters, their gradients and
the BN running buffers stay fp32 and live in the same ``nn.Conv2d`` /
``nn.BatchNorm2d`` / ``nn.Linear`` holders under the same names, so a
``state_dict`` moves between the two modes unchanged.  Every conv (the
7x7/2 stem and the 1x1 downsample convs included) runs
``ops.conv2d_bf16`` with bf16 output, every BN ``ops.batchnorm2d`` on the
module's own weight, bias, running buffers, momentum and eps, with the
ReLU fused into bn1 and bn2 and the residual add and final ReLU fused
into bn3, so a block's tail is one kernel.  ``self.training`` selects
batch or running statistics.  The classifier is ``ops.linear_bf16`` with
fp32 logits.  The stem's 3x3/2 max-pool is ``ops.maxpool2d`` with the
``self.maxpool`` holder's kernel size, stride and padding, and the head's
global average pool is ``ops.global_avgpool2d``, which already returns
[B,C]: no op of this mode's forward or backward is borrowed from torch.
``num_batches_tracked`` is not touched: torch reads it only when
``momentum=None``, which ``ops.batchnorm2d`` does not support.

``memory_format=torch.channels_last`` (only with
``compute_dtype=torch.bfloat16``) passes that keyword to every conv, BN and
pool of the bf16 forward.  The stem conv lays the input batch out
[B][H][W][C]; from there to the [B,C] pooled vector every activation and
every gradient has channels-last storage, so no op copies a layout.
Parameters, buffers and ``state_dict`` are the same in both layouts.

``fused_bn_stats=True`` (only with ``memory_format=torch.channels_last``)
makes every convolution that feeds a batch norm in training mode — the
stem, the three of a block and the downsample — reduce its own output
tiles to partial batch statistics (``ops.conv2d_bf16(..., bn_stats=True)``)
and hands them to that batch norm (``batch_stats=``), which then skips its
two statistics passes over the tensor.  Eval mode, parameters, buffers and
``state_dict`` do not change.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops


def _check_compute_dtype(who, compute_dtype):
    if compute_dtype not in (None, torch.bfloat16):
        raise ValueError(
            f"{who}: compute_dtype must be None or torch.bfloat16, "
            f"got {compute_dtype}")
    return compute_dtype


def _check_memory_format(who, memory_format, compute_dtype):
    if memory_format not in (torch.contiguous_format, torch.channels_last):
        raise ValueError(
            f"{who}: memory_format must be torch.contiguous_format or "
            f"torch.channels_last, got {memory_format}")
    if memory_format == torch.channels_last and compute_dtype is None:
        raise ValueError(
            f"{who}: memory_format=torch.channels_last needs "
            f"compute_dtype=torch.bfloat16")
    return memory_format


def _check_fused_bn_stats(who, fused_bn_stats, memory_format):
    if fused_bn_stats and memory_format != torch.channels_last:
        raise ValueError(
            f"{who}: fused_bn_stats=True needs "
            f"memory_format=torch.channels_last")
    return bool(fused_bn_stats)


def _layout_kw(memory_format):
    """What the bf16 forward adds to every conv, BN and pool call: nothing
    in the default layout, whose calls stay exactly as they were."""
    if memory_format == torch.channels_last:
        return {"memory_format": memory_format}
    return {}


def _conv_bf16(conv, x, **layout):
    return ops.conv2d_bf16(x, conv.weight, None, stride=conv.stride,
                           padding=conv.padding, out_dtype=torch.bfloat16,
                           **layout)


def _bn(bn, x, residual=None, fuse_relu=False, **layout):
    return ops.batchnorm2d(x, bn.weight, bn.bias, bn.running_mean,
                           bn.running_var, training=bn.training,
                           momentum=bn.momentum, eps=bn.eps,
                           residual=residual, fuse_relu=fuse_relu, **layout)


def _conv_bn(conv, bn, x, fused, residual=None, fuse_relu=False, **layout):
    """bn(conv(x)); with ``fused`` and a batch norm in training mode the
    convolution computes the batch statistics' partials on the way."""
    if not (fused and bn.training):
        return _bn(bn, _conv_bf16(conv, x, **layout), residual, fuse_relu,
                   **layout)
    out, stats = ops.conv2d_bf16(x, conv.weight, None, stride=conv.stride,
                                 padding=conv.padding,
                                 out_dtype=torch.bfloat16, bn_stats=True,
                                 **layout)
    return ops.batchnorm2d(out, bn.weight, bn.bias, bn.running_mean,
                           bn.running_var, training=True,
                           momentum=bn.momentum, eps=bn.eps,
                           residual=residual, fuse_relu=fuse_relu,
                           batch_stats=stats, **layout)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, in_ch, width, stride=1, downsample=None,
                 compute_dtype: Optional[torch.dtype] = None,
                 memory_format=torch.contiguous_format,
                 fused_bn_stats=False):
        super().__init__()
        self.compute_dtype = _check_compute_dtype("Bottleneck", compute_dtype)
        self.memory_format = _check_memory_format(
            "Bottleneck", memory_format, compute_dtype)
        self.fused_bn_stats = _check_fused_bn_stats(
            "Bottleneck", fused_bn_stats, memory_format)
        out_ch = width * self.expansion
        self.conv1 = nn.Conv2d(in_ch, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1,
                               bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, out_ch, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_ch)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def _forward_bf16(self, x):
        mf = _layout_kw(self.memory_format)
        fu = self.fused_bn_stats
        out = _conv_bn(self.conv1, self.bn1, x, fu, fuse_relu=True, **mf)
        out = _conv_bn(self.conv2, self.bn2, out, fu, fuse_relu=True, **mf)
        identity = x
        if self.downsample is not None:
            identity = _conv_bn(self.downsample[0], self.downsample[1], x, fu,
                                **mf)
        return _conv_bn(self.conv3, self.bn3, out, fu, residual=identity,
                        fuse_relu=True, **mf)

    def forward(self, x):
        if self.compute_dtype is not None:
            return self._forward_bf16(x)
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), num_classes=1000,
                 compute_dtype: Optional[torch.dtype] = None,
                 memory_format=torch.contiguous_format,
                 fused_bn_stats=False):
        super().__init__()
        self.compute_dtype = _check_compute_dtype("ResNet", compute_dtype)
        self.memory_format = _check_memory_format(
            "ResNet", memory_format, compute_dtype)
        self.fused_bn_stats = _check_fused_bn_stats(
            "ResNet", fused_bn_stats, memory_format)
        self.in_ch = 64
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512 * Bottleneck.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def _make_layer(self, width, blocks, stride=1):
        downsample = None
        out_ch = width * Bottleneck.expansion
        if stride != 1 or self.in_ch != out_ch:
            downsample = nn.Sequential(
                nn.Conv2d(self.in_ch, out_ch, 1, stride=stride,
                          bias=False),
                nn.BatchNorm2d(out_ch))
        layers = [Bottleneck(self.in_ch, width, stride, downsample,
                             compute_dtype=self.compute_dtype,
                             memory_format=self.memory_format,
                             fused_bn_stats=self.fused_bn_stats)]
        self.in_ch = out_ch
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.in_ch, width,
                                     compute_dtype=self.compute_dtype,
                                     memory_format=self.memory_format,
                                     fused_bn_stats=self.fused_bn_stats))
        return nn.Sequential(*layers)

    def forward(self, x):
        if self.compute_dtype is not None:
            mf = _layout_kw(self.memory_format)
            x = _conv_bn(self.conv1, self.bn1, x, self.fused_bn_stats,
                         fuse_relu=True, **mf)
            x = ops.maxpool2d(x, self.maxpool.kernel_size,
                              self.maxpool.stride, self.maxpool.padding, **mf)
            x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
            x = ops.global_avgpool2d(x, **mf)
            return ops.linear_bf16(x, self.fc.weight, self.fc.bias,
                                   out_dtype=torch.float32)
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.avgpool(x).flatten(1)
        return self.fc(x)


def resnet50(num_classes=1000,
             compute_dtype: Optional[torch.dtype] = None,
             memory_format=torch.contiguous_format,
             fused_bn_stats=False) -> ResNet:
    return ResNet((3, 4, 6, 3), num_classes, compute_dtype=compute_dtype,
                  memory_format=memory_format, fused_bn_stats=fused_bn_stats)
