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


def _conv_bf16(conv, x):
    return ops.conv2d_bf16(x, conv.weight, None, stride=conv.stride,
                           padding=conv.padding, out_dtype=torch.bfloat16)


def _bn(bn, x, residual=None, fuse_relu=False):
    return ops.batchnorm2d(x, bn.weight, bn.bias, bn.running_mean,
                           bn.running_var, training=bn.training,
                           momentum=bn.momentum, eps=bn.eps,
                           residual=residual, fuse_relu=fuse_relu)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, in_ch, width, stride=1, downsample=None,
                 compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self.compute_dtype = _check_compute_dtype("Bottleneck", compute_dtype)
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
        out = _bn(self.bn1, _conv_bf16(self.conv1, x), fuse_relu=True)
        out = _bn(self.bn2, _conv_bf16(self.conv2, out), fuse_relu=True)
        identity = x
        if self.downsample is not None:
            identity = _bn(self.downsample[1],
                           _conv_bf16(self.downsample[0], x))
        return _bn(self.bn3, _conv_bf16(self.conv3, out), residual=identity,
                   fuse_relu=True)

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
                 compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        self.compute_dtype = _check_compute_dtype("ResNet", compute_dtype)
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
                             compute_dtype=self.compute_dtype)]
        self.in_ch = out_ch
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.in_ch, width,
                                     compute_dtype=self.compute_dtype))
        return nn.Sequential(*layers)

    def forward(self, x):
        if self.compute_dtype is not None:
            x = _bn(self.bn1, _conv_bf16(self.conv1, x), fuse_relu=True)
            x = ops.maxpool2d(x, self.maxpool.kernel_size,
                              self.maxpool.stride, self.maxpool.padding)
            x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
            x = ops.global_avgpool2d(x)
            return ops.linear_bf16(x, self.fc.weight, self.fc.bias,
                                   out_dtype=torch.float32)
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.avgpool(x).flatten(1)
        return self.fc(x)


def resnet50(num_classes=1000,
             compute_dtype: Optional[torch.dtype] = None) -> ResNet:
    return ResNet((3, 4, 6, 3), num_classes, compute_dtype=compute_dtype)
