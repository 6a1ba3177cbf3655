"""The reference ConvNet (train_dist.py:53-71), built on this package's
CDNA4 HIP ops.

Architecture (21,840 params, SURVEY.md §2.1 'Net'):
  conv1: Conv2d(1,10,k=5)   B x 1 x 28 x 28 -> B x 10 x 24 x 24
  pool+relu (fused)                         -> B x 10 x 12 x 12
  conv2: Conv2d(10,20,k=5)                  -> B x 20 x 8 x 8
  dropout2d -> pool+relu (fused)            -> B x 20 x 4 x 4 -> flat 320
  fc1: Linear(320,50) + fused ReLU -> dropout
  fc2: Linear(50,10) -> log_softmax(dim=1)

The reference's ``log_softmax`` without a ``dim`` argument
(train_dist.py:71) meant dim=1 on 2-D input; made explicit here
(SURVEY.md §2.5.4).  Parameters live in stock ``nn.Conv2d``/``nn.Linear``
holders (same init semantics as the reference); compute goes through
``dist_tuto_pth_amd.ops`` — HIP kernels on GPU, the plain-torch fp32
reference on CPU.

``Net(compute_dtype=torch.bfloat16)`` is the mixed-precision form, as
``MLP`` has it: parameters and their gradients stay fp32, both convs run
``ops.conv2d_bf16`` and both linears ``ops.linear_bf16`` (bf16 operands on
the matrix cores, fp32 accumulation), every activation between them is
bf16, and fc2 returns fp32 logits so the loss kernels are the fp32 ones.
The fused whole-Net step (``ops.fused``) is fp32 only.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops


class Net(nn.Module):
    def __init__(self, compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        if compute_dtype not in (None, torch.bfloat16):
            raise ValueError(
                f"Net: compute_dtype must be None or torch.bfloat16, "
                f"got {compute_dtype}")
        self.compute_dtype = compute_dtype
        self.conv1 = nn.Conv2d(1, 10, kernel_size=5)
        self.conv2 = nn.Conv2d(10, 20, kernel_size=5)
        self.conv2_drop = nn.Dropout2d()
        self.fc1 = nn.Linear(320, 50)
        self.fc2 = nn.Linear(50, 10)

    def _logits_bf16(self, x):
        bf16 = torch.bfloat16
        x = ops.conv2d_bf16(x, self.conv1.weight, self.conv1.bias,
                            out_dtype=bf16)
        x = ops.maxpool2d_relu(x)
        x = ops.conv2d_bf16(x, self.conv2.weight, self.conv2.bias,
                            out_dtype=bf16)
        x = ops.dropout2d(x, p=self.conv2_drop.p, training=self.training)
        x = ops.maxpool2d_relu(x)
        x = x.reshape(-1, 320)
        x = ops.linear_bf16(x, self.fc1.weight, self.fc1.bias,
                            fuse_relu=True, out_dtype=bf16)
        x = ops.dropout(x, p=0.5, training=self.training)
        return ops.linear_bf16(x, self.fc2.weight, self.fc2.bias,
                               out_dtype=torch.float32)

    def forward(self, x):
        if self.compute_dtype is not None:
            return ops.log_softmax(self._logits_bf16(x))
        x = ops.conv2d(x, self.conv1.weight, self.conv1.bias)
        x = ops.maxpool2d_relu(x)
        x = ops.conv2d(x, self.conv2.weight, self.conv2.bias)
        x = ops.dropout2d(x, p=self.conv2_drop.p, training=self.training)
        x = ops.maxpool2d_relu(x)
        x = x.reshape(-1, 320)
        x = ops.linear(x, self.fc1.weight, self.fc1.bias, fuse_relu=True)
        x = ops.dropout(x, p=0.5, training=self.training)
        x = ops.linear(x, self.fc2.weight, self.fc2.bias)
        return ops.log_softmax(x)

    def forward_logits(self, x):
        """Forward stopping before log_softmax — pairs with the fused
        ``ops.log_softmax_nll`` loss (K9+K10 fusion)."""
        if self.compute_dtype is not None:
            return self._logits_bf16(x)
        x = ops.conv2d(x, self.conv1.weight, self.conv1.bias)
        x = ops.maxpool2d_relu(x)
        x = ops.conv2d(x, self.conv2.weight, self.conv2.bias)
        x = ops.dropout2d(x, p=self.conv2_drop.p, training=self.training)
        x = ops.maxpool2d_relu(x)
        x = x.reshape(-1, 320)
        x = ops.linear(x, self.fc1.weight, self.fc1.bias, fuse_relu=True)
        x = ops.dropout(x, p=0.5, training=self.training)
        return ops.linear(x, self.fc2.weight, self.fc2.bias)
