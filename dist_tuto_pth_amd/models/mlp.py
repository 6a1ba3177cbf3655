"""MLP on the same CDNA4 HIP op layer as `Net` — demonstrates that the
op layer (`dist_tuto_pth_amd.ops`) generalizes beyond the reference's
exact ConvNet shapes: arbitrary-width `linear` (+fused ReLU), dropout,
and the fused log_softmax+NLL loss all take any (B, K, N).

Not part of the reference surface (the tutorial ships exactly one
model, train_dist.py:53-71); provided as the second model family for
the training loop and the DP path.
"""

from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn

from .. import ops


class MLP(nn.Module):
    """`widths` = [in, hidden..., out]; ReLU (fused into the linear
    kernel) + dropout between layers, log_softmax output.

    ``compute_dtype=torch.bfloat16`` selects mixed precision: parameters
    and their gradients stay fp32, every layer runs `ops.linear_bf16`
    (bf16 operands on the matrix cores, fp32 accumulation), hidden
    activations and dropout are bf16, and the last layer returns fp32
    logits so the loss kernels are the fp32 ones.

    ``compute_dtype=torch.float8_e4m3fn`` is the same arrangement on
    `ops.linear_fp8`: operands quantised to fp8 per tensor on the 128-deep
    matrix instruction, bf16 hidden activations and dropout, fp32 logits,
    fp32 parameters and gradients under the same names, so a ``state_dict``
    moves between all three modes.  ``fp8_scaling="mx"`` (fp8 mode only)
    runs it with MXFP8 block scaling, ``ops.linear_fp8(scaling="mx")``: one
    e8m0 scale per 32 elements instead of one per tensor."""

    def __init__(self, widths: Sequence[int] = (784, 256, 128, 10),
                 dropout: float = 0.2,
                 compute_dtype: Optional[torch.dtype] = None,
                 fp8_scaling: str = "tensor"):
        super().__init__()
        assert len(widths) >= 2
        if compute_dtype not in (None, torch.bfloat16, torch.float8_e4m3fn):
            raise ValueError(
                f"MLP: compute_dtype must be None, torch.bfloat16 or "
                f"torch.float8_e4m3fn, got {compute_dtype}")
        if fp8_scaling not in ("tensor", "mx"):
            raise ValueError(f"MLP: fp8_scaling must be 'tensor' or 'mx', "
                             f"got {fp8_scaling!r}")
        if fp8_scaling != "tensor" and compute_dtype != torch.float8_e4m3fn:
            raise ValueError("MLP: fp8_scaling needs "
                             "compute_dtype=torch.float8_e4m3fn")
        self.compute_dtype = compute_dtype
        self.fp8_scaling = fp8_scaling
        self.widths = list(widths)
        self.p = dropout
        self.layers = nn.ModuleList(
            nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))

    def forward_logits(self, x: torch.Tensor) -> torch.Tensor:
        x = x.reshape(x.shape[0], self.widths[0])
        for i, lin in enumerate(self.layers):
            last = i == len(self.layers) - 1
            out_dtype = torch.float32 if last else torch.bfloat16
            if self.compute_dtype == torch.bfloat16:
                x = ops.linear_bf16(x, lin.weight, lin.bias,
                                    fuse_relu=not last, out_dtype=out_dtype)
            elif self.compute_dtype is not None:
                x = ops.linear_fp8(x, lin.weight, lin.bias,
                                   fuse_relu=not last, out_dtype=out_dtype,
                                   scaling=self.fp8_scaling)
            else:
                x = ops.linear(x, lin.weight, lin.bias, fuse_relu=not last)
            if not last:
                x = ops.dropout(x, p=self.p, training=self.training)
        return x

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.log_softmax(self.forward_logits(x))
