"""Fused SGD + momentum optimizer (K11-K13 of SURVEY.md §2.4b).

The reference uses ``optim.SGD(lr=0.01, momentum=0.5)``
(train_dist.py:110) with ``optimizer.zero_grad()`` each step
(train_dist.py:118).  Here the whole update — momentum buffer update,
parameter step, and optional gradient zeroing (K12 folded in) — is ONE
multi-tensor HIP kernel launch on GPU; CPU falls back to the plain
formula (the golden reference for the GPU numerics test).

Update rule (torch SGD semantics, as the reference's optimizer):
    buf = mu * buf + grad ;  p -= lr * buf
With ``weight_decay`` the gradient is first replaced by
``g' = grad + weight_decay * p``; with ``nesterov`` the step direction is
``g' + mu * buf`` instead of ``buf``.  Both are compile-time variants of
the same kernel.  Dampening is not offered: torch's first-step special
case for it does not fit buffers that start at zero.
"""

from __future__ import annotations

from typing import Iterable

import torch

from .utils.native import load_native


def _require_dense_fp32(i, p, grad, buf):
    """The kernel walks parameter, gradient and momentum buffer as flat
    fp32 arrays of ``p.numel()`` elements: refuse anything else before its
    pointer reaches it."""
    for name, t in (("parameter", p), ("gradient", grad),
                    ("momentum buffer", buf)):
        if t is None:
            continue
        if t.device != p.device or not t.is_cuda:
            raise ValueError(f"FusedSGD.step: {name} {i} is on {t.device}, "
                             f"its parameter on {p.device}")
        if t.dtype != torch.float32:
            raise TypeError(f"FusedSGD.step is fp32 only on GPU, got "
                            f"{name} {i} of dtype {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"FusedSGD.step: {name} {i} must be "
                             f"contiguous, got strides {t.stride()}")
        if t.shape != p.shape:
            raise ValueError(f"FusedSGD.step: {name} {i} has shape "
                             f"{tuple(t.shape)}, its parameter "
                             f"{tuple(p.shape)}")


class FusedSGD:
    def __init__(self, params: Iterable[torch.Tensor], lr: float = 0.01,
                 momentum: float = 0.0, zero_grad_in_step: bool = False,
                 weight_decay: float = 0.0, nesterov: bool = False):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no parameters to optimize")
        if weight_decay < 0.0:
            raise ValueError(f"FusedSGD: weight_decay must be >= 0, got "
                             f"{weight_decay}")
        if nesterov and momentum == 0.0:
            raise ValueError("FusedSGD: nesterov=True needs a momentum "
                             "other than 0")
        self.weight_decay = weight_decay
        self.nesterov = bool(nesterov)
        self.lr = lr
        self.momentum = momentum
        self.zero_grad_in_step = zero_grad_in_step
        self._bufs = [torch.zeros_like(p) for p in self.params] \
            if momentum != 0.0 else None
        self._is_cuda = self.params[0].is_cuda

    @torch.no_grad()
    def step(self):
        if self._is_cuda:
            k = load_native("_kernels")
            ptrs_p, ptrs_g, ptrs_b, numels = [], [], [], []
            for i, p in enumerate(self.params):
                if p.grad is None:
                    continue
                buf = self._bufs[i] if self._bufs is not None else None
                _require_dense_fp32(i, p, p.grad, buf)
                ptrs_p.append(p.data_ptr())
                ptrs_g.append(p.grad.data_ptr())
                ptrs_b.append(buf.data_ptr() if buf is not None else 0)
                numels.append(p.numel())
            stream = torch.cuda.current_stream().cuda_stream
            if self.weight_decay == 0.0 and not self.nesterov:
                k.sgd_step(ptrs_p, ptrs_g, ptrs_b, numels, self.lr,
                           self.momentum, self.zero_grad_in_step, stream)
            else:
                k.sgd_step(ptrs_p, ptrs_g, ptrs_b, numels, self.lr,
                           self.momentum, self.zero_grad_in_step, stream,
                           self.weight_decay, self.nesterov)
            return
        for i, p in enumerate(self.params):
            if p.grad is None:
                continue
            g = p.grad
            if self.weight_decay != 0.0:
                g = g.add(p, alpha=self.weight_decay)
            if self._bufs is not None:
                buf = self._bufs[i]
                buf.mul_(self.momentum).add_(g)
                g = g.add(buf, alpha=self.momentum) if self.nesterov \
                    else buf
            p.add_(g, alpha=-self.lr)
            if self.zero_grad_in_step:
                p.grad.zero_()

    @torch.no_grad()
    def zero_grad(self):
        for p in self.params:
            if p.grad is not None:
                p.grad.zero_()
