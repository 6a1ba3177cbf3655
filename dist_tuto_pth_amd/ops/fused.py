"""Fused whole-Net training step (GPU fast path).

Four dispatches per training step instead of ~30 per-op launches:
one kernel for the entire forward (conv1..log_softmax+NLL,
train_dist.py:64-71 + :120; 512 threads, both convs as 2x8 output blocks
fed by 16-byte LDS reads with the pool fused in registers, conv2's input
channels split over lanes and summed through LDS in a fixed order, two
sibling workgroups per sample at small batches, per-block loss partials;
DTP_FWD_TILED=0 selects the earlier 256-thread kernels), one for the
data backward (sibling-workgroup split,
2x4-tile register-blocked transposed conv with the conv2 channels split
over lanes), one segmented partial
weight-gradient kernel ([conv2 x8 | conv1 x8 | fc1 | fc2] tiles x batch
chunks), and one combine kernel that also finalizes the loss, advances
the dropout seed, and (single-GPU) applies the SGD+momentum update.
The kernels and their launchers are csrc/net_fused.hip; rocprof
evidence and the optimization ladder live in profiles/.
Numerically identical to the modular path in eval mode; dropout masks
use the same device-seed stream but a different indexing, so
train-mode losses match only in distribution.

Seed convention (all fused paths): a training step CONSUMES the current
device seed and the combine kernel at the end of backward ADVANCES it —
bump-after everywhere, so the autograd path (net_fused_loss) and the
fused-step paths can interleave without reusing dropout masks.  A
train-mode forward without a matching backward does not advance the
seed.
"""

from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from ..utils.native import load_native
from . import _seed_ptr, _stream


class _Workspace:
    """Per-(batch size, device) buffers shared by every fused entry
    point.  Read-only: the tensors are never replaced, so ``ptrs`` —
    their addresses in the native module's ``ws_fields`` order, the one
    vector every native call takes — stays valid for the process."""

    __slots__ = ("_tensors", "ptrs")

    def __init__(self, k, B: int, device):
        f = lambda *shape: torch.empty(*shape, device=device)  # noqa: E731
        u8 = lambda *shape: torch.empty(*shape, device=device,  # noqa: E731
                                        dtype=torch.uint8)
        t = {
            "p1": f(B, 1440), "idx1": u8(B, 1440), "m2": u8(B, 20),
            "p2": f(B, 320), "idx2": u8(B, 320), "h1": f(B, 50),
            "m3": u8(B, 50), "d3": f(B, 50), "logp": f(B, 10),
            "glog": f(B, 10), "gh1": f(B, 50), "ga2": f(B, 1280),
            "ga1": f(B, 5760), "part": f(k.GW_MAX_CH, k.GW_ROW),
            # loss_part must cover the LARGEST forward grid any caller
            # can launch (grid_for(B,1) <= 4096) — sized once here so
            # every entry point shares a safe buffer regardless of
            # which ran first (advisor r1 finding #1)
            "loss_part": f(4096), "loss": f(()),
            "one": torch.ones((), device=device),  # the loss gradient
        }
        object.__setattr__(self, "_tensors", t)
        object.__setattr__(self, "ptrs",
                           tuple(t[n].data_ptr() for n in k.ws_fields))

    def __getitem__(self, name: str) -> torch.Tensor:
        return self._tensors[name]

    def __setattr__(self, name, value):
        raise AttributeError("the fused workspace is read-only")


_ws_cache: Dict[Tuple, _Workspace] = {}


def _ws(B: int, device) -> _Workspace:
    key = (B, device.index)
    w = _ws_cache.get(key)
    if w is None:
        w = _ws_cache[key] = _Workspace(load_native("_kernels"), B, device)
    return w


def _reject_bf16(net, entry: str) -> None:
    """The fused kernels are fp32 only; a bf16-mode Net must not run them
    silently in fp32.  Every entry point checks ``compute_dtype`` inline
    (one attribute read per step) and comes here to raise."""
    raise TypeError(
        f"{entry}: the fused whole-Net kernels are fp32 only, but this Net "
        f"has compute_dtype={net.compute_dtype}; use the modular path "
        f"(net.forward_logits + ops.log_softmax_nll) or build the Net with "
        f"compute_dtype=None")


def _params(net) -> List[torch.Tensor]:
    """Net's 8 parameters in kernel order, each with a ``.grad`` to
    overwrite.  Pointers are read from these on every call: they can
    move (``attach_flat_grads`` re-points the grads)."""
    params = [net.conv1.weight, net.conv1.bias, net.conv2.weight,
              net.conv2.bias, net.fc1.weight, net.fc1.bias,
              net.fc2.weight, net.fc2.bias]
    for p in params:
        if p.grad is None:
            p.grad = torch.empty_like(p)
    return params


def _ptrs(tensors) -> List[int]:
    return [t.data_ptr() for t in tensors]


def _sgd(opt, params):
    """(param ptrs, momentum-buffer ptrs, lr, momentum) of the in-kernel
    FusedSGD update; an empty param list means no update."""
    if opt is None:
        return [], [], 0.0, 0.0
    return (_ptrs(params), _ptrs(opt._bufs) if opt._bufs else [],
            opt.lr, opt.momentum)


def attach_flat_grads(net) -> torch.Tensor:
    """Point every parameter's ``.grad`` at a slice of ONE flat buffer
    so the DP gradient average is a single all-reduce with no
    pack/unpack copies (the xGMI-friendly layout: one large message
    instead of 8 tiny ones — SURVEY.md §5 'bucketed').  Returns the
    flat buffer."""
    params = [p for p in net.parameters()]
    total = sum(p.numel() for p in params)
    flat = torch.zeros(total, device=params[0].device)
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    return flat


class _NetFusedLoss(torch.autograd.Function):
    # legacy loss mode (use_loss_part=False): the forward accumulates
    # the loss scalar atomically, so it is complete before backward

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, wf1, bf1, wf2, bf2, tgt, training):
        k = load_native("_kernels")
        B = x.shape[0]
        ws = _ws(B, x.device)
        params = (w1, b1, w2, b2, wf1, bf1, wf2, bf2)
        k.net_fused_fwd(x.data_ptr(), _ptrs(params), tgt.data_ptr(),
                        ws.ptrs, False, _seed_ptr(x.device), B, training,
                        _stream())
        ctx.save_for_backward(x, w2, wf1, wf2, tgt)
        ctx.meta = (B, training)
        ctx.shapes = [p.shape for p in params]
        return ws["loss"].clone()

    @staticmethod
    def backward(ctx, gl):
        k = load_native("_kernels")
        x, w2, wf1, wf2, tgt = ctx.saved_tensors
        B, training = ctx.meta
        ws = _ws(B, x.device)
        grads = [torch.empty(s, device=x.device) for s in ctx.shapes]
        gl = gl.contiguous()
        k.net_fused_bwd(x.data_ptr(), w2.data_ptr(), wf1.data_ptr(),
                        wf2.data_ptr(), tgt.data_ptr(), gl.data_ptr(),
                        ws.ptrs, _ptrs(grads), [], [], 0.0, 0.0, B,
                        training, False, _seed_ptr(x.device), _stream())
        return (None, *grads, None, None)


def _fwd_bwd(net, x, tgt, opt) -> torch.Tensor:
    # loss_part mode: no prologue dispatch — the forward writes
    # per-block loss partials (fwd grid <= 4096 at any B); the combine
    # kernel finalizes the loss scalar and bumps the dropout seed
    k = load_native("_kernels")
    B = x.shape[0]
    ws = _ws(B, x.device)
    params = _params(net)
    prm = _ptrs(params)
    s = _stream()
    k.net_fused_fwd(x.data_ptr(), prm, tgt.data_ptr(), ws.ptrs, True,
                    _seed_ptr(x.device), B, net.training, s)
    k.net_fused_bwd(x.data_ptr(), prm[2], prm[4], prm[6], tgt.data_ptr(),
                    ws["one"].data_ptr(), ws.ptrs,
                    _ptrs(p.grad for p in params), *_sgd(opt, params), B,
                    net.training, True, _seed_ptr(x.device), s)
    return ws["loss"]


def net_fused_step(net, x: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """Forward + backward in one call, OVERWRITING each parameter's
    ``.grad`` (no autograd graph, no accumulate-add kernels — the
    minimal-launch training step used by bench.py).  Returns the loss
    as a device scalar (no host sync)."""
    if getattr(net, "compute_dtype", None) is not None:
        _reject_bf16(net, "net_fused_step")
    return _fwd_bwd(net, x, tgt, None)


def net_fused_step_opt(net, x: torch.Tensor, tgt: torch.Tensor,
                       opt) -> torch.Tensor:
    """``net_fused_step`` with the SGD+momentum update fused into the
    combine kernel (one dispatch fewer; single-GPU training only — the
    DP path needs the all-reduce between combine and step).  ``opt``
    must be a FusedSGD; its momentum buffers are updated in-kernel."""
    if getattr(net, "compute_dtype", None) is not None:
        _reject_bf16(net, "net_fused_step_opt")
    return _fwd_bwd(net, x, tgt, opt)


def net_fused_step_fb(net, x: torch.Tensor, tgt: torch.Tensor,
                      opt=None) -> torch.Tensor:
    """Three-dispatch training step: forward AND data-backward share
    ONE kernel (each workgroup runs its sample's fwd then immediately
    its bwd — valid because the loss gradient is the constant 1 in the
    training loop), then gw-partial, then combine.  With ``opt`` (a
    FusedSGD) the combine also applies the update; without it, grads
    land in ``.grad`` for the DP all-reduce.  Trade-off vs
    net_fused_step: one dispatch + w2 re-staging saved, but the
    backward loses its sibling-workgroup split (grid = B), so at small
    B the chip is underfilled — measured, see profiles/."""
    if getattr(net, "compute_dtype", None) is not None:
        _reject_bf16(net, "net_fused_step_fb")
    k = load_native("_kernels")
    B = x.shape[0]
    ws = _ws(B, x.device)
    params = _params(net)
    k.net_fused_fwdbwd(x.data_ptr(), _ptrs(params), tgt.data_ptr(), ws.ptrs,
                       _ptrs(p.grad for p in params), *_sgd(opt, params), B,
                       net.training, _seed_ptr(x.device), _stream())
    return ws["loss"]


def net_step_available() -> bool:
    """True when the device supports the single-launch cooperative
    training-step kernel (hipLaunchCooperativeKernel)."""
    try:
        return bool(load_native("_kernels").net_step_available())
    except Exception:
        return False


def net_fused_train_step(net, x: torch.Tensor, tgt: torch.Tensor,
                         opt=None, do_sgd: bool = True) -> torch.Tensor:
    """The WHOLE training step — forward, backward, weight-gradient
    reduction and (optionally) the SGD+momentum update — in ONE
    cooperative kernel launch (csrc/net_fused.hip net_step_kernel).

    The 6-dispatch fused path pays a ~4.5 us device dispatch floor per
    kernel at the reference's batch sizes; this replaces them with one
    dispatch and grid barriers.  Gradients are still written to each
    parameter's ``.grad`` (so the DP path can all-reduce them when
    ``do_sgd=False``).  ``opt`` must be a FusedSGD when ``do_sgd`` —
    its momentum buffers are updated in-kernel.  Returns the loss as a
    device scalar (no host sync).
    """
    if getattr(net, "compute_dtype", None) is not None:
        _reject_bf16(net, "net_fused_train_step")
    k = load_native("_kernels")
    B = x.shape[0]
    ws = _ws(B, x.device)
    params = _params(net)
    _, bufs, lr, mu = _sgd(opt if do_sgd else None, params)
    k.net_step(x.data_ptr(), tgt.data_ptr(), ws["one"].data_ptr(), ws.ptrs,
               _seed_ptr(x.device), _ptrs(params),
               _ptrs(p.grad for p in params), bufs, lr, mu, do_sgd, B,
               net.training, _stream())
    return ws["loss"]


def net_fused_loss(net, x: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """Mean NLL loss of ``net`` (a models.Net) on (x, tgt), computed by
    the fused kernels.  Gradients flow to the 8 parameters."""
    if getattr(net, "compute_dtype", None) is not None:
        _reject_bf16(net, "net_fused_loss")
    assert x.is_cuda, "fused path is the GPU fast path"
    return _NetFusedLoss.apply(
        x.contiguous(), net.conv1.weight, net.conv1.bias,
        net.conv2.weight, net.conv2.bias, net.fc1.weight, net.fc1.bias,
        net.fc2.weight, net.fc2.bias, tgt.contiguous(), net.training)
