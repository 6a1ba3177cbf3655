"""Training-path ops.

Every op the reference's ``Net.forward`` + SGD step trigger implicitly
through torch (train_dist.py:58-71,110,118-124) is a hand-written CDNA4
HIP kernel here, with forward *and* backward (``csrc/kernels.hip``; K3-K6
in ``csrc/pointwise.hip``, K16-K21 in the files named at their sections):

  K1/K2  conv2d (direct, LDS-tiled)        -> conv2d
  K3+K4  maxpool2d(k2) fused with ReLU     -> maxpool2d_relu (fp32, bf16)
  K4     ReLU                              -> relu
  K5/K6  dropout2d (channel) / dropout     -> dropout2d / dropout
                                              (fp32, bf16)
  K7/K8  linear (+fused ReLU epilogue)     -> linear
  K16    bf16 MFMA linear, fp32 accumulate  -> linear_bf16
  K17    bf16 MFMA conv2d (stride, padding) -> conv2d_bf16
  K18    batchnorm2d (+residual add, +ReLU) -> batchnorm2d
  K19    maxpool2d (kernel, stride, padding) -> maxpool2d (fp32, bf16)
  K20    global average pool [B,C,H,W]->[B,C] -> global_avgpool2d
                                              (fp32, bf16)
  K9+K10 log_softmax fused with NLL loss   -> log_softmax, nll_loss,
                                              log_softmax_nll
  K21    cross-entropy for wide rows (label   -> cross_entropy (fp32, bf16)
         smoothing, ignore_index, reduction)
  K11-13 fused multi-tensor SGD+momentum   -> optim.FusedSGD

Dispatch: GPU tensors REQUIRE the native extension (loud failure, no
eager fallback — the HIP path must be the one that runs on a GPU box);
CPU tensors run a plain-torch fp32 reference implementation of the same
op, which is also the golden model for the GPU numerics tests
(tests/test_ops_gpu.py).
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from ..utils.native import load_native


def _k():
    return load_native("_kernels")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t) -> int:
    """Device address of an optional tensor; 0 for ``None``."""
    return t.data_ptr() if t is not None else 0


def _require_fp32(op, hint="", **tensors):
    """The kernels behind ``op`` read and write fp32: refuse a CUDA tensor
    of any other dtype before its pointer reaches them."""
    for name, t in tensors.items():
        if t is not None and t.dtype != torch.float32 and t.is_cuda:
            raise TypeError(f"ops.{op} is fp32 only on GPU, got {name} of "
                            f"dtype {t.dtype}{hint}")


_INT_MAX = 2 ** 31 - 1   # the fp32 kernels index weights and planes in int


def _require_tensors(op, **tensors):
    for name, t in tensors.items():
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"ops.{op}: {name} must be a tensor")


def _require_same_device(op, x, **others):
    for name, t in others.items():
        if t is not None and t.device != x.device:
            raise ValueError(f"ops.{op}: {name} is on {t.device}, the input "
                             f"on {x.device}")


def _require_fits_int(op, **sizes):
    for what, v in sizes.items():
        if v > _INT_MAX:
            raise ValueError(f"ops.{op}: {what} = {v} does not fit the "
                             f"kernel's 32-bit index")


def _check_rows(op, name, x):
    """``x`` is the [B,N] matrix of a row-wise op."""
    if x.dim() != 2:
        raise ValueError(f"ops.{op}: {name} [B,N] expected, got "
                         f"{tuple(x.shape)}")
    if min(x.shape) < 1:
        raise ValueError(f"ops.{op}: B and N must be >= 1, got "
                         f"{tuple(x.shape)}")
    _require_fits_int(op, B=x.shape[0], N=x.shape[1])


def _check_target(op, x, target):
    """``target`` holds one int64 class index per row of ``x``.  Its values
    stay unchecked: reading them would synchronize with the device, which
    a captured graph forbids."""
    _require_tensors(op, target=target)
    if target.dtype != torch.int64:
        raise TypeError(f"ops.{op}: target must be int64, got "
                        f"{target.dtype}")
    if target.shape != (x.shape[0],):
        raise ValueError(f"ops.{op}: target must have shape "
                         f"[{x.shape[0]}], got {tuple(target.shape)}")
    _require_same_device(op, x, target=target)


# ---------------------------------------------------------------------------
# K1/K2 — direct convolution (no padding, stride 1: the only form Net uses)
# ---------------------------------------------------------------------------
class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        if x.is_cuda:
            k = _k()
            B, C, H, W = x.shape
            K, _, R, S = w.shape
            OH, OW = H - R + 1, W - S + 1
            out = torch.empty(B, K, OH, OW, device=x.device, dtype=x.dtype)
            k.conv2d_fwd(x.data_ptr(), w.data_ptr(), _ptr(b),
                         out.data_ptr(), B, C, H, W, K, R, S, _stream())
            return out
        return F.conv2d(x, w, b)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        if x.is_cuda:
            k = _k()
            B, C, H, W = x.shape
            K, _, R, S = w.shape
            # fully written by the kernels, in dense order
            gx = torch.empty(x.shape, device=x.device, dtype=x.dtype)
            gw = torch.empty(w.shape, device=x.device, dtype=x.dtype)
            gb = torch.empty(K, device=x.device, dtype=x.dtype) \
                if ctx.needs_input_grad[2] else None
            k.conv2d_bwd(x.data_ptr(), w.data_ptr(), gy.data_ptr(),
                         gx.data_ptr(), gw.data_ptr(), _ptr(gb),
                         B, C, H, W, K, R, S, _stream())
            return gx, gw, gb
        gx = torch.nn.grad.conv2d_input(x.shape, w, gy)
        gw = torch.nn.grad.conv2d_weight(x, w.shape, gy)
        gb = gy.sum(dim=(0, 2, 3)) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


def conv2d(x, w, b=None):
    """Valid cross-correlation, stride 1: ``x`` [B,C,H,W], ``w`` [K,C,R,S]
    and ``b`` [K] or None, fp32 on GPU, in any memory layout (the kernels
    read dense copies and return dense gradients)."""
    _require_tensors("conv2d", x=x, w=w, b=b)
    _require_fp32("conv2d", x=x, w=w, b=b)
    if x.dim() != 4 or w.dim() != 4:
        raise ValueError(f"ops.conv2d: x [B,C,H,W] and w [K,C,R,S] expected, "
                         f"got {tuple(x.shape)} and {tuple(w.shape)}")
    if x.shape[1] != w.shape[1]:
        raise ValueError(f"ops.conv2d: x has {x.shape[1]} channels, w "
                         f"expects {w.shape[1]}")
    if min(x.shape) < 1 or min(w.shape) < 1:
        raise ValueError("ops.conv2d: every dimension must be >= 1")
    if b is not None and b.shape != (w.shape[0],):
        raise ValueError(f"ops.conv2d: b must have shape [{w.shape[0]}], "
                         f"got {tuple(b.shape)}")
    B, C, H, W = x.shape
    K, _, R, S = w.shape
    if R > H or S > W:
        raise ValueError(f"ops.conv2d: a {R}x{S} filter does not fit the "
                         f"{H}x{W} input")
    _require_same_device("conv2d", x, w=w, b=b)
    _require_fits_int("conv2d", **{"B": B, "C*H*W": C * H * W,
                                   "K*C*R*S": K * C * R * S,
                                   "K*OH*OW": K * (H - R + 1) * (W - S + 1)})
    return _Conv2d.apply(x.contiguous(), w.contiguous(),
                         None if b is None else b.contiguous())


# ---------------------------------------------------------------------------
# K3+K4 — fused 2x2 maxpool + ReLU (train_dist.py:65-66 applies
# relu(max_pool2d(.., 2))); backward routes grad to the argmax where the
# pooled max was positive.
# ---------------------------------------------------------------------------
class _MaxPool2dRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        if x.is_cuda:
            k = _k()
            B, C, H, W = x.shape
            OH, OW = H // 2, W // 2
            out = torch.empty(B, C, OH, OW, device=x.device, dtype=x.dtype)
            idx = torch.empty(B, C, OH, OW, device=x.device,
                              dtype=torch.int32)
            k.maxpool2d_relu_fwd(
                _aligned4(x).data_ptr(), out.data_ptr(), idx.data_ptr(),
                B, C, H, W, x.dtype == torch.bfloat16, _stream())
            ctx.save_for_backward(idx)
            ctx.in_shape = x.shape
            return out
        pooled, idx = F.max_pool2d(x, 2, return_indices=True)
        out = F.relu(pooled)
        ctx.save_for_backward(idx, pooled)
        ctx.in_shape = x.shape
        return out

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        if gy.is_cuda:
            (idx,) = ctx.saved_tensors
            k = _k()
            B, C, H, W = ctx.in_shape
            # the kernel writes every slot of every window; an odd last
            # row or column is in no window and gets no gradient
            alloc = torch.zeros if H % 2 or W % 2 else torch.empty
            gx = alloc(ctx.in_shape, device=gy.device, dtype=gy.dtype)
            k.maxpool2d_relu_bwd(
                gy.data_ptr(), idx.data_ptr(), gx.data_ptr(), B, C, H, W,
                gy.dtype == torch.bfloat16, _stream())
            return gx
        idx, pooled = ctx.saved_tensors
        gy = gy * (pooled > 0)
        return F.max_unpool2d(gy, idx, 2, output_size=ctx.in_shape[-2:])


def _aligned4(t):
    """The bf16 pool kernels move 2 elements per access."""
    return t if t.data_ptr() % 4 == 0 else t.clone()


def maxpool2d_relu(x):
    """``relu(max_pool2d(x, 2))`` on fp32 or bf16 tensors.  Max and ReLU
    only select values, so the bf16 result is the fp32 op's on the same
    values, bit for bit; the saved index encoding is shared.  The bf16
    GPU path requires even ``H`` and ``W``."""
    if x.is_cuda:
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"ops.maxpool2d_relu: fp32 or bf16 CUDA tensors "
                            f"only, got {x.dtype}")
        if x.dtype == torch.bfloat16:
            if x.dim() != 4:
                raise ValueError("ops.maxpool2d_relu: [B,C,H,W] expected")
            if x.shape[2] % 2 or x.shape[3] % 2 or min(x.shape[2:]) < 2:
                raise ValueError(
                    f"ops.maxpool2d_relu (bf16): H and W must be even, got "
                    f"{tuple(x.shape[2:])}")
    return _MaxPool2dRelu.apply(x.contiguous())


def relu(x):
    _require_fp32("relu", x=x)
    return _Relu.apply(x.contiguous())


class _Relu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        if x.is_cuda:
            k = _k()
            out = torch.empty_like(x)
            k.relu_fwd(x.data_ptr(), out.data_ptr(), x.numel(), _stream())
            ctx.save_for_backward(out)
            return out
        out = F.relu(x)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gy):
        (out,) = ctx.saved_tensors
        gy = gy.contiguous()
        if gy.is_cuda:
            k = _k()
            gx = torch.empty_like(gy)
            k.relu_bwd(gy.data_ptr(), out.data_ptr(), gx.data_ptr(),
                       gy.numel(), _stream())
            return gx
        return gy * (out > 0)


# ---------------------------------------------------------------------------
# K5/K6 — dropout2d (per-channel mask, train_dist.py:60,66) and
# elementwise dropout (train_dist.py:69), device-side philox-style RNG.
# ---------------------------------------------------------------------------
# per-device RNG seed counter living in DEVICE memory: the dropout
# kernels bump-and-read it on the stream, so masks advance correctly
# across hipGraph replays (host-side seeds would be frozen at capture).
_seed_bufs = {}


def _seed_ptr(device) -> int:
    key = device.index
    if key not in _seed_bufs:
        _seed_bufs[key] = torch.tensor([12345], dtype=torch.int64,
                                       device=device)
    return _seed_bufs[key].data_ptr()


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, training, channelwise):
        if not training or p == 0.0:
            ctx.mask = None
            return x
        scale = 1.0 / (1.0 - p)
        if x.is_cuda:
            k = _k()
            out = torch.empty_like(x)
            if channelwise:
                B, C = x.shape[0], x.shape[1]
                hw = x.numel() // (B * C)
                mask = torch.empty(B * C, device=x.device,
                                   dtype=torch.uint8)
                k.dropout2d_fwd(x.data_ptr(), out.data_ptr(),
                                mask.data_ptr(), B * C, hw, p,
                                _seed_ptr(x.device),
                                x.dtype == torch.bfloat16, _stream())
            else:
                mask = torch.empty(x.numel(), device=x.device,
                                   dtype=torch.uint8)
                k.dropout_fwd(x.data_ptr(), out.data_ptr(), mask.data_ptr(),
                              x.numel(), p, _seed_ptr(x.device),
                              x.dtype == torch.bfloat16, _stream())
            ctx.save_for_backward(mask)
            ctx.meta = (scale, channelwise, x.shape)
            ctx.mask = mask
            return out
        # CPU reference
        if channelwise:
            B, C = x.shape[0], x.shape[1]
            mask = (torch.rand(B, C, device=x.device) >= p).to(x.dtype)
            out = x * mask.view(B, C, *([1] * (x.dim() - 2))) * scale
        else:
            mask = (torch.rand_like(x) >= p).to(x.dtype)
            out = x * mask * scale
        ctx.save_for_backward(mask)
        ctx.meta = (scale, channelwise, x.shape)
        ctx.mask = mask
        return out

    @staticmethod
    def backward(ctx, gy):
        if ctx.mask is None:
            return gy, None, None, None
        (mask,) = ctx.saved_tensors
        scale, channelwise, shape = ctx.meta
        gy = gy.contiguous()
        if gy.is_cuda:
            k = _k()
            gx = torch.empty_like(gy)
            if channelwise:
                B, C = shape[0], shape[1]
                hw = gy.numel() // (B * C)
                k.dropout2d_bwd(gy.data_ptr(), mask.data_ptr(),
                                gx.data_ptr(), B * C, hw, scale,
                                gy.dtype == torch.bfloat16, _stream())
            else:
                k.dropout_bwd(gy.data_ptr(), mask.data_ptr(), gx.data_ptr(),
                              gy.numel(), scale,
                              gy.dtype == torch.bfloat16, _stream())
            return gx, None, None, None
        if channelwise:
            B, C = shape[0], shape[1]
            gx = gy * mask.view(B, C, *([1] * (gy.dim() - 2))) * scale
        else:
            gx = gy * mask * scale
        return gx, None, None, None


def dropout(x, p=0.5, training=True):
    """Elementwise dropout on fp32 or bf16 tensors.  The bf16 kernels hash
    the same element index with the same device-side seed as the fp32
    ones, so for equal seed and ``p`` the keep-mask is identical; kept
    values are ``bf16(float(x) * scale)``."""
    if x.is_cuda and x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(
            f"ops.dropout: fp32 or bf16 CUDA tensors only, got {x.dtype}")
    return _Dropout.apply(x.contiguous(), p, training, False)


def dropout2d(x, p=0.5, training=True):
    """Channel dropout on fp32 or bf16 tensors.  The bf16 kernels hash the
    same plane index with the same device-side seed as the fp32 ones, so
    for equal seed and ``p`` the channel mask is identical; kept values
    are ``bf16(float(x) * scale)``."""
    if x.is_cuda and x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(
            f"ops.dropout2d: fp32 or bf16 CUDA tensors only, got {x.dtype}")
    return _Dropout.apply(x.contiguous(), p, training, True)


# ---------------------------------------------------------------------------
# K7/K8 — linear with optional fused-ReLU epilogue (fc1 path is
# relu(fc1(x)), train_dist.py:68)
# ---------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, fuse_relu):
        if x.is_cuda:
            k = _k()
            B, K = x.shape
            N = w.shape[0]
            out = torch.empty(B, N, device=x.device, dtype=x.dtype)
            k.linear_fwd(x.data_ptr(), w.data_ptr(), _ptr(b),
                         out.data_ptr(), B, K, N, fuse_relu, _stream())
        else:
            out = F.linear(x, w, b)
            if fuse_relu:
                out = F.relu(out)
        ctx.save_for_backward(x, w, out)
        ctx.fuse_relu = fuse_relu
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, gy):
        x, w, out = ctx.saved_tensors
        gy = gy.contiguous()
        if x.is_cuda:
            k = _k()
            B, K = x.shape
            N = w.shape[0]
            # fully written by the kernels, in dense order
            gx = torch.empty(x.shape, device=x.device, dtype=x.dtype)
            gw = torch.empty(w.shape, device=x.device, dtype=x.dtype)
            gb = torch.empty(N, device=x.device, dtype=x.dtype) \
                if ctx.has_bias else None
            k.linear_bwd(x.data_ptr(), w.data_ptr(), gy.data_ptr(),
                         out.data_ptr() if ctx.fuse_relu else 0,
                         gx.data_ptr(), gw.data_ptr(), _ptr(gb),
                         B, K, N, _stream())
            return gx, gw, gb, None
        if ctx.fuse_relu:
            gy = gy * (out > 0)
        gx = gy @ w
        gw = gy.t() @ x
        gb = gy.sum(0) if ctx.has_bias else None
        return gx, gw, gb, None


def linear(x, w, b=None, fuse_relu=False):
    """``relu?(x @ w.T + b)``: ``x`` [B,K], ``w`` [N,K] and ``b`` [N] or
    None, fp32 on GPU, in any memory layout (the kernels read dense copies
    and return dense gradients)."""
    _require_tensors("linear", x=x, w=w, b=b)
    _require_fp32("linear", "; use ops.linear_bf16 for bf16 operands",
                  x=x, w=w, b=b)
    if x.dim() != 2 or w.dim() != 2:
        raise ValueError(f"ops.linear: x [B,K] and w [N,K] expected, got "
                         f"{tuple(x.shape)} and {tuple(w.shape)}")
    if x.shape[1] != w.shape[1]:
        raise ValueError(f"ops.linear: x has K = {x.shape[1]}, w expects "
                         f"{w.shape[1]}")
    if min(x.shape) < 1 or w.shape[0] < 1:
        raise ValueError("ops.linear: B, K and N must be >= 1")
    if b is not None and b.shape != (w.shape[0],):
        raise ValueError(f"ops.linear: b must have shape [{w.shape[0]}], "
                         f"got {tuple(b.shape)}")
    _require_same_device("linear", x, w=w, b=b)
    _require_fits_int("linear", **{"B": x.shape[0],
                                   "N*K": w.shape[0] * w.shape[1]})
    return _Linear.apply(x.contiguous(), w.contiguous(),
                         None if b is None else b.contiguous(),
                         bool(fuse_relu))


# ---------------------------------------------------------------------------
# K16 — mixed-precision linear: bf16 operands on the matrix cores, fp32
# accumulation, fp32 master weights and gradients (csrc/linear_bf16.hip).
# Contract, on GPU and CPU alike: every GEMM operand is bf16 (fp32 inputs
# are rounded RNE first), products are summed in fp32, and each result is
# rounded once to its output dtype.
# ---------------------------------------------------------------------------
def _to_bf16(t):
    """RNE cast to a contiguous bf16 tensor (identity for bf16 input)."""
    if t.dtype == torch.bfloat16:
        return t.contiguous()
    if t.dtype != torch.float32:
        raise TypeError(f"linear_bf16: fp32 or bf16 tensors only, "
                        f"got {t.dtype}")
    if not t.is_cuda:
        return t.contiguous().to(torch.bfloat16)
    t = t.contiguous()
    out = torch.empty(t.shape, device=t.device, dtype=torch.bfloat16)
    _k().cast_f32_to_bf16(t.data_ptr(), out.data_ptr(), t.numel(),
                          _stream())
    return out


class _LinearBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, fuse_relu, out_dtype):
        # the bf16 copies are saved, so each operand is cast once per step
        xb, wb = _to_bf16(x), _to_bf16(w)
        B, K = xb.shape
        N = wb.shape[0]
        if x.is_cuda:
            k = _k()
            out = torch.empty(B, N, device=x.device, dtype=out_dtype)
            k.linear_bf16_fwd(xb.data_ptr(), wb.data_ptr(), _ptr(b),
                              out.data_ptr(), B, K, N, fuse_relu,
                              out_dtype == torch.float32, _stream())
        else:
            acc = xb.float() @ wb.float().t()
            if b is not None:
                acc = acc + b
            if fuse_relu:
                acc = F.relu(acc)
            out = acc.to(out_dtype)
        ctx.save_for_backward(xb, wb, out if fuse_relu else None)
        ctx.x_dtype, ctx.w_dtype = x.dtype, w.dtype
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, gy):
        xb, wb, out = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        B, K = xb.shape
        N = wb.shape[0]
        gyb = _to_bf16(gy)
        gx = gw = gb = None
        if xb.is_cuda:
            k = _k()
            mask = _ptr(out)
            mask_f32 = out is not None and out.dtype == torch.float32
            if need_x:
                gx = torch.empty(B, K, device=xb.device, dtype=ctx.x_dtype)
                k.linear_bf16_bwd_x(gyb.data_ptr(), wb.data_ptr(), mask,
                                    mask_f32, gx.data_ptr(), B, K, N,
                                    ctx.x_dtype == torch.float32, _stream())
            if need_w or need_b:
                gw = torch.empty(N, K, device=xb.device,
                                 dtype=torch.float32)
                gb = torch.empty(N, device=xb.device, dtype=torch.float32) \
                    if need_b else None
                splits = k.linear_bf16_gw_splits(B, K, N)
                part = torch.empty(splits * (N * K + N), device=xb.device,
                                   dtype=torch.float32) \
                    if splits > 1 else None
                k.linear_bf16_bwd_w(
                    gyb.data_ptr(), xb.data_ptr(), mask, mask_f32,
                    gw.data_ptr(), _ptr(gb), _ptr(part), splits,
                    B, K, N, _stream())
                if ctx.w_dtype == torch.bfloat16:
                    gw = _to_bf16(gw)
                if not need_w:
                    gw = None
            return gx, gw, gb, None, None
        g = gyb.float()
        if out is not None:
            g = g * (out > 0)
        if need_x:
            gx = (g @ wb.float()).to(ctx.x_dtype)
        if need_w:
            gw = (g.t() @ xb.float()).to(ctx.w_dtype)
        if need_b:
            gb = g.sum(0)
        return gx, gw, gb, None, None


def linear_bf16(x, w, b=None, fuse_relu=False, out_dtype=torch.bfloat16):
    """``relu?(x @ w.T + b)`` with bf16 operands and fp32 accumulation.

    ``x`` [B,K] and ``w`` [N,K] are fp32 or bf16, ``b`` is fp32 or None;
    the result is [B,N] in ``out_dtype`` (bf16 or fp32).  Backward gives
    ``gx`` in ``x``'s dtype, ``gb`` in fp32, and ``gw`` in fp32 for an fp32
    (master) weight — so optimizers and gradient all-reduce see exactly
    the fp32 tensors they see on the fp32 path — or rounded once to bf16
    for a bf16 weight.  The weight gradient is bitwise reproducible."""
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"linear_bf16: out_dtype must be torch.bfloat16 or "
                        f"torch.float32, got {out_dtype}")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError(f"linear_bf16: x [B,K] and w [N,K] expected, got "
                         f"{tuple(x.shape)} and {tuple(w.shape)}")
    if min(x.shape[0], x.shape[1], w.shape[0]) < 1:
        raise ValueError("linear_bf16: B, K and N must be >= 1")
    for name, t in (("x", x), ("w", w)):
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"linear_bf16: {name} must be fp32 or bf16, "
                            f"got {t.dtype}")
    if b is not None:
        if b.dtype != torch.float32:
            raise TypeError(f"linear_bf16: b must be fp32, got {b.dtype}")
        if b.shape != (w.shape[0],):
            raise ValueError("linear_bf16: b must have shape [N]")
        b = b.contiguous()
    return _LinearBf16.apply(x, w, b, fuse_relu, out_dtype)


# ---------------------------------------------------------------------------
# K17 — mixed-precision convolution: the three products of a conv layer as
# implicit GEMMs on the bf16 matrix-core tile of linear_bf16, behind
# im2col loaders (csrc/conv_bf16.hip).  Same contract as linear_bf16, on
# GPU and CPU alike: bf16 operands (fp32 inputs are rounded RNE first),
# fp32 accumulation, one rounding per result; padding adds exact zeros.
# ---------------------------------------------------------------------------
_CONV_DIM_MAX = 2 ** 31 - 1 - 128   # the kernel's int GEMM dimensions


def _pair(v, name, low, op="conv2d_bf16"):
    if isinstance(v, bool):
        raise ValueError(f"{op}: {name} must be an int or a pair")
    if isinstance(v, int):
        v = (v, v)
    else:
        try:
            v = tuple(v)
        except TypeError:
            raise ValueError(
                f"{op}: {name} must be an int or a pair") from None
    if len(v) != 2 or not all(isinstance(e, int) and not isinstance(e, bool)
                              for e in v):
        raise ValueError(f"{op}: {name} must be an int or a pair of "
                         f"ints, got {v}")
    if min(v) < low:
        raise ValueError(f"{op}: {name} must be >= {low}, got {v}")
    return v


class _Conv2dBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, padding, out_dtype):
        xb, wb = _to_bf16(x), _to_bf16(w)
        B, C, H, W = xb.shape
        K, _, R, S = wb.shape
        (sh, sw), (ph, pw) = stride, padding
        OH = (H + 2 * ph - R) // sh + 1
        OW = (W + 2 * pw - S) // sw + 1
        if x.is_cuda:
            out = torch.empty(B, K, OH, OW, device=x.device, dtype=out_dtype)
            _k().conv2d_bf16_fwd(
                xb.data_ptr(), wb.data_ptr(), _ptr(b), out.data_ptr(),
                B, C, H, W, K, R, S, sh, sw, ph, pw,
                out_dtype == torch.float32, _stream())
        else:
            out = F.conv2d(xb.float(), wb.float(), b, stride,
                           padding).to(out_dtype)
        ctx.save_for_backward(xb, wb)
        ctx.geom = (stride, padding, OH, OW)
        ctx.x_dtype, ctx.w_dtype = x.dtype, w.dtype
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, gy):
        xb, wb = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        B, C, H, W = xb.shape
        K, _, R, S = wb.shape
        stride, padding, OH, OW = ctx.geom
        (sh, sw), (ph, pw) = stride, padding
        gyb = _to_bf16(gy)
        gx = gw = gb = None
        if xb.is_cuda:
            k = _k()
            dims = (B, C, H, W, K, R, S, sh, sw, ph, pw)
            if need_x:
                gx = torch.empty(B, C, H, W, device=xb.device,
                                 dtype=ctx.x_dtype)  # fully written
                k.conv2d_bf16_bwd_x(gyb.data_ptr(), wb.data_ptr(),
                                    gx.data_ptr(), *dims,
                                    ctx.x_dtype == torch.float32, _stream())
            if need_w or need_b:
                n_gw = K * C * R * S
                gw = torch.empty(K, C, R, S, device=xb.device,
                                 dtype=torch.float32)
                gb = torch.empty(K, device=xb.device, dtype=torch.float32) \
                    if need_b else None
                splits = k.conv2d_bf16_gw_splits(*dims)
                part = torch.empty(splits * (n_gw + K), device=xb.device,
                                   dtype=torch.float32) \
                    if splits > 1 else None
                k.conv2d_bf16_bwd_w(
                    gyb.data_ptr(), xb.data_ptr(), gw.data_ptr(), _ptr(gb),
                    _ptr(part), splits, *dims, _stream())
                if ctx.w_dtype == torch.bfloat16:
                    gw = _to_bf16(gw)
                if not need_w:
                    gw = None
            return gx, gw, gb, None, None, None
        g = gyb.float()
        if need_x:
            gx = torch.nn.grad.conv2d_input(
                xb.shape, wb.float(), g, stride, padding).to(ctx.x_dtype)
        if need_w:
            gw = torch.nn.grad.conv2d_weight(
                xb.float(), wb.shape, g, stride, padding).to(ctx.w_dtype)
        if need_b:
            gb = g.sum(dim=(0, 2, 3))
        return gx, gw, gb, None, None, None


def conv2d_bf16(x, w, b=None, stride=1, padding=0,
                out_dtype=torch.bfloat16):
    """2-D convolution (cross-correlation, NCHW) with bf16 operands and
    fp32 accumulation.

    ``x`` [B,C,H,W] and ``w`` [K,C,R,S] are fp32 or bf16, ``b`` is fp32 [K]
    or None; ``stride`` (>= 1) and zero ``padding`` (>= 0) are ints or
    (h, w) pairs.  The result is [B,K,OH,OW] in ``out_dtype`` (bf16 or
    fp32) with ``OH = (H + 2*ph - R)//sh + 1``.  No dilation, groups or
    fused activation.  Backward gives ``gx`` in ``x``'s dtype (exact zeros
    where no output reads the input), ``gb`` in fp32 and ``gw`` in fp32
    for an fp32 (master) weight, or rounded once to bf16 for a bf16
    weight; ``gw`` and ``gb`` are bitwise reproducible."""
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"conv2d_bf16: out_dtype must be torch.bfloat16 or "
                        f"torch.float32, got {out_dtype}")
    for name, t in (("x", x), ("w", w)):
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"conv2d_bf16: {name} must be fp32 or bf16, "
                            f"got {t.dtype}")
    if b is not None and b.dtype != torch.float32:
        raise TypeError(f"conv2d_bf16: b must be fp32, got {b.dtype}")
    if x.dim() != 4 or w.dim() != 4:
        raise ValueError(f"conv2d_bf16: x [B,C,H,W] and w [K,C,R,S] expected,"
                         f" got {tuple(x.shape)} and {tuple(w.shape)}")
    if x.shape[1] != w.shape[1]:
        raise ValueError(f"conv2d_bf16: x has {x.shape[1]} channels, w "
                         f"expects {w.shape[1]} (groups are not supported)")
    if min(x.shape) < 1 or min(w.shape) < 1:
        raise ValueError("conv2d_bf16: every dimension must be >= 1")
    if b is not None:
        if b.shape != (w.shape[0],):
            raise ValueError("conv2d_bf16: b must have shape [K]")
        b = b.contiguous()
    sh, sw = _pair(stride, "stride", 1)
    ph, pw = _pair(padding, "padding", 0)
    B, C, H, W = x.shape
    K, _, R, S = w.shape
    OH = (H + 2 * ph - R) // sh + 1
    OW = (W + 2 * pw - S) // sw + 1
    if H + 2 * ph < R or W + 2 * pw < S or OH < 1 or OW < 1:
        raise ValueError(
            f"conv2d_bf16: a {R}x{S} filter does not fit the padded "
            f"{H + 2 * ph}x{W + 2 * pw} input")
    for what, v in (("B*OH*OW", B * OH * OW), ("B*H*W", B * H * W),
                    ("C*R*S", C * R * S), ("K*R*S", K * R * S),
                    ("H+2*ph", H + 2 * ph), ("W+2*pw", W + 2 * pw)):
        if v > _CONV_DIM_MAX:
            raise ValueError(
                f"conv2d_bf16: {what} = {v} does not fit the kernel's "
                f"32-bit GEMM index")
    for what, v in (("x", B * C * H * W), ("w", K * C * R * S),
                    ("out", B * K * OH * OW)):
        if v >= 2 ** 62:
            raise ValueError(f"conv2d_bf16: {what} has too many elements")
    return _Conv2dBf16.apply(x, w, b, (sh, sw), (ph, pw), out_dtype)


# ---------------------------------------------------------------------------
# K18 — batch normalization over NCHW, fp32 or bf16 activations, with an
# optional residual add and ReLU fused into the same pass
# (csrc/batchnorm.hip).  Contract, on GPU and CPU alike: statistics and all
# arithmetic are fp32, the variance is the centred second moment (never
# E[x^2] - E[x]^2), each output element is rounded once to its dtype, and
# nothing uses float atomics, so every result is bitwise reproducible.
# ---------------------------------------------------------------------------
_BN_MAX_ELEMS = 2 ** 31 - 1   # the kernels' 32-bit access indices


def _bn_chan(t):
    return t.view(1, -1, 1, 1)


def _batchnorm2d_forward(x, weight, bias, running_mean, running_var,
                         training, momentum, eps, residual, fuse_relu):
    """The forward of ``batchnorm2d`` on checked, contiguous tensors.
    Returns ``(y, save_mean, save_invstd)``: the fp32 batch statistics the
    backward uses in training, ``(y, None, None)`` in eval."""
    B, C, H, W = x.shape
    if x.is_cuda:
        k = _k()
        y = torch.empty_like(x)
        mean = invstd = ws = None
        splits = 1
        if training:
            mean = torch.empty(C, device=x.device, dtype=torch.float32)
            invstd = torch.empty(C, device=x.device, dtype=torch.float32)
            splits = k.batchnorm2d_splits(B, C, H * W)
            ws = torch.empty(C * splits * 3, device=x.device,
                             dtype=torch.float32)
        k.batchnorm2d_fwd(
            x.data_ptr(), _ptr(residual), y.data_ptr(), weight.data_ptr(),
            bias.data_ptr(), _ptr(running_mean), _ptr(running_var),
            _ptr(mean), _ptr(invstd), _ptr(ws), splits, B, C, H * W,
            training, momentum, eps, fuse_relu, x.dtype == torch.bfloat16,
            _stream())
        return y, mean, invstd
    xf = x.float()
    if training:
        n = B * H * W
        mean = xf.mean(dim=(0, 2, 3))
        d = xf - _bn_chan(mean)
        var = (d * d).mean(dim=(0, 2, 3))
        invstd = 1.0 / torch.sqrt(var + eps)
        if running_mean is not None:
            running_mean.mul_(1.0 - momentum).add_(mean, alpha=momentum)
            running_var.mul_(1.0 - momentum).add_(var * (n / (n - 1.0)),
                                                  alpha=momentum)
        mu, inv = mean, invstd
    else:
        mean = invstd = None
        mu, inv = running_mean, 1.0 / torch.sqrt(running_var + eps)
    yf = (xf - _bn_chan(mu)) * _bn_chan(weight * inv) + _bn_chan(bias)
    if residual is not None:
        yf = yf + residual.float()
    if fuse_relu:
        yf = F.relu(yf)
    return yf.to(x.dtype), mean, invstd


class _BatchNorm2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var,
                training, momentum, eps, fuse_relu):
        y, mean, invstd = _batchnorm2d_forward(
            x, weight, bias, running_mean, running_var, training, momentum,
            eps, residual, fuse_relu)
        if training:
            ctx.save_for_backward(x, weight, mean, invstd,
                                  y if fuse_relu else None)
        else:
            ctx.save_for_backward(x, weight, running_mean, running_var,
                                  y if fuse_relu else None)
        ctx.training, ctx.eps = training, eps
        ctx.has_residual = residual is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, mean, stat, y = ctx.saved_tensors
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        need_r = need_r and ctx.has_residual
        B, C, H, W = x.shape
        n = B * H * W
        gy = gy.contiguous()
        gx = gres = None
        if x.is_cuda:
            k = _k()
            gw = torch.empty(C, device=x.device, dtype=torch.float32)
            gb = torch.empty(C, device=x.device, dtype=torch.float32)
            if need_x:
                gx = torch.empty_like(x)     # fully written
            if need_r:
                gres = torch.empty_like(x)
            splits = k.batchnorm2d_splits(B, C, H * W)
            ws = torch.empty(C * splits * 2, device=x.device,
                             dtype=torch.float32)
            k.batchnorm2d_bwd(
                x.data_ptr(), gy.data_ptr(), _ptr(y), weight.data_ptr(),
                mean.data_ptr(), stat.data_ptr(), gw.data_ptr(),
                gb.data_ptr(), _ptr(gx), _ptr(gres), ws.data_ptr(), splits,
                B, C, H * W, ctx.training, ctx.eps,
                x.dtype == torch.bfloat16, _stream())
        else:
            inv = stat if ctx.training else 1.0 / torch.sqrt(stat + ctx.eps)
            g = gy.float()
            if y is not None:
                g = g * (y > 0)
            xhat = (x.float() - _bn_chan(mean)) * _bn_chan(inv)
            gb = g.sum(dim=(0, 2, 3))
            gw = (g * xhat).sum(dim=(0, 2, 3))
            if need_x:
                if ctx.training:
                    t = g - _bn_chan(gb / n) - xhat * _bn_chan(gw / n)
                else:
                    t = g
                gx = (_bn_chan(weight * inv) * t).to(x.dtype)
            if need_r:
                gres = g.to(x.dtype)
        return (gx, gw if need_w else None, gb if need_b else None, gres,
                None, None, None, None, None, None)


def batchnorm2d(x, weight, bias, running_mean=None, running_var=None,
                training=True, momentum=0.1, eps=1e-5, residual=None,
                fuse_relu=False):
    """``relu?(batch_norm(x) + residual?)`` over NCHW in one pass.

    ``x`` [B,C,H,W] is fp32 or bf16 and the result has its dtype and shape;
    ``residual``, when given, has both too.  ``weight``, ``bias`` and the
    running buffers are fp32 [C].  ``training=True`` normalizes with the
    batch statistics (biased variance) and, when running buffers are
    given, updates them in place on the stream —
    ``rm = (1-m)*rm + m*mean``, ``rv = (1-m)*rv + m*var*n/(n-1)`` — so the
    update survives graph replay; ``training=False`` normalizes with the
    running buffers and leaves them alone.  ``momentum=None`` (torch's
    cumulative average) is not supported.  Backward gives ``gx`` in ``x``'s
    dtype, the residual's gradient in its dtype (the gradient after the
    ReLU mask, exactly) and fp32 ``gweight``/``gbias``.  Statistics and
    arithmetic are fp32 with a centred variance and one rounding per
    element; every output is bitwise reproducible."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"ops.batchnorm2d: x must be fp32 or bf16, got "
                        f"{x.dtype}")
    if x.dim() != 4:
        raise ValueError(f"ops.batchnorm2d: x [B,C,H,W] expected, got "
                         f"{tuple(x.shape)}")
    if min(x.shape) < 1:
        raise ValueError("ops.batchnorm2d: every dimension must be >= 1")
    B, C, H, W = x.shape
    if x.numel() > _BN_MAX_ELEMS:
        raise ValueError(f"ops.batchnorm2d: {x.numel()} elements do not fit "
                         f"the kernel's 32-bit index")
    named = [("weight", weight), ("bias", bias)]
    if (running_mean is None) != (running_var is None):
        raise ValueError("ops.batchnorm2d: running_mean and running_var "
                         "must both be given or both be None")
    if running_mean is not None:
        named += [("running_mean", running_mean),
                  ("running_var", running_var)]
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"ops.batchnorm2d: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"ops.batchnorm2d: {name} must be fp32, got "
                            f"{t.dtype}")
        if t.shape != (C,):
            raise ValueError(f"ops.batchnorm2d: {name} must have shape "
                             f"[{C}], got {tuple(t.shape)}")
        if t.device != x.device:
            raise ValueError(f"ops.batchnorm2d: {name} is on {t.device}, x "
                             f"on {x.device}")
    if running_mean is not None and not (running_mean.is_contiguous()
                                         and running_var.is_contiguous()):
        raise ValueError("ops.batchnorm2d: the running buffers are updated "
                         "in place and must be contiguous")
    if residual is not None:
        if residual.dtype != x.dtype:
            raise TypeError(f"ops.batchnorm2d: residual must have x's dtype "
                            f"{x.dtype}, got {residual.dtype}")
        if residual.shape != x.shape:
            raise ValueError(f"ops.batchnorm2d: residual must have x's "
                             f"shape {tuple(x.shape)}, got "
                             f"{tuple(residual.shape)}")
        if residual.device != x.device:
            raise ValueError("ops.batchnorm2d: residual is on another "
                             "device than x")
        residual = residual.contiguous()
    if momentum is None:
        raise ValueError("ops.batchnorm2d: momentum=None (cumulative moving "
                         "average) is not supported; pass a float in [0, 1]")
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) \
            or not 0.0 <= momentum <= 1.0:
        raise ValueError(f"ops.batchnorm2d: momentum must be a float in "
                         f"[0, 1], got {momentum!r}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) \
            or not eps >= 0.0:
        raise ValueError(f"ops.batchnorm2d: eps must be a float >= 0, got "
                         f"{eps!r}")
    if training and B * H * W == 1:
        raise ValueError(f"ops.batchnorm2d: training needs more than one "
                         f"value per channel, got input size "
                         f"{tuple(x.shape)}")
    if not training and running_mean is None:
        raise ValueError("ops.batchnorm2d: training=False needs "
                         "running_mean and running_var")
    return _BatchNorm2d.apply(
        x.contiguous(), weight.contiguous(), bias.contiguous(), residual,
        running_mean, running_var, bool(training), float(momentum),
        float(eps), bool(fuse_relu))


# ---------------------------------------------------------------------------
# K19 — general max-pool over NCHW (kernel, stride, padding; windows may
# overlap), fp32 or bf16 (csrc/pool.hip).  Contract, on GPU and CPU alike:
# padding is -inf and never selected, the first maximum of a window wins a
# tie, NaN propagates, the output carries the selected element's bits; the
# backward sums, per input element and in fp32, the gradients of the windows
# that selected it and rounds once.  No atomics: bitwise reproducible.
# ---------------------------------------------------------------------------
_POOL_MAX_PLANE = 2 ** 29     # the kernels' 32-bit in-plane indices
_POOL_DTYPES = (torch.float32, torch.bfloat16)


def _check_pool_input(op, x):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"ops.{op}: x must be a tensor")
    if x.dtype not in _POOL_DTYPES:
        raise TypeError(f"ops.{op}: x must be fp32 or bf16, got {x.dtype}")
    if x.dim() != 4:
        raise ValueError(f"ops.{op}: x [B,C,H,W] expected, got "
                         f"{tuple(x.shape)}")
    if min(x.shape) < 1:
        raise ValueError(f"ops.{op}: every dimension must be >= 1, got "
                         f"{tuple(x.shape)}")
    if x.shape[2] * x.shape[3] > _POOL_MAX_PLANE:
        raise ValueError(f"ops.{op}: H*W = {x.shape[2] * x.shape[3]} does "
                         f"not fit the kernel's 32-bit plane index")


class _MaxPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        B, C, H, W = x.shape
        (kh, kw), (sh, sw), (ph, pw) = kernel, stride, padding
        ctx.geom = (B, C, H, W, kh, kw, sh, sw, ph, pw)
        if x.is_cuda:
            OH = (H + 2 * ph - kh) // sh + 1
            OW = (W + 2 * pw - kw) // sw + 1
            y = torch.empty(B, C, OH, OW, device=x.device, dtype=x.dtype)
            slot = torch.empty(B, C, OH, OW, device=x.device,
                               dtype=torch.uint8)
            _k().maxpool2d_fwd(x.data_ptr(), y.data_ptr(), slot.data_ptr(),
                               *ctx.geom, x.dtype == torch.bfloat16,
                               _stream())
            ctx.save_for_backward(slot)
            return y
        y, idx = F.max_pool2d(x, kernel, stride, padding,
                              return_indices=True)
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, gy):
        (saved,) = ctx.saved_tensors
        B, C, H, W = ctx.geom[:4]
        gy = gy.contiguous()
        if gy.is_cuda:
            gx = torch.empty(B, C, H, W, device=gy.device,
                             dtype=gy.dtype)      # fully written
            _k().maxpool2d_bwd(gy.data_ptr(), saved.data_ptr(),
                               gx.data_ptr(), *ctx.geom,
                               gy.dtype == torch.bfloat16, _stream())
            return gx, None, None, None
        gx = torch.zeros(B * C, H * W, dtype=torch.float32)
        gx.scatter_add_(1, saved.reshape(B * C, -1),
                        gy.float().reshape(B * C, -1))
        return gx.to(gy.dtype).view(B, C, H, W), None, None, None


def maxpool2d(x, kernel_size, stride=None, padding=0):
    """``max_pool2d(x, kernel_size, stride, padding)`` over NCHW.

    ``x`` [B,C,H,W] is fp32 or bf16 and the result [B,C,OH,OW] has its
    dtype, with ``OH = (H + 2*ph - kh)//sh + 1``.  ``kernel_size`` (>= 1),
    ``stride`` (>= 1, ``None`` means ``kernel_size``) and ``padding``
    (>= 0, at most half the kernel, torch's rule) are ints or (h, w) pairs;
    ``kh*kw`` is at most 256 and windows may overlap.  No dilation,
    ``ceil_mode`` or ``return_indices``.  Padding counts as -inf and is
    never selected; the first maximum of a window (row-major) wins a tie,
    a window of all -inf selects its first element and NaN propagates, as
    in torch.  Max only selects, so the output carries the selected
    element's bits and the bf16 result is the fp32 op's on the same values.
    Backward gives ``gx`` in ``x``'s dtype: per input element the fp32 sum,
    in a fixed order, of the gradients of the windows that selected it,
    rounded once, and exact zeros elsewhere.  No atomics are used, so the
    gradient of overlapping windows is bitwise reproducible."""
    op = "ops.maxpool2d"
    _check_pool_input("maxpool2d", x)
    kh, kw = _pair(kernel_size, "kernel_size", 1, op)
    sh, sw = (kh, kw) if stride is None else _pair(stride, "stride", 1, op)
    ph, pw = _pair(padding, "padding", 0, op)
    if ph > kh // 2 or pw > kw // 2:
        raise ValueError(f"{op}: padding must be at most half the kernel "
                         f"size, got padding {(ph, pw)} for kernel "
                         f"{(kh, kw)}")
    if kh * kw > 256:
        raise ValueError(f"{op}: kernel_size {(kh, kw)} has more than 256 "
                         f"positions")
    H, W = x.shape[2:]
    if H + 2 * ph < kh or W + 2 * pw < kw:
        raise ValueError(f"{op}: a {kh}x{kw} window does not fit the padded "
                         f"{H + 2 * ph}x{W + 2 * pw} input")
    if max(sh, sw) > _POOL_MAX_PLANE:
        raise ValueError(f"{op}: stride {(sh, sw)} does not fit the "
                         f"kernel's 32-bit index")
    return _MaxPool2d.apply(x.contiguous(), (kh, kw), (sh, sw), (ph, pw))


# ---------------------------------------------------------------------------
# K20 — global average pool [B,C,H,W] -> [B,C], fp32 or bf16
# (csrc/pool.hip).  Contract, on GPU and CPU alike: each plane is summed in
# fp32, divided once by H*W and rounded once to the output dtype.  The GPU
# sum has a fixed order that depends on H*W alone, so it is bitwise
# reproducible and independent of the pointer's alignment and of the dtype.
# ---------------------------------------------------------------------------
class _GlobalAvgPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        ctx.in_shape = (B, C, H, W)
        if x.is_cuda:
            y = torch.empty(B, C, device=x.device, dtype=x.dtype)
            _k().global_avgpool2d_fwd(x.data_ptr(), y.data_ptr(), B * C,
                                      H * W, x.dtype == torch.bfloat16,
                                      _stream())
            return y
        return (x.float().sum(dim=(2, 3)) / (H * W)).to(x.dtype)

    @staticmethod
    def backward(ctx, gy):
        B, C, H, W = ctx.in_shape
        gy = gy.contiguous()
        if gy.is_cuda:
            gx = torch.empty(B, C, H, W, device=gy.device,
                             dtype=gy.dtype)      # fully written
            _k().global_avgpool2d_bwd(gy.data_ptr(), gx.data_ptr(), B * C,
                                      H * W, gy.dtype == torch.bfloat16,
                                      _stream())
            return gx
        g = (gy.float() / (H * W)).to(gy.dtype)
        return g.view(B, C, 1, 1).expand(B, C, H, W).contiguous()


def global_avgpool2d(x):
    """The mean of every plane: ``adaptive_avg_pool2d(x, 1).flatten(1)``.

    ``x`` [B,C,H,W] is fp32 or bf16; the result is [B,C] in its dtype.
    Each plane is summed in fp32, divided once by ``H*W`` and rounded once.
    On the GPU the order of the sum is fixed by ``H*W`` alone: the result is
    bitwise reproducible, a view at any element offset gives the bits of
    its aligned copy, and the bf16 result is the fp32 op's on the same
    values, rounded once.  Backward gives ``gx[b,c,:,:] = gy[b,c] / (H*W)``
    in ``x``'s dtype, computed in fp32 and rounded once."""
    _check_pool_input("global_avgpool2d", x)
    return _GlobalAvgPool2d.apply(x.contiguous())


# ---------------------------------------------------------------------------
# K9+K10 — log_softmax over dim 1 (train_dist.py:71) and NLL loss
# (train_dist.py:120), plus the fused form used by the trainer.
# ---------------------------------------------------------------------------
class _LogSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        if x.is_cuda:
            k = _k()
            B, N = x.shape
            out = torch.empty_like(x)
            k.log_softmax_fwd(x.data_ptr(), out.data_ptr(), B, N, _stream())
        else:
            out = F.log_softmax(x, dim=1)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, gy):
        (out,) = ctx.saved_tensors
        gy = gy.contiguous()
        if out.is_cuda:
            k = _k()
            B, N = out.shape
            gx = torch.empty_like(out)
            k.log_softmax_bwd(gy.data_ptr(), out.data_ptr(), gx.data_ptr(),
                              B, N, _stream())
            return gx
        return gy - out.exp() * gy.sum(dim=1, keepdim=True)


def log_softmax(x):
    """``log_softmax(x, dim=1)`` of ``x`` [B,N], fp32 on GPU."""
    _require_tensors("log_softmax", x=x)
    _require_fp32("log_softmax", x=x)
    _check_rows("log_softmax", "x", x)
    return _LogSoftmax.apply(x.contiguous())


class _NllLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, target):
        ctx.save_for_backward(logp, target)
        if logp.is_cuda:
            k = _k()
            B, N = logp.shape
            loss = torch.empty((), device=logp.device, dtype=logp.dtype)
            k.nll_loss_fwd(logp.data_ptr(), target.data_ptr(),
                           loss.data_ptr(), B, N, _stream())
            return loss
        return F.nll_loss(logp, target)

    @staticmethod
    def backward(ctx, gloss):
        logp, target = ctx.saved_tensors
        if logp.is_cuda:
            k = _k()
            B, N = logp.shape
            gx = torch.zeros_like(logp)
            gl = gloss.contiguous()
            k.nll_loss_bwd(target.data_ptr(), gx.data_ptr(),
                           gl.data_ptr(), B, N, _stream())
            return gx, None
        B, N = logp.shape
        gx = torch.zeros_like(logp)
        gx[torch.arange(B), target] = -gloss / B
        return gx, None


def nll_loss(logp, target):
    """Mean of ``-logp[b, target[b]]`` over ``logp`` [B,N] (fp32 on GPU)
    and an int64 ``target`` [B].  A target value outside ``[0, N)`` is not
    checked: reading it would synchronize with the device, which a
    captured graph forbids."""
    _require_tensors("nll_loss", logp=logp)
    _require_fp32("nll_loss", logp=logp)
    _check_rows("nll_loss", "logp", logp)
    _check_target("nll_loss", logp, target)
    return _NllLoss.apply(logp.contiguous(), target.contiguous())


class _LogSoftmaxNll(torch.autograd.Function):
    """Fused K9+K10: one kernel computes log_softmax and the mean NLL;
    backward is the closed form softmax(x) - onehot, scaled."""

    @staticmethod
    def forward(ctx, logits, target):
        if logits.is_cuda:
            k = _k()
            B, N = logits.shape
            logp = torch.empty_like(logits)
            loss = torch.empty((), device=logits.device, dtype=logits.dtype)
            k.log_softmax_nll_fwd(logits.data_ptr(), target.data_ptr(),
                                  logp.data_ptr(), loss.data_ptr(),
                                  B, N, _stream())
        else:
            logp = F.log_softmax(logits, dim=1)
            loss = F.nll_loss(logp, target)
        ctx.save_for_backward(logp, target)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        logp, target = ctx.saved_tensors
        B, N = logp.shape
        if logp.is_cuda:
            k = _k()
            gx = torch.empty_like(logp)
            gl = gloss.contiguous()
            k.log_softmax_nll_bwd(logp.data_ptr(), target.data_ptr(),
                                  gx.data_ptr(), gl.data_ptr(), B, N,
                                  _stream())
            return gx, None
        gx = logp.exp()
        gx[torch.arange(B), target] -= 1.0
        return gx * (gloss / B), None


def log_softmax_nll(logits, target):
    """``nll_loss(log_softmax(logits), target)`` in one kernel, for
    ``logits`` [B,N] (fp32 on GPU) and an int64 ``target`` [B].  A target
    value outside ``[0, N)`` is not checked: reading it would synchronize
    with the device, which a captured graph forbids."""
    _require_tensors("log_softmax_nll", logits=logits)
    _require_fp32("log_softmax_nll", logits=logits)
    _check_rows("log_softmax_nll", "logits", logits)
    _check_target("log_softmax_nll", logits, target)
    return _LogSoftmaxNll.apply(logits.contiguous(), target.contiguous())


# ---------------------------------------------------------------------------
# K21 — cross-entropy over [B,N] logits, fp32 or bf16, for rows of any
# width (csrc/cross_entropy.hip).  Contract, on GPU and CPU alike: all
# arithmetic is fp32 and the loss is fp32 whatever the logits' dtype.  With
# eps = label_smoothing and t = target[b],
#     row[b]  = lse[b] - (1-eps)*x[b,t] - (eps/N)*sum_i x[b,i]
#     gx[b,i] = (exp(x[b,i] - lse[b]) - q[b,i]) * g,
#               q = (1-eps)*onehot + eps/N
# where the smoothing term is left out for eps == 0 (a -inf logit then gives
# p = 0 and a finite loss).  A row with t == ignore_index contributes 0 and
# its gx row is stored zeros; "mean" divides by the number of rows not
# ignored, taken on the device (0 rows give NaN, as in torch).  g is the
# upstream gradient, divided by that count for "mean".  The forward saves
# lse [B] and the count, never a [B,N] tensor; the backward recomputes the
# softmax from the logits and rounds gx once to their dtype.  No float
# atomics: every result is bitwise reproducible.
# ---------------------------------------------------------------------------
_XENT_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def _cross_entropy_cpu_forward(xf, target, eps, ignore_index):
    """Row losses, lse and the keep mask of the contract, in plain fp32
    torch.  The target is only compared with the column index."""
    B, N = xf.shape
    m = xf.max(dim=1, keepdim=True).values
    lse = (m + torch.log(torch.exp(xf - m).sum(dim=1, keepdim=True)))[:, 0]
    keep = target != ignore_index
    onehot = torch.arange(N)[None, :] == target[:, None]
    x_t = torch.where(onehot, xf, torch.zeros_like(xf)).sum(dim=1)
    row = lse - (1.0 - eps) * x_t
    if eps != 0.0:
        row = row - (eps / N) * xf.sum(dim=1)
    zero = torch.zeros_like(row)
    return torch.where(keep, row, zero), torch.where(keep, lse, zero), keep


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, eps, ignore_index, reduction):
        B, N = logits.shape
        red = _XENT_REDUCTIONS[reduction]
        ctx.meta = (eps, ignore_index, red)
        f32 = dict(device=logits.device, dtype=torch.float32)
        if logits.is_cuda:
            row = torch.empty(B, **f32)
            lse = torch.empty(B, **f32)
            loss = count = None
            if red:
                loss = torch.empty((), **f32)
                count = torch.empty(1, **f32)
            _k().cross_entropy_fwd(
                logits.data_ptr(), target.data_ptr(), row.data_ptr(),
                lse.data_ptr(), _ptr(loss), _ptr(count), B, N, eps,
                ignore_index, red, logits.dtype == torch.bfloat16, 0,
                _stream())
            ctx.save_for_backward(logits, target, lse, count)
            return loss if red else row
        row, lse, keep = _cross_entropy_cpu_forward(
            logits.float(), target, eps, ignore_index)
        count = keep.sum().to(torch.float32).reshape(1)
        ctx.save_for_backward(logits, target, lse, count)
        if red == 0:
            return row
        return row.sum() / count[0] if red == 1 else row.sum()

    @staticmethod
    def backward(ctx, gloss):
        logits, target, lse, count = ctx.saved_tensors
        eps, ignore_index, red = ctx.meta
        B, N = logits.shape
        gl = gloss.contiguous().float()
        if logits.is_cuda:
            gx = torch.empty_like(logits)       # fully written
            _k().cross_entropy_bwd(
                logits.data_ptr(), target.data_ptr(), lse.data_ptr(),
                _ptr(count), gl.data_ptr(), gx.data_ptr(), B, N, eps,
                ignore_index, red, logits.dtype == torch.bfloat16, 0,
                _stream())
            return gx, None, None, None, None
        xf = logits.float()
        keep = (target != ignore_index)[:, None]
        onehot = torch.arange(N)[None, :] == target[:, None]
        en = torch.tensor(eps, dtype=torch.float32) / N
        q = torch.where(onehot, (1.0 - eps) + en, en)
        if red == 0:
            g = gl[:, None]
        else:
            g = gl / count[0] if red == 1 else gl
        gx = (torch.exp(xf - lse[:, None]) - q) * g
        # stored zeros, never 0 * g
        gx = torch.where(keep, gx, torch.zeros_like(gx))
        return gx.to(logits.dtype), None, None, None, None


def cross_entropy(logits, target, *, label_smoothing=0.0, ignore_index=-100,
                  reduction="mean"):
    """Cross-entropy of ``logits`` [B,N] (fp32 or bf16) against an int64
    ``target`` [B] of class indices, for rows of any width.

    The result is fp32 whatever the logits' dtype: a scalar for
    ``reduction`` ``"mean"`` or ``"sum"``, [B] for ``"none"``.  With
    ``eps = label_smoothing`` in [0, 1] the row loss is
    ``lse - (1-eps)*x[t] - (eps/N)*sum(x)``; a row whose target equals
    ``ignore_index`` contributes 0 and gets an all-zero gradient row, and
    ``"mean"`` divides by the number of rows not ignored (NaN when there
    are none, as in torch).  That count is taken on the device, so the op
    can be captured in a graph.  Backward gives ``gx`` in the logits'
    dtype, ``(softmax(x) - q) * g`` with ``q = (1-eps)*onehot + eps/N``,
    computed in fp32 from the saved log-sum-exp and rounded once; nothing
    of size [B,N] is saved.  No atomics: loss and gradient are bitwise
    reproducible, do not depend on the pointer's alignment, and the bf16
    row losses are those of the fp32 op on the same values.

    Not supported: class weights, probability (soft) targets and logits of
    more than two dimensions.  A target value outside ``[0, N)`` that is
    not ``ignore_index`` is not checked, because reading it would
    synchronize with the device; the GPU kernels only compare it with the
    column index, so it gives a meaningless loss but no out-of-bounds
    access."""
    op = "cross_entropy"
    _require_tensors(op, logits=logits)
    if logits.is_cuda and logits.dtype not in (torch.float32,
                                               torch.bfloat16):
        raise TypeError(f"ops.{op}: fp32 or bf16 logits only on GPU, got "
                        f"{logits.dtype}")
    if not logits.is_floating_point():
        raise TypeError(f"ops.{op}: logits must be floating point, got "
                        f"{logits.dtype}")
    _check_rows(op, "logits", logits)
    _check_target(op, logits, target)
    if isinstance(label_smoothing, bool) \
            or not isinstance(label_smoothing, (int, float)) \
            or not 0.0 <= label_smoothing <= 1.0:
        raise ValueError(f"ops.{op}: label_smoothing must be a real number "
                         f"in [0, 1], got {label_smoothing!r}")
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
        raise TypeError(f"ops.{op}: ignore_index must be an int, got "
                        f"{ignore_index!r}")
    if not -2 ** 63 <= ignore_index < 2 ** 63:
        raise ValueError(f"ops.{op}: ignore_index does not fit int64")
    if reduction not in _XENT_REDUCTIONS:
        raise ValueError(f"ops.{op}: reduction must be 'none', 'mean' or "
                         f"'sum', got {reduction!r}")
    return _CrossEntropy.apply(logits.contiguous(), target.contiguous(),
                               float(label_smoothing), ignore_index,
                               reduction)
