"""Training-path ops.

Every op the reference's ``Net.forward`` + SGD step trigger implicitly
through torch (train_dist.py:58-71,110,118-124) is a hand-written CDNA4
HIP kernel here, with forward *and* backward (``csrc/kernels.hip``; K3-K6
in ``csrc/pointwise.hip``, K16-K23 in the files named at their sections):

  K1/K2  conv2d (direct, LDS-tiled)        -> conv2d
  K3+K4  maxpool2d(k2) fused with ReLU     -> maxpool2d_relu (fp32, bf16)
  K4     ReLU                              -> relu
  K5/K6  dropout2d (channel) / dropout     -> dropout2d / dropout
                                              (fp32, bf16)
  K7/K8  linear (+fused ReLU epilogue)     -> linear
  K16    bf16 MFMA linear, fp32 accumulate  -> linear_bf16
  K22    fp8 (e4m3/e5m2) 128-deep MFMA linear -> linear_fp8, quantize_fp8
  K23    MXFP8: e8m0 scales per 32 elements, applied by the scaled MFMA
                                    -> linear_fp8(scaling="mx"),
                                       quantize_fp8(block=32)
  K17    bf16 MFMA conv2d (stride, padding) -> conv2d_bf16
         the same on channels-last storage  -> conv2d_bf16(memory_format=
                                              torch.channels_last)
  K18    batchnorm2d (+residual add, +ReLU) -> batchnorm2d (fp32, bf16)
  K19    maxpool2d (kernel, stride, padding) -> maxpool2d (fp32, bf16)
  K20    global average pool [B,C,H,W]->[B,C] -> global_avgpool2d
                                              (fp32, bf16)
         K18-K20 on channels-last storage   -> the same three with
                                              memory_format=
                                              torch.channels_last
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
# K22 — fp8 linear on the 128-deep fp8 matrix instruction
# (csrc/linear_fp8.hip).  Contract, on GPU and CPU alike: per-tensor,
# current, power-of-two scaling; x and w quantised to e4m3, the incoming
# gradient to e5m2, each RNE from the exactly scaled value; exact products
# summed in fp32; the sum multiplied by the exact inverse scales, bias added
# in fp32, ReLU, one rounding to the output dtype.
# ---------------------------------------------------------------------------
_FP8_E = {torch.float8_e4m3fn: 8, torch.float8_e5m2: 15}   # FMAX = 1.75 * 2^E


def _fp8_quantize_cpu(t, dtype):
    """``quantize_fp8``'s rule with torch ops: the executable statement of
    the contract.  Returns ``(q, s)`` with ``s`` a 0-dim fp32 tensor."""
    amax = t.detach().abs().max().float()
    m, ex = torch.frexp(amax)            # amax = m * 2^ex, m in [0.5, 1)
    # amax = f * 2^e with f = 2m in [1, 2), e = ex - 1
    k = _FP8_E[dtype] - (ex - 1) - (m > 0.875).to(ex.dtype)
    k = torch.where(amax == 0, torch.zeros_like(k), k.clamp(-126, 126))
    s = torch.ldexp(torch.ones((), dtype=torch.float32), k)
    return (t.detach().float() * s).to(dtype), s


def _fp8_quantize_gpu(t, dtype, mask=None, want_q=True, want_qT=False,
                      want_gb=False):
    """Quantise the dense 2-D CUDA tensor ``t`` (fp32 or bf16), zeroed where
    ``mask <= 0``.  Returns ``(q, qT, ws, gb)``: the padded row-major and
    transposed uint8 storages (None where not wanted), the fp32 workspace
    whose first two elements are ``s`` and ``1/s``, and the fp32 column sums
    of the masked ``t``."""
    k = _k()
    R, C = t.shape
    dev = t.device
    q = torch.empty(R, k.fp8_pitch(C), device=dev, dtype=torch.uint8) \
        if want_q else None
    qT = torch.empty(C, k.fp8_pitch(R), device=dev, dtype=torch.uint8) \
        if want_qT else None
    ws = torch.empty(k.fp8_ws_floats(), device=dev, dtype=torch.float32)
    gb = gb_part = None
    if want_gb:
        gb = torch.empty(C, device=dev, dtype=torch.float32)
        gb_part = torch.empty(k.fp8_pitch(R) // 64 * C, device=dev,
                              dtype=torch.float32)
    k.fp8_quantize(t.data_ptr(), t.dtype == torch.bfloat16, _ptr(mask),
                   mask is not None and mask.dtype == torch.float32, R, C,
                   dtype == torch.float8_e5m2, _ptr(q), _ptr(qT),
                   ws.data_ptr(), _ptr(gb_part), _ptr(gb), _stream())
    return q, qT, ws, gb


def _mxfp8_quantize_cpu(t, dtype):
    """``quantize_fp8(block=32)``'s rule with torch ops: the executable
    statement of the MX contract.  Returns ``(q, scales)``: ``t``'s shape in
    ``dtype`` and the uint8 e8m0 bytes ``127 - k`` per 32-block of the last
    dimension."""
    C = t.shape[-1]
    nb = -(-C // 32)
    blocks = F.pad(t.detach().float(), (0, nb * 32 - C)).reshape(
        t.shape[:-1] + (nb, 32))
    amax = blocks.abs().amax(-1)
    m, ex = torch.frexp(amax)            # amax = m * 2^ex, m in [0.5, 1)
    k = _FP8_E[dtype] - (ex - 1) - (m > 0.875).to(ex.dtype)
    k = torch.where(amax == 0, torch.zeros_like(k), k.clamp(-126, 126))
    s = torch.ldexp(torch.ones((), dtype=torch.float32), k)
    q = (blocks * s.unsqueeze(-1)).to(dtype).reshape(
        t.shape[:-1] + (nb * 32,))[..., :C]
    return q, (127 - k).to(torch.uint8)


def _mxfp8_dequantize(q, scales):
    """fp32 ``q * 2^(scales - 127)`` per 32-block of the last dimension
    (exact: a power-of-two multiple of an fp8 value)."""
    f = torch.ldexp(torch.ones((), dtype=torch.float32),
                    scales.to(torch.int32) - 127)
    return q.float() * f.repeat_interleave(32, -1)[..., :q.shape[-1]]


def _mxfp8_quantize_gpu(t, dtype, mask=None, want_q=True, want_qT=False,
                        want_gb=False):
    """One launch of K23's quantiser on the dense 2-D CUDA tensor ``t``,
    zeroed where ``mask <= 0``.  Returns ``(q, sq, qT, sqT, gb)``: the padded
    uint8 storage blocked along columns with its e8m0 scales, the transposed
    storage blocked along rows with its scales (None where not wanted), and
    the fp32 column sums of the masked ``t``."""
    k = _k()
    R, C = t.shape
    dev = t.device
    q = sq = qT = sqT = gb = gb_part = None
    if want_q:
        q = torch.empty(R, k.fp8_pitch(C), device=dev, dtype=torch.uint8)
        sq = torch.empty(R, k.fp8_pitch(C) // 32, device=dev,
                         dtype=torch.uint8)
    if want_qT:
        qT = torch.empty(C, k.fp8_pitch(R), device=dev, dtype=torch.uint8)
        sqT = torch.empty(C, k.fp8_pitch(R) // 32, device=dev,
                          dtype=torch.uint8)
    if want_gb:
        gb = torch.empty(C, device=dev, dtype=torch.float32)
        gb_part = torch.empty(k.fp8_pitch(R) // 64 * C, device=dev,
                              dtype=torch.float32)
    k.mxfp8_quantize(t.data_ptr(), t.dtype == torch.bfloat16, _ptr(mask),
                     mask is not None and mask.dtype == torch.float32, R, C,
                     dtype == torch.float8_e5m2, _ptr(q), _ptr(sq), _ptr(qT),
                     _ptr(sqT), _ptr(gb_part), _ptr(gb), _stream())
    return q, sq, qT, sqT, gb


def quantize_fp8(t, dtype, block=None):
    """Quantise ``t`` (fp32 or bf16, at least 1-D, no empty dimension) to
    ``dtype`` (``torch.float8_e4m3fn`` or ``torch.float8_e5m2``) with one
    power-of-two scale for the whole tensor.  Returns ``(q, scale)``.

    ``block=32`` (K23, MXFP8) scales every 32 consecutive elements of the
    last dimension on their own, the last block of a row completed with
    zeros, by the rule below applied to the block's amax.  It returns
    ``(q, scales)`` with ``scales`` the uint8 e8m0 bytes ``127 - k`` of the
    decode factors ``2^-k``, shape ``t.shape[:-1] + (ceil(C/32),)``, always
    in [1, 253]; an all-zero block has 127.  On GPU both are views of the
    kernel's padded storage.  Any other ``block`` raises ``ValueError``.

    With ``amax = max|t| = f * 2^e``, ``f`` in [1, 2), the scale is
    ``2^k``, ``k = E - e`` for ``f <= 1.75`` and ``E - 1 - e`` otherwise
    (``E`` = 8 for e4m3, 15 for e5m2): the largest power of two with
    ``amax * scale <= FMAX``.  ``k`` is clamped to [-126, 126] and is 0 for
    ``amax == 0``; non-finite input is outside the contract.  ``q`` is
    ``RNE(t * scale)``, bit for bit torch's CPU cast of that product; it has
    ``t``'s shape and, on GPU, is a view of the kernel's storage, whose rows
    are zero-padded to a multiple of 128 bytes.  ``scale`` is a 0-dim fp32
    tensor on ``t``'s device; nothing is read back to the host."""
    if dtype not in _FP8_E:
        raise TypeError(f"quantize_fp8: dtype must be torch.float8_e4m3fn or "
                        f"torch.float8_e5m2, got {dtype}")
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32,
                                                          torch.bfloat16):
        raise TypeError("quantize_fp8: t must be an fp32 or bf16 tensor")
    if t.dim() < 1 or min(t.shape) < 1:
        raise ValueError(f"quantize_fp8: t must have at least one dimension "
                         f"and none empty, got {tuple(t.shape)}")
    if block not in (None, 32):
        raise ValueError(f"quantize_fp8: block must be None or 32, "
                         f"got {block!r}")
    if not t.is_cuda:
        return _mxfp8_quantize_cpu(t, dtype) if block \
            else _fp8_quantize_cpu(t, dtype)
    C = t.shape[-1]
    t2 = t.detach().contiguous().view(-1, C)
    if block:
        q, sq, _, _, _ = _mxfp8_quantize_gpu(t2, dtype)
        return (q[:, :C].view(dtype).reshape(t.shape),
                sq[:, :-(-C // 32)].reshape(t.shape[:-1] + (-(-C // 32),)))
    q, _, ws, _ = _fp8_quantize_gpu(t2, dtype)
    return q[:, :C].view(dtype).reshape(t.shape), ws[0]


class _LinearFp8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, fuse_relu, out_dtype):
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        B, K = x.shape
        N = w.shape[0]
        e4m3 = torch.float8_e4m3fn
        if x.is_cuda:
            k = _k()
            # each operand is quantised once per step: the transposed copies
            # the backward needs come out of the same pass
            xq, xqT, sx, _ = _fp8_quantize_gpu(
                x.detach().contiguous(), e4m3, want_qT=need_w)
            wq, wqT, sw, _ = _fp8_quantize_gpu(
                w.detach().contiguous(), e4m3, want_qT=need_x)
            out = torch.empty(B, N, device=x.device, dtype=out_dtype)
            k.linear_fp8_fwd(xq.data_ptr(), wq.data_ptr(), sx.data_ptr(),
                             sw.data_ptr(), _ptr(b), out.data_ptr(), B, K, N,
                             fuse_relu, out_dtype == torch.float32,
                             _stream())
            ctx.save_for_backward(xqT, wqT, sx, sw,
                                  out if fuse_relu else None)
        else:
            xq, sx = _fp8_quantize_cpu(x.detach(), e4m3)
            wq, sw = _fp8_quantize_cpu(w.detach(), e4m3)
            acc = (xq.float() @ wq.float().t()) * (1.0 / sx) * (1.0 / sw)
            if b is not None:
                acc = acc + b
            if fuse_relu:
                acc = F.relu(acc)
            out = acc.to(out_dtype)
            ctx.save_for_backward(xq, wq, sx, sw, out if fuse_relu else None)
        ctx.dims = (B, K, N)
        ctx.x_dtype, ctx.w_dtype = x.dtype, w.dtype
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, gy):
        xs, ws_, sx, sw, out = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        B, K, N = ctx.dims
        e5m2 = torch.float8_e5m2
        gx = gw = gb = None
        if gy.is_cuda:
            k = _k()
            dev = gy.device
            gq, gqT, sg, gb = _fp8_quantize_gpu(
                gy.contiguous(), e5m2, mask=out, want_q=need_x,
                want_qT=need_w or not need_x, want_gb=need_b)
            if need_x:
                gx = torch.empty(B, K, device=dev, dtype=ctx.x_dtype)
                k.linear_fp8_bwd_x(gq.data_ptr(), ws_.data_ptr(),
                                   sg.data_ptr(), sw.data_ptr(),
                                   gx.data_ptr(), B, K, N,
                                   ctx.x_dtype == torch.float32, _stream())
            if need_w:
                gw = torch.empty(N, K, device=dev, dtype=torch.float32)
                splits = k.linear_fp8_gw_splits(B, K, N)
                part = torch.empty(splits * N * K, device=dev,
                                   dtype=torch.float32) \
                    if splits > 1 else None
                k.linear_fp8_bwd_w(gqT.data_ptr(), xs.data_ptr(),
                                   sg.data_ptr(), sx.data_ptr(),
                                   gw.data_ptr(), _ptr(part), splits,
                                   B, K, N, _stream())
                if ctx.w_dtype == torch.bfloat16:
                    gw = _to_bf16(gw)
            return gx, gw, gb, None, None
        g = gy.float()
        if out is not None:
            g = torch.where(out > 0, g, torch.zeros_like(g))
        gq, sg = _fp8_quantize_cpu(g, e5m2)
        if need_x:
            gx = ((gq.float() @ ws_.float()) * (1.0 / sg)
                  * (1.0 / sw)).to(ctx.x_dtype)
        if need_w:
            gw = ((gq.float().t() @ xs.float()) * (1.0 / sg)
                  * (1.0 / sx)).to(ctx.w_dtype)
        if need_b:
            gb = g.sum(0)
        return gx, gw, gb, None, None


# ---------------------------------------------------------------------------
# K23 — MXFP8: the same three products with one e8m0 scale per 32 elements
# along each product's reduction axis, applied by the matrix instruction
# (csrc/linear_fp8.hip).  Forward blocks x and w along K, gx blocks gy and w
# along N, gw blocks gy and x along B, so a transposed copy is quantised on
# its own.  No per-tensor scale is left: the fp32 accumulator is the result.
# ---------------------------------------------------------------------------
class _LinearMxFp8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, fuse_relu, out_dtype):
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        B, K = x.shape
        N = w.shape[0]
        e4m3 = torch.float8_e4m3fn
        if x.is_cuda:
            k = _k()
            # one launch per operand: the copy the backward needs, blocked
            # along the other axis, comes out of the same tile
            xq, sx, xqT, sxT, _ = _mxfp8_quantize_gpu(
                x.detach().contiguous(), e4m3, want_qT=need_w)
            wq, sw, wqT, swT, _ = _mxfp8_quantize_gpu(
                w.detach().contiguous(), e4m3, want_qT=need_x)
            out = torch.empty(B, N, device=x.device, dtype=out_dtype)
            k.linear_mxfp8_fwd(xq.data_ptr(), wq.data_ptr(), sx.data_ptr(),
                               sw.data_ptr(), _ptr(b), out.data_ptr(), B, K,
                               N, fuse_relu, out_dtype == torch.float32,
                               _stream())
            ctx.save_for_backward(xqT, sxT, wqT, swT,
                                  out if fuse_relu else None)
        else:
            xd, wd = x.detach(), w.detach()
            acc = _mxfp8_dequantize(*_mxfp8_quantize_cpu(xd, e4m3)) \
                @ _mxfp8_dequantize(*_mxfp8_quantize_cpu(wd, e4m3)).t()
            if b is not None:
                acc = acc + b
            if fuse_relu:
                acc = F.relu(acc)
            out = acc.to(out_dtype)
            # dequantised [K,B] and [K,N] copies, blocked along B and N
            xT = _mxfp8_dequantize(*_mxfp8_quantize_cpu(xd.t(), e4m3)) \
                if need_w else None
            wT = _mxfp8_dequantize(*_mxfp8_quantize_cpu(wd.t(), e4m3)) \
                if need_x else None
            ctx.save_for_backward(xT, None, wT, None,
                                  out if fuse_relu else None)
        ctx.dims = (B, K, N)
        ctx.x_dtype, ctx.w_dtype = x.dtype, w.dtype
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, gy):
        xT, sxT, wT, swT, out = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        B, K, N = ctx.dims
        e5m2 = torch.float8_e5m2
        gx = gw = gb = None
        if gy.is_cuda:
            k = _k()
            dev = gy.device
            gq, sg, gqT, sgT, gb = _mxfp8_quantize_gpu(
                gy.contiguous(), e5m2, mask=out, want_q=need_x,
                want_qT=need_w or not need_x, want_gb=need_b)
            if need_x:
                gx = torch.empty(B, K, device=dev, dtype=ctx.x_dtype)
                k.linear_mxfp8_bwd_x(gq.data_ptr(), wT.data_ptr(),
                                     sg.data_ptr(), swT.data_ptr(),
                                     gx.data_ptr(), B, K, N,
                                     ctx.x_dtype == torch.float32, _stream())
            if need_w:
                gw = torch.empty(N, K, device=dev, dtype=torch.float32)
                splits = k.linear_fp8_gw_splits(B, K, N)
                part = torch.empty(splits * N * K, device=dev,
                                   dtype=torch.float32) \
                    if splits > 1 else None
                k.linear_mxfp8_bwd_w(gqT.data_ptr(), xT.data_ptr(),
                                     sgT.data_ptr(), sxT.data_ptr(),
                                     gw.data_ptr(), _ptr(part), splits,
                                     B, K, N, _stream())
                if ctx.w_dtype == torch.bfloat16:
                    gw = _to_bf16(gw)
            return gx, gw, gb, None, None
        g = gy.float()
        if out is not None:
            g = torch.where(out > 0, g, torch.zeros_like(g))
        if need_x:
            gd = _mxfp8_dequantize(*_mxfp8_quantize_cpu(g, e5m2))
            gx = (gd @ wT.t()).to(ctx.x_dtype)
        if need_w:
            gdT = _mxfp8_dequantize(*_mxfp8_quantize_cpu(g.t(), e5m2))
            gw = (gdT @ xT.t()).to(ctx.w_dtype)
        if need_b:
            gb = g.sum(0)
        return gx, gw, gb, None, None


def linear_fp8(x, w, b=None, fuse_relu=False, out_dtype=torch.bfloat16,
               scaling="tensor"):
    """``relu?(x @ w.T + b)`` with fp8 operands and fp32 accumulation.

    ``x`` [B,K] and ``w`` [N,K] are fp32 or bf16, ``b`` is fp32 or None;
    the result is [B,N] in ``out_dtype`` (bf16 or fp32).  ``x`` and ``w``
    are quantised to e4m3 and, in backward, the incoming gradient to e5m2,
    each with its own power-of-two scale of the current tensor
    (``quantize_fp8``'s rule; scales stay on the device).  Products are
    exact in fp32 and are summed in fp32; the sum is multiplied by the exact
    inverse scales, the bias added, ReLU applied, and the result rounded
    once.  With ``fuse_relu`` the gradient is zeroed where ``out <= 0``
    before it is quantised, so its scale is the masked gradient's.  On the
    GPU the sum is the matrix instruction's, which drops a product 2^-14 or
    more below the largest one it is first added to
    (profiles/linear_fp8_numbers.md); it is deterministic all the same.

    Backward gives ``gx`` in ``x``'s dtype, ``gw`` in fp32 for an fp32
    (master) weight or rounded once to bf16 for a bf16 weight, and ``gb``
    in fp32 — the column sum of the masked, *unquantised* gradient.  ``gw``
    and ``gb`` are bitwise reproducible.  CPU tensors run the same contract
    with torch's float8 casts and an fp32 matmul.

    ``scaling="mx"`` (K23, MXFP8) gives every 32 consecutive elements along
    a product's reduction axis their own power-of-two scale
    (``quantize_fp8(block=32)``'s rule): forward blocks ``x`` and ``w`` along
    K, ``gx`` blocks the gradient and ``w`` along N, ``gw`` blocks the
    gradient and ``x`` along B, so each operand is quantised once per axis
    it is reduced over, in one launch with no amax pass.  The matrix
    instruction applies the two e8m0 block scales to each block's products;
    the fp32 accumulator is the result, bias, ReLU and the one rounding
    follow as above, and ``gw`` and ``gb`` stay bitwise reproducible.  On
    CPU the operands are dequantised per block and multiplied in fp32."""
    if scaling not in ("tensor", "mx"):
        raise ValueError(f"linear_fp8: scaling must be 'tensor' or 'mx', "
                         f"got {scaling!r}")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"linear_fp8: out_dtype must be torch.bfloat16 or "
                        f"torch.float32, got {out_dtype}")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError(f"linear_fp8: x [B,K] and w [N,K] expected, got "
                         f"{tuple(x.shape)} and {tuple(w.shape)}")
    if min(x.shape[0], x.shape[1], w.shape[0]) < 1:
        raise ValueError("linear_fp8: B, K and N must be >= 1")
    for name, t in (("x", x), ("w", w)):
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"linear_fp8: {name} must be fp32 or bf16, "
                            f"got {t.dtype}")
    if w.device != x.device:
        raise ValueError(f"linear_fp8: w is on {w.device}, x on {x.device}")
    if b is not None:
        if b.dtype != torch.float32:
            raise TypeError(f"linear_fp8: b must be fp32, got {b.dtype}")
        if b.shape != (w.shape[0],):
            raise ValueError("linear_fp8: b must have shape [N]")
        b = b.contiguous()
    fn = _LinearMxFp8 if scaling == "mx" else _LinearFp8
    return fn.apply(x, w, b, bool(fuse_relu), out_dtype)


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


def _as_nhwc(t):
    """``t`` [B,C,H,W] with dense channels-last storage (no copy where it
    has that already)."""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _to_bf16_nhwc(t):
    """RNE cast to a bf16 tensor with dense channels-last storage.  The cast
    kernel is elementwise, so it rounds the storage in whatever order it
    lies."""
    t = _as_nhwc(t)
    if t.dtype == torch.bfloat16:
        return t
    if not t.is_cuda:
        return t.to(torch.bfloat16)
    out = torch.empty_like(t, dtype=torch.bfloat16)
    _k().cast_f32_to_bf16(t.data_ptr(), out.data_ptr(), t.numel(),
                          _stream())
    return out


def _empty_nhwc(B, C, H, W, like, dtype):
    return torch.empty(B, H, W, C, device=like.device,
                       dtype=dtype).permute(0, 3, 1, 2)


def _is_nhwc(op, memory_format):
    """True for ``torch.channels_last``, False for
    ``torch.contiguous_format``; the layout is named, never guessed from
    strides, so anything else is an error."""
    if memory_format not in (torch.contiguous_format, torch.channels_last):
        raise ValueError(f"{op}: memory_format must be "
                         f"torch.contiguous_format or torch.channels_last, "
                         f"got {memory_format}")
    return memory_format == torch.channels_last


def _laid_out(t, nhwc):
    """``t`` in the storage the kernels of the chosen layout read.  CPU
    tensors always run the default path's arithmetic, on NCHW storage."""
    if t is None:
        return None
    return _as_nhwc(t) if nhwc and t.is_cuda else t.contiguous()


class ConvBatchStats:
    """What ``conv2d_bf16(..., bn_stats=True)`` hands to
    ``batchnorm2d(..., batch_stats=...)``: the per-channel partial
    statistics of the convolution's output ``out`` and what identifies that
    tensor.  Opaque: only those two functions read it.

    ``partials`` is fp32 [tiles, K, 2] — the mean and the centred second
    moment of ``out``'s rows (pixels) [64t, min(rows, 64t + 64)) — or None
    for a CPU tensor, whose batch norm computes its own statistics."""

    __slots__ = ("partials", "rows", "K", "data_ptr", "shape", "is_cpu")

    def __init__(self, partials, out):
        B, K, OH, OW = out.shape
        self.partials = partials
        self.rows, self.K = B * OH * OW, K
        self.data_ptr, self.shape = out.data_ptr(), tuple(out.shape)
        self.is_cpu = not out.is_cuda


class _Conv2dNhwcBf16(torch.autograd.Function):
    """conv2d_bf16 on channels-last storage (csrc/conv_nhwc_bf16.hip): the
    logical shapes are _Conv2dBf16's, activations lie [B][H][W][C].  With
    ``bn_stats`` on a GPU tensor the forward runs the kernel with the
    statistics epilogue and returns ``(out, partials)``."""

    @staticmethod
    def forward(ctx, x, w, b, stride, padding, out_dtype, bn_stats):
        B, C, H, W = x.shape
        K, _, R, S = w.shape
        (sh, sw), (ph, pw) = stride, padding
        OH = (H + 2 * ph - R) // sh + 1
        OW = (W + 2 * pw - S) // sw + 1
        ctx.x_dtype, ctx.w_dtype = x.dtype, w.dtype
        if x.is_cuda:
            k = _k()
            xb, w = _to_bf16_nhwc(x), w.contiguous()
            # [K][R][S][C], rounded to bf16 on the way
            wp = torch.empty(K, R, S, C, device=x.device,
                             dtype=torch.bfloat16)
            k.conv2d_nhwc_bf16_pack_w(w.data_ptr(), wp.data_ptr(), K, C, R, S,
                                      w.dtype == torch.float32, False,
                                      _stream())
            out = _empty_nhwc(B, K, OH, OW, x, out_dtype)
            dims = (B, C, H, W, K, R, S, sh, sw, ph, pw)
            if bn_stats:
                tiles = k.conv2d_nhwc_bf16_stats_tiles(B * OH * OW)
                tws = torch.empty(tiles, K, 2, device=x.device,
                                  dtype=torch.float32)   # fully written
                k.conv2d_nhwc_bf16_fwd_stats(
                    xb.data_ptr(), wp.data_ptr(), _ptr(b), out.data_ptr(),
                    tws.data_ptr(), *dims, out_dtype == torch.float32,
                    _stream())
            else:
                k.conv2d_nhwc_bf16_fwd(
                    xb.data_ptr(), wp.data_ptr(), _ptr(b), out.data_ptr(),
                    *dims, out_dtype == torch.float32, _stream())
        else:
            # the default path's arithmetic, so the values are its bits
            xb, w = _to_bf16(x), _to_bf16(w)
            out = _as_nhwc(F.conv2d(xb.float(), w.float(), b, stride,
                                    padding).to(out_dtype))
        # on GPU the master weight: backward packs it again, for gx
        ctx.save_for_backward(xb, w)
        ctx.geom = (stride, padding, OH, OW)
        ctx.has_bias = b is not None
        if bn_stats and x.is_cuda:
            ctx.mark_non_differentiable(tws)
            return out, tws
        return out

    @staticmethod
    def backward(ctx, gy, _g_partials=None):
        xb, w = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        B, C, H, W = xb.shape
        K, _, R, S = w.shape
        stride, padding, OH, OW = ctx.geom
        (sh, sw), (ph, pw) = stride, padding
        gx = gw = gb = None
        if xb.is_cuda:
            k = _k()
            gyb = _to_bf16_nhwc(gy)
            dims = (B, C, H, W, K, R, S, sh, sw, ph, pw)
            if need_x:
                wp = torch.empty(C, R, S, K, device=xb.device,
                                 dtype=torch.bfloat16)
                k.conv2d_nhwc_bf16_pack_w(w.data_ptr(), wp.data_ptr(), K, C,
                                          R, S, w.dtype == torch.float32,
                                          True, _stream())
                gx = _empty_nhwc(B, C, H, W, xb, ctx.x_dtype)  # fully written
                k.conv2d_nhwc_bf16_bwd_x(
                    gyb.data_ptr(), wp.data_ptr(), gx.data_ptr(), *dims,
                    ctx.x_dtype == torch.float32, _stream())
            if need_w or need_b:
                n_gw = K * C * R * S
                gw = torch.empty(K, C, R, S, device=xb.device,
                                 dtype=torch.float32)
                gb = torch.empty(K, device=xb.device, dtype=torch.float32) \
                    if need_b else None
                # gb is the row sum of the gw GEMM's gy tile, so a bias that
                # alone needs a gradient still runs that GEMM and drops gw
                # (as the NCHW path does); no layer here trains only a bias
                splits = k.conv2d_nhwc_bf16_gw_splits(*dims)
                part = torch.empty(splits * (n_gw + K), device=xb.device,
                                   dtype=torch.float32) \
                    if splits > 1 else None
                k.conv2d_nhwc_bf16_bwd_w(
                    gyb.data_ptr(), xb.data_ptr(), gw.data_ptr(), _ptr(gb),
                    _ptr(part), splits, *dims, _stream())
                if ctx.w_dtype == torch.bfloat16:
                    gw = _to_bf16(gw)
                if not need_w:
                    gw = None
            return gx, gw, gb, None, None, None, None
        g = _to_bf16(gy).float()
        if need_x:
            gx = _as_nhwc(torch.nn.grad.conv2d_input(
                xb.shape, w.float(), g, stride, padding).to(ctx.x_dtype))
        if need_w:
            gw = torch.nn.grad.conv2d_weight(
                xb.float(), w.shape, g, stride, padding).to(ctx.w_dtype)
        if need_b:
            gb = g.sum(dim=(0, 2, 3))
        return gx, gw, gb, None, None, None, None


def conv2d_bf16(x, w, b=None, stride=1, padding=0,
                out_dtype=torch.bfloat16,
                memory_format=torch.contiguous_format, bn_stats=False):
    """2-D convolution (cross-correlation, NCHW) with bf16 operands and
    fp32 accumulation.

    ``x`` [B,C,H,W] and ``w`` [K,C,R,S] are fp32 or bf16, ``b`` is fp32 [K]
    or None; ``stride`` (>= 1) and zero ``padding`` (>= 0) are ints or
    (h, w) pairs.  The result is [B,K,OH,OW] in ``out_dtype`` (bf16 or
    fp32) with ``OH = (H + 2*ph - R)//sh + 1``.  No dilation, groups or
    fused activation.  Backward gives ``gx`` in ``x``'s dtype (exact zeros
    where no output reads the input), ``gb`` in fp32 and ``gw`` in fp32
    for an fp32 (master) weight, or rounded once to bf16 for a bf16
    weight; ``gw`` and ``gb`` are bitwise reproducible.

    ``memory_format=torch.channels_last`` runs the same contract on
    channels-last storage (K17's kernels in csrc/conv_nhwc_bf16.hip): ``x``
    and, in backward, ``gy`` keep their logical [B,C,H,W] shape and are
    brought to [B][H][W][C] storage, which costs nothing where they have it;
    the result and ``gx`` come back with that storage, ``gw`` dense
    [K,C,R,S].  The layout is never taken from ``x``'s strides: any other
    value than these two raises ``ValueError``.

    ``bn_stats=True`` (channels-last only, else ``ValueError``) is for a
    convolution whose output goes to a training batch norm.  The call
    returns ``(out, stats)``: ``out`` and the gradients are bit for bit
    those of the plain call, and ``stats`` (a ``ConvBatchStats``, not
    differentiable) holds per-channel partial means and centred second
    moments of ``out`` as stored — after its one rounding, bias included —
    which the forward kernel reduced from its own output tiles.
    ``batchnorm2d(out, ..., batch_stats=stats)`` starts from them instead
    of reading ``out`` twice.  For CPU tensors ``stats`` is empty."""
    nhwc = _is_nhwc("conv2d_bf16", memory_format)
    if bn_stats and not nhwc:
        raise ValueError("conv2d_bf16: bn_stats=True needs "
                         "memory_format=torch.channels_last")
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
    if nhwc:
        res = _Conv2dNhwcBf16.apply(x, w, b, (sh, sw), (ph, pw), out_dtype,
                                    bool(bn_stats))
        if not bn_stats:
            return res
        out, partials = res if x.is_cuda else (res, None)
        return out, ConvBatchStats(partials, out)
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
                         training, momentum, eps, residual, fuse_relu,
                         memory_format=torch.contiguous_format,
                         batch_stats=None):
    """The forward of ``batchnorm2d`` on checked tensors, contiguous or,
    with ``memory_format=torch.channels_last``, brought to channels-last
    storage here.  ``batch_stats`` (checked too) with partials replaces the
    statistics pass by a merge of those.  Returns ``(y, save_mean, save_invstd)``: the fp32 batch
    statistics the backward uses in training, ``(y, None, None)`` in
    eval."""
    nhwc = _is_nhwc("ops.batchnorm2d", memory_format)
    B, C, H, W = x.shape
    if x.is_cuda:
        k = _k()
        mean = invstd = ws = None
        splits = 1
        if nhwc:
            x, residual = _as_nhwc(x), _laid_out(residual, True)
            y = _empty_nhwc(B, C, H, W, x, x.dtype)
            get_splits, dims = k.batchnorm2d_nhwc_splits, (B * H * W, C)
            fwd = k.batchnorm2d_nhwc_fwd
        else:
            y = torch.empty_like(x)
            get_splits, dims = k.batchnorm2d_splits, (B, C, H * W)
            fwd = k.batchnorm2d_fwd
        if training:
            mean = torch.empty(C, device=x.device, dtype=torch.float32)
            invstd = torch.empty(C, device=x.device, dtype=torch.float32)
        if batch_stats is not None and batch_stats.partials is not None:
            n_ws = k.batchnorm2d_nhwc_merge_ws(*dims)
            ws = torch.empty(n_ws, device=x.device, dtype=torch.float32) \
                if n_ws else None
            k.batchnorm2d_nhwc_fwd_from_partials(
                x.data_ptr(), _ptr(residual), y.data_ptr(),
                weight.data_ptr(), bias.data_ptr(), _ptr(running_mean),
                _ptr(running_var), mean.data_ptr(), invstd.data_ptr(),
                batch_stats.partials.data_ptr(), _ptr(ws), *dims, momentum,
                eps, fuse_relu, x.dtype == torch.bfloat16, _stream())
            return y, mean, invstd
        if training:
            splits = get_splits(*dims)
            ws = torch.empty(C * splits * 3, device=x.device,
                             dtype=torch.float32)
        fwd(x.data_ptr(), _ptr(residual), y.data_ptr(), weight.data_ptr(),
            bias.data_ptr(), _ptr(running_mean), _ptr(running_var),
            _ptr(mean), _ptr(invstd), _ptr(ws), splits, *dims,
            training, momentum, eps, fuse_relu, x.dtype == torch.bfloat16,
            _stream())
        return y, mean, invstd
    if nhwc:
        # the default path's arithmetic, so the values are its bits
        y, mean, invstd = _batchnorm2d_forward(
            x.contiguous(), weight, bias, running_mean, running_var,
            training, momentum, eps, _laid_out(residual, False), fuse_relu)
        return _as_nhwc(y), mean, invstd
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
                training, momentum, eps, fuse_relu, memory_format,
                batch_stats):
        y, mean, invstd = _batchnorm2d_forward(
            x, weight, bias, running_mean, running_var, training, momentum,
            eps, residual, fuse_relu, memory_format, batch_stats)
        ctx.nhwc = memory_format == torch.channels_last
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
        gy = _laid_out(gy, ctx.nhwc)
        gx = gres = None
        if x.is_cuda:
            k = _k()
            gw = torch.empty(C, device=x.device, dtype=torch.float32)
            gb = torch.empty(C, device=x.device, dtype=torch.float32)
            # x is the tensor the forward read: empty_like keeps its layout
            if need_x:
                gx = torch.empty_like(x)     # fully written
            if need_r:
                gres = torch.empty_like(x)
            if ctx.nhwc:
                get_splits, dims = k.batchnorm2d_nhwc_splits, (B * H * W, C)
                bwd = k.batchnorm2d_nhwc_bwd
            else:
                get_splits, dims = k.batchnorm2d_splits, (B, C, H * W)
                bwd = k.batchnorm2d_bwd
            splits = get_splits(*dims)
            ws = torch.empty(C * splits * 2, device=x.device,
                             dtype=torch.float32)
            bwd(x.data_ptr(), gy.data_ptr(), _ptr(y), weight.data_ptr(),
                mean.data_ptr(), stat.data_ptr(), gw.data_ptr(),
                gb.data_ptr(), _ptr(gx), _ptr(gres), ws.data_ptr(), splits,
                *dims, ctx.training, ctx.eps,
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
            if ctx.nhwc:
                gx = _as_nhwc(gx) if need_x else None
                gres = _as_nhwc(gres) if need_r else None
        return (gx, gw if need_w else None, gb if need_b else None, gres,
                None, None, None, None, None, None, None, None)


def batchnorm2d(x, weight, bias, running_mean=None, running_var=None,
                training=True, momentum=0.1, eps=1e-5, residual=None,
                fuse_relu=False, memory_format=torch.contiguous_format,
                batch_stats=None):
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
    element; every output is bitwise reproducible.

    ``memory_format=torch.channels_last`` runs the same contract on
    channels-last storage (csrc/batchnorm_nhwc.hip), with
    ``conv2d_bf16``'s rules: ``x``, ``residual`` and, in backward, ``gy``
    keep their logical [B,C,H,W] shape and are brought to [B][H][W][C]
    storage, which costs nothing where they have it; ``y``, ``gx`` and the
    residual's gradient come back with that storage.  The layout is never
    taken from ``x``'s strides: any other value raises ``ValueError``.

    ``batch_stats`` is the second result of
    ``conv2d_bf16(..., bn_stats=True)`` and ``x`` that call's first.  The
    batch statistics are then merged from the convolution's per-tile
    partials (Chan's formula, fixed order) instead of computed in two
    passes over ``x``; they are statistics of the same stored values, so
    the contract above holds unchanged, and the backward is the same.
    ``ValueError`` unless ``training`` is true, the layout channels-last
    and ``x`` the tensor (shape and data pointer) the statistics were made
    for.  On CPU the (empty) ``batch_stats`` is checked and ignored."""
    nhwc = _is_nhwc("ops.batchnorm2d", memory_format)
    if batch_stats is not None:
        if not isinstance(batch_stats, ConvBatchStats):
            raise TypeError("ops.batchnorm2d: batch_stats must come from "
                            "conv2d_bf16(..., bn_stats=True)")
        if not training:
            raise ValueError("ops.batchnorm2d: batch_stats is for "
                             "training=True; eval uses the running buffers")
        if not nhwc:
            raise ValueError("ops.batchnorm2d: batch_stats needs "
                             "memory_format=torch.channels_last")
        if not isinstance(x, torch.Tensor) \
                or tuple(x.shape) != batch_stats.shape \
                or x.data_ptr() != batch_stats.data_ptr \
                or x.is_cuda == batch_stats.is_cpu \
                or (x.is_cuda and _as_nhwc(x).data_ptr() != x.data_ptr()):
            raise ValueError("ops.batchnorm2d: batch_stats was made for "
                             "another tensor than x")
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
        residual = _laid_out(residual, nhwc)
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
        _laid_out(x, nhwc), weight.contiguous(), bias.contiguous(), residual,
        running_mean, running_var, bool(training), float(momentum),
        float(eps), bool(fuse_relu), memory_format, batch_stats)


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
    def forward(ctx, x, kernel, stride, padding, nhwc):
        B, C, H, W = x.shape
        (kh, kw), (sh, sw), (ph, pw) = kernel, stride, padding
        ctx.geom = (B, C, H, W, kh, kw, sh, sw, ph, pw)
        ctx.nhwc = nhwc
        if x.is_cuda:
            OH = (H + 2 * ph - kh) // sh + 1
            OW = (W + 2 * pw - kw) // sw + 1
            if nhwc:    # y and the slots both lie [B][OH][OW][C]
                y = _empty_nhwc(B, C, OH, OW, x, x.dtype)
                slot = _empty_nhwc(B, C, OH, OW, x, torch.uint8)
                fwd = _k().maxpool2d_nhwc_fwd
            else:
                y = torch.empty(B, C, OH, OW, device=x.device, dtype=x.dtype)
                slot = torch.empty(B, C, OH, OW, device=x.device,
                                   dtype=torch.uint8)
                fwd = _k().maxpool2d_fwd
            fwd(x.data_ptr(), y.data_ptr(), slot.data_ptr(), *ctx.geom,
                x.dtype == torch.bfloat16, _stream())
            ctx.save_for_backward(slot)
            return y
        y, idx = F.max_pool2d(x, kernel, stride, padding,
                              return_indices=True)
        ctx.save_for_backward(idx)
        return _as_nhwc(y) if nhwc else y

    @staticmethod
    def backward(ctx, gy):
        (saved,) = ctx.saved_tensors
        B, C, H, W = ctx.geom[:4]
        gy = _laid_out(gy, ctx.nhwc)
        if gy.is_cuda:
            if ctx.nhwc:
                gx = _empty_nhwc(B, C, H, W, gy, gy.dtype)  # fully written
                bwd = _k().maxpool2d_nhwc_bwd
            else:
                gx = torch.empty(B, C, H, W, device=gy.device,
                                 dtype=gy.dtype)      # fully written
                bwd = _k().maxpool2d_bwd
            bwd(gy.data_ptr(), saved.data_ptr(), gx.data_ptr(), *ctx.geom,
                gy.dtype == torch.bfloat16, _stream())
            return gx, None, None, None, None
        gx = torch.zeros(B * C, H * W, dtype=torch.float32)
        gx.scatter_add_(1, saved.reshape(B * C, -1),
                        gy.float().reshape(B * C, -1))
        gx = gx.to(gy.dtype).view(B, C, H, W)
        return _as_nhwc(gx) if ctx.nhwc else gx, None, None, None, None


def maxpool2d(x, kernel_size, stride=None, padding=0,
              memory_format=torch.contiguous_format):
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
    gradient of overlapping windows is bitwise reproducible.

    ``memory_format=torch.channels_last`` (``conv2d_bf16``'s rules) runs
    csrc/pool_nhwc.hip on [B][H][W][C] storage: ``x`` and ``gy`` are brought
    to it at no cost where they have it, ``y`` and ``gx`` come back with
    it, and every element is the default layout's, bit for bit."""
    op = "ops.maxpool2d"
    nhwc = _is_nhwc(op, memory_format)
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
    return _MaxPool2d.apply(_laid_out(x, nhwc), (kh, kw), (sh, sw), (ph, pw),
                            nhwc)


# ---------------------------------------------------------------------------
# K20 — global average pool [B,C,H,W] -> [B,C], fp32 or bf16
# (csrc/pool.hip).  Contract, on GPU and CPU alike: each plane is summed in
# fp32, divided once by H*W and rounded once to the output dtype.  The GPU
# sum has a fixed order that depends on H*W alone, so it is bitwise
# reproducible and independent of the pointer's alignment and of the dtype.
# ---------------------------------------------------------------------------
class _GlobalAvgPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, nhwc):
        B, C, H, W = x.shape
        ctx.in_shape = (B, C, H, W)
        ctx.nhwc = nhwc
        if x.is_cuda:
            y = torch.empty(B, C, device=x.device, dtype=x.dtype)
            if nhwc:
                _k().global_avgpool2d_nhwc_fwd(
                    x.data_ptr(), y.data_ptr(), B, C, H * W,
                    x.dtype == torch.bfloat16, _stream())
            else:
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
            if ctx.nhwc:
                gx = _empty_nhwc(B, C, H, W, gy, gy.dtype)  # fully written
                _k().global_avgpool2d_nhwc_bwd(
                    gy.data_ptr(), gx.data_ptr(), B, C, H * W,
                    gy.dtype == torch.bfloat16, _stream())
                return gx, None
            gx = torch.empty(B, C, H, W, device=gy.device,
                             dtype=gy.dtype)      # fully written
            _k().global_avgpool2d_bwd(gy.data_ptr(), gx.data_ptr(), B * C,
                                      H * W, gy.dtype == torch.bfloat16,
                                      _stream())
            return gx, None
        g = (gy.float() / (H * W)).to(gy.dtype)
        gx = g.view(B, C, 1, 1).expand(B, C, H, W)
        return _as_nhwc(gx) if ctx.nhwc else gx.contiguous(), None


def global_avgpool2d(x, memory_format=torch.contiguous_format):
    """The mean of every plane: ``adaptive_avg_pool2d(x, 1).flatten(1)``.

    ``x`` [B,C,H,W] is fp32 or bf16; the result is [B,C] in its dtype.
    Each plane is summed in fp32, divided once by ``H*W`` and rounded once.
    On the GPU the order of the sum is fixed by ``H*W`` alone: the result is
    bitwise reproducible, a view at any element offset gives the bits of
    its aligned copy, and the bf16 result is the fp32 op's on the same
    values, rounded once.  Backward gives ``gx[b,c,:,:] = gy[b,c] / (H*W)``
    in ``x``'s dtype, computed in fp32 and rounded once.

    ``memory_format=torch.channels_last`` (``conv2d_bf16``'s rules) runs
    csrc/pool_nhwc.hip on [B][H][W][C] storage, which ``x`` is brought to at
    no cost where it has it; the result is still a dense [B,C] and ``gx``
    comes back channels-last.  The order of the sum is again fixed by
    ``H*W`` alone, but it is another order than the default layout's."""
    nhwc = _is_nhwc("ops.global_avgpool2d", memory_format)
    _check_pool_input("global_avgpool2d", x)
    return _GlobalAvgPool2d.apply(_laid_out(x, nhwc), nhwc)


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
