#!/usr/bin/env python3
"""Micro-benchmark of ops.batchnorm2d (K18) at ResNet-50's BN shapes
(hipEvent timing, 1 GPU), fp32 and bf16, training mode.

For each shape (B,C,H,W) and dtype it times forward and forward+backward of
  (a) ops.batchnorm2d                         plain BN
  (b) ops.batchnorm2d(residual=r, fuse_relu)  BN + add + ReLU in one pass
  (c) relu(F.batch_norm(x) + r) on torch      MIOpen + two elementwise
                                              kernels, the external reference
and prints microseconds, effective GB/s and that rate as a share of the
6.3 TB/s achievable HBM rate of an MI355X.  Effective GB/s counts the
MINIMUM traffic of the op, in tensors of B*C*H*W elements:
  plain forward   3   x read twice (statistics, apply), y written
  plain backward  5   x and gy read twice (reduce, apply), gx written
  fused forward   4   + the residual read
  fused backward  7   + y read (the ReLU mask) and g_residual written
Forward+backward is the sum.  Rows (b) and (c) are both accounted with the
fused counts, so their GB/s compare directly.  The kernels move more than
the minimum (the statistics kernel reads its slice twice, the second time
from L2; the fused backward reads y in both passes), which is the point
of reporting against the minimum.

Rows (a) and (b) go through autograd and allocate their outputs, so small
shapes and every forward+backward column carry that host cost; ``--direct``
times the native forward and backward entry points alone on preallocated
buffers, with the same accounting.

Run on a GPU box:  python benchmarks/bench_batchnorm.py [--markdown]
                   python benchmarks/bench_batchnorm.py --direct
"""

import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.utils.native import load_native  # noqa: E402

SHAPES = [
    (32, 64, 112, 112),
    (32, 256, 56, 56),
    (32, 512, 28, 28),
    (32, 1024, 14, 14),
    (32, 2048, 7, 7),
]
HBM_GBS = 6300.0   # achievable HBM rate of one MI355X


def time_fn(fn, reps=100, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1000.0  # us


def _variants(shape, dtype, dev):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, H, W, generator=g).to(dev).to(dtype)
    r = torch.randn(B, C, H, W, generator=g).to(dev).to(dtype)
    gy = torch.randn(B, C, H, W, generator=g).to(dev).to(dtype)
    w32 = (0.5 + torch.rand(C, generator=g)).to(dev)
    b32 = torch.randn(C, generator=g).to(dev)

    def make(fn, w, b, with_res):
        xx = x.clone().requires_grad_(True)
        rr = r.clone().requires_grad_(True) if with_res else None
        w = w.clone().requires_grad_(True)
        b = b.clone().requires_grad_(True)
        rm = torch.zeros(C, device=dev, dtype=w.dtype)
        rv = torch.ones(C, device=dev, dtype=w.dtype)

        def fwd():
            with torch.no_grad():
                fn(xx, w, b, rm, rv, rr)

        def fwdbwd():
            xx.grad = w.grad = b.grad = None
            if rr is not None:
                rr.grad = None
            fn(xx, w, b, rm, rv, rr).backward(gy)

        return fwd, fwdbwd

    def plain(xx, w, b, rm, rv, rr):
        return ops.batchnorm2d(xx, w, b, rm, rv, training=True)

    def fused(xx, w, b, rm, rv, rr):
        return ops.batchnorm2d(xx, w, b, rm, rv, training=True, residual=rr,
                               fuse_relu=True)

    def torch_ref(xx, w, b, rm, rv, rr):
        return F.relu(F.batch_norm(xx, rm, rv, w, b, True, 0.1, 1e-5) + rr)

    return [
        ("ops.batchnorm2d", make(plain, w32, b32, False), (3, 5)),
        ("ops.batchnorm2d +add+ReLU", make(fused, w32, b32, True), (4, 7)),
        ("F.batch_norm, add, relu (torch)",
         make(torch_ref, w32, b32, True), (4, 7)),
    ]


def _direct(shape, dtype, fused, dev):
    """The native entry points on preallocated buffers: no autograd, no
    allocation, so the time is the kernels' (three launches forward, three
    backward) wherever they outlast their own launch cost."""
    k = load_native("_kernels")
    B, C, H, W = shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, H, W, generator=g).to(dev).to(dtype)
    r = torch.randn(B, C, H, W, generator=g).to(dev).to(dtype)
    gy = torch.randn(B, C, H, W, generator=g).to(dev).to(dtype)
    w = (0.5 + torch.rand(C, generator=g)).to(dev)
    b = torch.randn(C, generator=g).to(dev)
    y, gx, gr = (torch.empty_like(x) for _ in range(3))
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    mean, inv, gw, gb = (torch.empty(C, device=dev) for _ in range(4))
    splits = k.batchnorm2d_splits(B, C, H * W)
    ws = torch.empty(C * splits * 3, device=dev)
    bf = dtype == torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream

    def fwd():
        k.batchnorm2d_fwd(x.data_ptr(), r.data_ptr() if fused else 0,
                          y.data_ptr(), w.data_ptr(), b.data_ptr(),
                          rm.data_ptr(), rv.data_ptr(), mean.data_ptr(),
                          inv.data_ptr(), ws.data_ptr(), splits, B, C, H * W,
                          True, 0.1, 1e-5, fused, bf, st)

    def bwd():
        k.batchnorm2d_bwd(x.data_ptr(), gy.data_ptr(),
                          y.data_ptr() if fused else 0, w.data_ptr(),
                          mean.data_ptr(), inv.data_ptr(), gw.data_ptr(),
                          gb.data_ptr(), gx.data_ptr(),
                          gr.data_ptr() if fused else 0, ws.data_ptr(),
                          splits, B, C, H * W, True, 1e-5, bf, st)

    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--markdown", action="store_true",
                    help="print the table as markdown")
    ap.add_argument("--direct", action="store_true",
                    help="time the native forward and backward entry "
                         "points on preallocated buffers instead of the "
                         "autograd op")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_batchnorm needs a GPU"
    dev = torch.device("cuda:0")
    load_native("_kernels")

    if args.direct:
        print("| shape | form | fwd us | fwd GB/s | % of 6.3 TB/s "
              "| bwd us | bwd GB/s | % of 6.3 TB/s |")
        print("|---|---|---|---|---|---|---|---|")
        for shape in SHAPES:
            for dtype, dname in ((torch.float32, "fp32"),
                                 (torch.bfloat16, "bf16")):
                desc = "x".join(str(v) for v in shape) + " " + dname
                nbytes = float(torch.Size(shape).numel()) * \
                    (4 if dtype == torch.float32 else 2)
                for fused, (cf, cb) in ((False, (3, 5)), (True, (4, 7))):
                    fwd, bwd = _direct(shape, dtype, fused, dev)
                    t_f = time_fn(fwd, args.reps, args.warmup)
                    t_b = time_fn(bwd, args.reps, args.warmup)
                    gb_f = cf * nbytes / t_f * 1e-3
                    gb_b = cb * nbytes / t_b * 1e-3
                    print("| %s | %s | %.1f | %.0f | %.1f | %.1f | %.0f "
                          "| %.1f |" % (
                              desc, "+add+ReLU" if fused else "plain", t_f,
                              gb_f, 100 * gb_f / HBM_GBS, t_b, gb_b,
                              100 * gb_b / HBM_GBS))
        return

    rows = []
    for shape in SHAPES:
        for dtype, dname in ((torch.float32, "fp32"),
                             (torch.bfloat16, "bf16")):
            desc = "x".join(str(v) for v in shape) + " " + dname
            nbytes = float(torch.Size(shape).numel()) * \
                (4 if dtype == torch.float32 else 2)
            for name, fns, (cf, cb) in _variants(shape, dtype, dev):
                print(f"timing {desc} / {name}", file=sys.stderr, flush=True)
                t_f = time_fn(fns[0], args.reps, args.warmup)
                t_fb = time_fn(fns[1], args.reps, args.warmup)
                gb_f = cf * nbytes / t_f * 1e-3          # GB/s
                gb_fb = (cf + cb) * nbytes / t_fb * 1e-3
                rows.append((desc, name, t_f, gb_f, 100 * gb_f / HBM_GBS,
                             t_fb, gb_fb, 100 * gb_fb / HBM_GBS))

    if args.markdown:
        print("| shape | path | fwd us | fwd GB/s | % of 6.3 TB/s "
              "| fwd+bwd us | fwd+bwd GB/s | % of 6.3 TB/s |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %s | %s | %.1f | %.0f | %.1f | %.1f | %.0f | %.1f |" % r)
    else:
        print(f"{'shape':<24} {'path':<32} {'fwd us':>9} {'GB/s':>7} "
              f"{'%':>6} {'fwd+bwd us':>11} {'GB/s':>7} {'%':>6}")
        for r in rows:
            print("%-24s %-32s %9.1f %7.0f %6.1f %11.1f %7.0f %6.1f" % r)


if __name__ == "__main__":
    main()
