#!/usr/bin/env python3
"""Micro-benchmark of ops.maxpool2d (K19) and ops.global_avgpool2d (K20) at
ResNet-50's two pooling shapes (hipEvent timing, 1 GPU), fp32 and bf16,
B = 32 and 64:

  max-pool 3x3 / stride 2 / padding 1 on  B x 64 x 112 x 112
  global average pool                 on  B x 2048 x 7 x 7

For each it times forward and forward+backward of the op through autograd
next to torch's F.max_pool2d / F.adaptive_avg_pool2d on the same dtype
(default and ``--markdown``), or the native forward and backward entry
points alone on preallocated buffers (``--direct``), and prints
microseconds, effective GB/s and that rate as a share of the 6.3 TB/s
achievable HBM rate of an MI355X.  Effective GB/s counts the MINIMUM
traffic of the op.  With N input elements of e bytes each:
  max-pool forward    N*e + (N/4)*e + N/4   x read, y and the uint8 slots
                                            written (OH*OW = H*W/4 here)
  max-pool backward   (N/4)*e + N/4 + N*e   gy and slots read, gx written
  average forward     N*e + (N/HW)*e        x read, y written
  average backward    the same              gy read, gx written
Forward+backward is the sum.  torch's rows are accounted with the same
counts (its max-pool saves int64 indices, which is not this op's minimum),
so the GB/s compare directly.

Run on a GPU box:  python benchmarks/bench_pool.py [--markdown]
                   python benchmarks/bench_pool.py --direct
"""

import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.utils.native import load_native  # noqa: E402

POOL = (3, 2, 1)            # kernel, stride, padding of ResNet's stem pool
CASES = [
    ("maxpool 3/2/1", (32, 64, 112, 112)),
    ("maxpool 3/2/1", (64, 64, 112, 112)),
    ("global avg", (32, 2048, 7, 7)),
    ("global avg", (64, 2048, 7, 7)),
]
DTYPES = ((torch.float32, "fp32"), (torch.bfloat16, "bf16"))
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


def min_bytes(kind, shape, dtype):
    """(forward, backward) minimum traffic in bytes."""
    B, C, H, W = shape
    n = B * C * H * W
    e = 4 if dtype == torch.float32 else 2
    if kind.startswith("maxpool"):
        k, s, p = POOL
        no = B * C * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
        return n * e + no * e + no, no * e + no + n * e
    return n * e + (n // (H * W)) * e, (n // (H * W)) * e + n * e


def _out_shape(kind, shape):
    B, C, H, W = shape
    if kind.startswith("maxpool"):
        k, s, p = POOL
        return (B, C, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    return (B, C)


def _inputs(kind, shape, dtype, dev):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(shape, generator=g)
    if kind.startswith("maxpool"):
        x = F.relu(x)        # the stem pool reads a ReLU output: many ties
    gy = torch.randn(_out_shape(kind, shape), generator=g)
    return x.to(dev).to(dtype), gy.to(dev).to(dtype)


def _variants(kind, shape, dtype, dev):
    x, gy = _inputs(kind, shape, dtype, dev)
    if kind.startswith("maxpool"):
        paths = [("ops.maxpool2d", lambda t: ops.maxpool2d(t, *POOL)),
                 ("F.max_pool2d (torch)", lambda t: F.max_pool2d(t, *POOL))]
    else:
        paths = [("ops.global_avgpool2d", ops.global_avgpool2d),
                 ("F.adaptive_avg_pool2d (torch)",
                  lambda t: F.adaptive_avg_pool2d(t, 1).flatten(1))]

    def make(fn):
        xx = x.clone().requires_grad_(True)

        def fwd():
            with torch.no_grad():
                fn(xx)

        def fwdbwd():
            xx.grad = None
            fn(xx).backward(gy)

        return fwd, fwdbwd

    return [(name, make(fn)) for name, fn in paths]


def _direct(kind, shape, dtype, dev):
    """The native entry points on preallocated buffers: no autograd, no
    allocation, one launch each."""
    k = load_native("_kernels")
    B, C, H, W = shape
    x, gy = _inputs(kind, shape, dtype, dev)
    y = torch.empty_like(gy)
    gx = torch.empty_like(x)
    bf = dtype == torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    if kind.startswith("maxpool"):
        ks, s, p = POOL
        geom = (B, C, H, W, ks, ks, s, s, p, p)
        slot = torch.empty(gy.shape, device=dev, dtype=torch.uint8)

        def fwd():
            k.maxpool2d_fwd(x.data_ptr(), y.data_ptr(), slot.data_ptr(),
                            *geom, bf, st)

        def bwd():
            k.maxpool2d_bwd(gy.data_ptr(), slot.data_ptr(), gx.data_ptr(),
                            *geom, bf, st)
    else:
        def fwd():
            k.global_avgpool2d_fwd(x.data_ptr(), y.data_ptr(), B * C, H * W,
                                   bf, st)

        def bwd():
            k.global_avgpool2d_bwd(gy.data_ptr(), gx.data_ptr(), B * C,
                                   H * W, bf, st)

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
    assert torch.cuda.is_available(), "bench_pool needs a GPU"
    dev = torch.device("cuda:0")
    load_native("_kernels")

    if args.direct:
        print("| op | shape | fwd us | fwd GB/s | % of 6.3 TB/s "
              "| bwd us | bwd GB/s | % of 6.3 TB/s |")
        print("|---|---|---|---|---|---|---|---|")
        for kind, shape in CASES:
            for dtype, dname in DTYPES:
                desc = "x".join(str(v) for v in shape) + " " + dname
                bytes_f, bytes_b = min_bytes(kind, shape, dtype)
                fwd, bwd = _direct(kind, shape, dtype, dev)
                t_f = time_fn(fwd, args.reps, args.warmup)
                t_b = time_fn(bwd, args.reps, args.warmup)
                gb_f = bytes_f / t_f * 1e-3
                gb_b = bytes_b / t_b * 1e-3
                print("| %s | %s | %.1f | %.0f | %.1f | %.1f | %.0f | %.1f |"
                      % (kind, desc, t_f, gb_f, 100 * gb_f / HBM_GBS, t_b,
                         gb_b, 100 * gb_b / HBM_GBS))
        return

    rows = []
    for kind, shape in CASES:
        for dtype, dname in DTYPES:
            desc = "x".join(str(v) for v in shape) + " " + dname
            bytes_f, bytes_b = min_bytes(kind, shape, dtype)
            for name, fns in _variants(kind, shape, dtype, dev):
                print(f"timing {desc} / {name}", file=sys.stderr, flush=True)
                t_f = time_fn(fns[0], args.reps, args.warmup)
                t_fb = time_fn(fns[1], args.reps, args.warmup)
                gb_f = bytes_f / t_f * 1e-3          # GB/s
                gb_fb = (bytes_f + bytes_b) / t_fb * 1e-3
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
