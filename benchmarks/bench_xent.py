#!/usr/bin/env python3
"""Micro-benchmark of ops.cross_entropy (K21) in fp32 and bf16 next to
ops.log_softmax_nll (fp32, the one-thread-per-row kernels of K9+K10) and
torch's F.cross_entropy, all in one process (hipEvent timing, 1 GPU), at

  [128,10]  [64,1000]  [256,1000]  [4096,1000]  [64,32768]  [2048,32768]

``--direct`` times the native forward and backward entry points alone on
preallocated buffers (cross_entropy and log_softmax_nll; torch has none);
the default and ``--markdown`` time forward and forward+backward through
autograd.  ``--sweep`` times cross_entropy's two row mappings (the lanes of
a wave per row, a block per row) against each other around the dispatch
threshold.  Printed are microseconds, effective GB/s and that rate as a
share of the 6.3 TB/s achievable HBM rate of an MI355X.  Effective GB/s
counts the MINIMUM traffic of the op, with B*N logits of e bytes each:
  forward    B*N*e          x read once
  backward   2*B*N*e        x read, gx written
Every path is accounted with the same counts (log_softmax_nll also writes
and re-reads a [B,N] logp, which is not the op's minimum), so the GB/s
compare directly.

Run on a GPU box:  python benchmarks/bench_xent.py [--markdown]
                   python benchmarks/bench_xent.py --direct
                   python benchmarks/bench_xent.py --sweep
"""

import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.utils.native import load_native  # noqa: E402

SHAPES = [(128, 10), (64, 1000), (256, 1000), (4096, 1000), (64, 32768),
          (2048, 32768)]
SWEEP = [(64, 512), (64, 1000), (256, 1000), (4096, 1000), (64, 2048),
         (256, 2048), (4096, 2048), (64, 4096), (256, 4096), (4096, 4096),
         (64, 8192), (1024, 8192)]
HBM_GBS = 6300.0   # achievable HBM rate of one MI355X
F32, BF16 = torch.float32, torch.bfloat16


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


def min_bytes(shape, dtype):
    """(forward, backward) minimum traffic in bytes."""
    n = shape[0] * shape[1] * (4 if dtype == F32 else 2)
    return n, 2 * n


def _inputs(shape, dtype, dev):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(shape, generator=g).to(dev).to(dtype)
    t = torch.randint(0, shape[1], (shape[0],), generator=g).to(dev)
    return x, t


def _direct_xent(shape, dtype, dev, mapping=0):
    k = load_native("_kernels")
    B, N = shape
    x, t = _inputs(shape, dtype, dev)
    f32 = dict(device=dev, dtype=F32)
    row, lse = torch.empty(B, **f32), torch.empty(B, **f32)
    loss, count = torch.empty(1, **f32), torch.empty(1, **f32)
    gl = torch.ones(1, **f32)
    gx = torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream
    args = (B, N, 0.0, -100, 1, dtype == BF16, mapping, st)

    def fwd():
        k.cross_entropy_fwd(x.data_ptr(), t.data_ptr(), row.data_ptr(),
                            lse.data_ptr(), loss.data_ptr(),
                            count.data_ptr(), *args)

    def bwd():
        k.cross_entropy_bwd(x.data_ptr(), t.data_ptr(), lse.data_ptr(),
                            count.data_ptr(), gl.data_ptr(), gx.data_ptr(),
                            *args)

    return fwd, bwd


def _direct_lsnll(shape, dev):
    k = load_native("_kernels")
    B, N = shape
    x, t = _inputs(shape, F32, dev)
    logp, gx = torch.empty_like(x), torch.empty_like(x)
    loss = torch.empty(1, device=dev)
    gl = torch.ones(1, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def fwd():
        k.log_softmax_nll_fwd(x.data_ptr(), t.data_ptr(), logp.data_ptr(),
                              loss.data_ptr(), B, N, st)

    def bwd():
        k.log_softmax_nll_bwd(logp.data_ptr(), t.data_ptr(), gx.data_ptr(),
                              gl.data_ptr(), B, N, st)

    return fwd, bwd


def _autograd_paths(shape, dev):
    paths = [("ops.cross_entropy fp32", F32, ops.cross_entropy),
             ("ops.cross_entropy bf16", BF16, ops.cross_entropy),
             ("ops.log_softmax_nll fp32", F32, ops.log_softmax_nll),
             ("F.cross_entropy fp32 (torch)", F32, F.cross_entropy),
             ("F.cross_entropy bf16 (torch)", BF16, F.cross_entropy)]
    out = []
    for name, dtype, fn in paths:
        x, t = _inputs(shape, dtype, dev)
        xx = x.clone().requires_grad_(True)

        def fwd(fn=fn, xx=xx, t=t):
            with torch.no_grad():
                fn(xx, t)

        def fwdbwd(fn=fn, xx=xx, t=t):
            xx.grad = None
            fn(xx, t).backward()

        out.append((name, dtype, fwd, fwdbwd))
    return out


def _desc(shape):
    return "[%d,%d]" % shape


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
    ap.add_argument("--sweep", action="store_true",
                    help="cross_entropy's two row mappings, forced, around "
                         "the dispatch threshold (direct entry points)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_xent needs a GPU"
    dev = torch.device("cuda:0")
    load_native("_kernels")
    t = lambda fn: time_fn(fn, args.reps, args.warmup)  # noqa: E731

    if args.sweep:
        print("| shape | dtype | wave fwd us | block fwd us | wave bwd us "
              "| block bwd us |")
        print("|---|---|---|---|---|---|")
        for shape in SWEEP:
            for dtype, dname in ((F32, "fp32"), (BF16, "bf16")):
                wf, wb = _direct_xent(shape, dtype, dev, mapping=1)
                bf, bb = _direct_xent(shape, dtype, dev, mapping=2)
                print("| %s | %s | %.1f | %.1f | %.1f | %.1f |"
                      % (_desc(shape), dname, t(wf), t(bf), t(wb), t(bb)),
                      flush=True)
        return

    if args.direct:
        print("| shape | path | fwd us | fwd GB/s | % of 6.3 TB/s "
              "| bwd us | bwd GB/s | % of 6.3 TB/s | fwd+bwd us |")
        print("|---|---|---|---|---|---|---|---|---|")
        for shape in SHAPES:
            paths = [("cross_entropy fp32", F32,
                      _direct_xent(shape, F32, dev)),
                     ("cross_entropy bf16", BF16,
                      _direct_xent(shape, BF16, dev)),
                     ("log_softmax_nll fp32", F32,
                      _direct_lsnll(shape, dev))]
            for name, dtype, (fwd, bwd) in paths:
                bytes_f, bytes_b = min_bytes(shape, dtype)
                t_f, t_b = t(fwd), t(bwd)
                gb_f = bytes_f / t_f * 1e-3
                gb_b = bytes_b / t_b * 1e-3
                print("| %s | %s | %.1f | %.0f | %.1f | %.1f | %.0f | %.1f "
                      "| %.1f |"
                      % (_desc(shape), name, t_f, gb_f,
                         100 * gb_f / HBM_GBS, t_b, gb_b,
                         100 * gb_b / HBM_GBS, t_f + t_b), flush=True)
        return

    rows = []
    for shape in SHAPES:
        for name, dtype, fwd, fwdbwd in _autograd_paths(shape, dev):
            print(f"timing {_desc(shape)} / {name}", file=sys.stderr,
                  flush=True)
            bytes_f, bytes_b = min_bytes(shape, dtype)
            t_f, t_fb = t(fwd), t(fwdbwd)
            gb_f = bytes_f / t_f * 1e-3
            gb_fb = (bytes_f + bytes_b) / t_fb * 1e-3
            rows.append((_desc(shape), name, t_f, gb_f,
                         100 * gb_f / HBM_GBS, t_fb, gb_fb,
                         100 * gb_fb / HBM_GBS))

    if args.markdown:
        print("| shape | path | fwd us | fwd GB/s | % of 6.3 TB/s "
              "| fwd+bwd us | fwd+bwd GB/s | % of 6.3 TB/s |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %s | %s | %.1f | %.0f | %.1f | %.1f | %.0f | %.1f |" % r)
    else:
        print(f"{'shape':<14} {'path':<30} {'fwd us':>9} {'GB/s':>7} "
              f"{'%':>6} {'fwd+bwd us':>11} {'GB/s':>7} {'%':>6}")
        for r in rows:
            print("%-14s %-30s %9.1f %7.0f %6.1f %11.1f %7.0f %6.1f" % r)


if __name__ == "__main__":
    main()
