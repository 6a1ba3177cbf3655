#!/usr/bin/env python3
"""Micro-benchmark of the bf16 MFMA linear (K16) against the fp32 linear
kernels (K7/K8) and hipBLASLt (hipEvent timing, 1 GPU).

For each shape (B, K, N) it times forward and forward+backward of
  (a) ops.linear              fp32 operands, scalar FMA kernels
  (b) ops.linear_bf16         bf16 operands (pre-cast activations, fp32
                              master weight + bias), bf16 output
  (c) F.linear on bf16        hipBLASLt, the external reference
and prints microseconds and achieved TFLOP/s (2*B*K*N per GEMM: one for
forward, three for forward+backward).

Run on a GPU box:  python benchmarks/bench_linear_bf16.py [--markdown]
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
    (128, 784, 256),      # MLP layer 1, one rank's batch
    (4096, 784, 256),     # MLP layer 1, large batch
    (4096, 256, 128),     # MLP layer 2
    (4096, 4096, 4096),   # large square
]


def time_fn(fn, reps=200, warmup=20):
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


def _variants(B, K, N, dev):
    g = torch.Generator().manual_seed(0)
    x32 = torch.randn(B, K, generator=g).to(dev)
    w32 = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b32 = torch.randn(N, generator=g).to(dev)
    gy32 = torch.randn(B, N, generator=g).to(dev)
    xb, wb, bb, gyb = (x32.bfloat16(), w32.bfloat16(), b32.bfloat16(),
                       gy32.bfloat16())

    def make(fn, x, w, b, gy):
        x = x.clone().requires_grad_(True)
        w = w.clone().requires_grad_(True)
        b = b.clone().requires_grad_(True)

        def fwd():
            with torch.no_grad():
                fn(x, w, b)

        def fwdbwd():
            x.grad = w.grad = b.grad = None
            fn(x, w, b).backward(gy)

        return fwd, fwdbwd

    return [
        ("ops.linear fp32", make(ops.linear, x32, w32, b32, gy32)),
        ("ops.linear_bf16", make(ops.linear_bf16, xb, w32, b32, gyb)),
        ("F.linear bf16 (hipBLASLt)", make(F.linear, xb, wb, bb, gyb)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--markdown", action="store_true",
                    help="print the table as markdown")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    load_native("_kernels")

    rows = []
    for B, K, N in SHAPES:
        flop = 2.0 * B * K * N
        for name, (fwd, fwdbwd) in _variants(B, K, N, dev):
            # the fp32 scalar kernels take ~100 ms at the large square
            big = flop > 1e10 and name.startswith("ops.linear fp32")
            reps = 3 if big else args.reps
            warm = 1 if big else args.warmup
            t_f = time_fn(fwd, reps, warm)
            t_fb = time_fn(fwdbwd, reps, warm)
            rows.append((B, K, N, name, t_f, flop / t_f * 1e-6,
                         t_fb, 3 * flop / t_fb * 1e-6))

    if args.markdown:
        print("| B | K | N | path | fwd us | fwd TFLOP/s | fwd+bwd us "
              "| fwd+bwd TFLOP/s |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %d | %d | %d | %s | %.1f | %.2f | %.1f | %.2f |" % r)
    else:
        print(f"{'B':>5} {'K':>5} {'N':>5}  {'path':<26} "
              f"{'fwd us':>10} {'TF/s':>8} {'fwd+bwd us':>11} {'TF/s':>8}")
        for r in rows:
            print("%5d %5d %5d  %-26s %10.1f %8.2f %11.1f %8.2f" % r)


if __name__ == "__main__":
    main()
