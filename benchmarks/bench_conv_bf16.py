#!/usr/bin/env python3
"""Micro-benchmark of the bf16 MFMA convolution (K17) against the fp32
direct convolution (K1/K2) and MIOpen (hipEvent timing, 1 GPU).

For each shape (B,C,H,W, K,R,S, stride, padding) it times forward and
forward+backward of
  (a) ops.conv2d              fp32 direct kernel; stride 1, no padding and
                              Net-sized planes only, "n/a" elsewhere
  (b) ops.conv2d_bf16         bf16 activations, fp32 master weight + bias,
                              bf16 output
  (c) F.conv2d on bf16        MIOpen, the external reference
and prints microseconds and achieved TFLOP/s (2*B*OH*OW*K*C*R*S per
product: one for forward, three for forward+backward).  It then times one
modular training step of Net (forward_logits, fused loss, backward,
FusedSGD) in fp32 and in bf16 mode.

Run on a GPU box:  python benchmarks/bench_conv_bf16.py [--markdown]
"""

import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.models import Net  # noqa: E402
from dist_tuto_pth_amd.optim import FusedSGD  # noqa: E402
from dist_tuto_pth_amd.utils.native import load_native  # noqa: E402

SHAPES = [
    # (B, C, H, W, K, R, S, stride, padding, label)
    (128, 1, 28, 28, 10, 5, 5, 1, 0, "Net conv1"),
    (4096, 1, 28, 28, 10, 5, 5, 1, 0, "Net conv1"),
    (128, 10, 12, 12, 20, 5, 5, 1, 0, "Net conv2"),
    (4096, 10, 12, 12, 20, 5, 5, 1, 0, "Net conv2"),
    (32, 64, 56, 56, 64, 3, 3, 1, 1, "3x3 pad 1"),
    (32, 64, 56, 56, 128, 1, 1, 2, 0, "1x1 stride 2"),
]
NET_STEP_B = 4096


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


def _variants(shape, dev):
    B, C, H, W, K, R, S, stride, padding, _ = shape
    g = torch.Generator().manual_seed(0)
    x32 = torch.randn(B, C, H, W, generator=g).to(dev)
    w32 = (torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5).to(dev)
    b32 = torch.randn(K, generator=g).to(dev)
    OH = (H + 2 * padding - R) // stride + 1
    OW = (W + 2 * padding - S) // stride + 1
    gy32 = torch.randn(B, K, OH, OW, generator=g).to(dev)
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

    def conv_bf16(x, w, b):
        return ops.conv2d_bf16(x, w, b, stride=stride, padding=padding)

    def miopen(x, w, b):
        return F.conv2d(x, w, b, stride, padding)

    # the fp32 direct kernel stages one sample's planes and the whole
    # filter in LDS: Net's own shapes only
    direct_ok = stride == 1 and padding == 0 and C * H * W <= 2048
    return OH, OW, [
        ("ops.conv2d fp32",
         make(ops.conv2d, x32, w32, b32, gy32) if direct_ok else None),
        ("ops.conv2d_bf16", make(conv_bf16, xb, w32, b32, gyb)),
        ("F.conv2d bf16 (MIOpen)", make(miopen, xb, wb, bb, gyb)),
    ]


def _net_step(compute_dtype, dev, reps, warmup):
    torch.manual_seed(0)
    net = Net(compute_dtype=compute_dtype).to(dev)
    net.train()
    opt = FusedSGD(net.parameters(), lr=0.01, momentum=0.5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(NET_STEP_B, 1, 28, 28, generator=g).to(dev)
    tgt = torch.randint(0, 10, (NET_STEP_B,), generator=g).to(dev)

    def step():
        opt.zero_grad()
        ops.log_softmax_nll(net.forward_logits(x), tgt).backward()
        opt.step()

    return time_fn(step, reps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--markdown", action="store_true",
                    help="print the tables as markdown")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_bf16 needs a GPU"
    dev = torch.device("cuda:0")
    load_native("_kernels")

    rows = []
    for shape in SHAPES:
        B, C, H, W, K, R, S, stride, padding, label = shape
        OH, OW, variants = _variants(shape, dev)
        flop = 2.0 * B * OH * OW * K * C * R * S
        desc = (f"{label}: {B}x{C}x{H}x{W}, {K}x{R}x{S}, s{stride} "
                f"p{padding}")
        for name, fns in variants:
            print(f"timing {desc} / {name}", file=sys.stderr, flush=True)
            if fns is None:
                rows.append((desc, name, None))
                continue
            t_f = time_fn(fns[0], args.reps, args.warmup)
            t_fb = time_fn(fns[1], args.reps, args.warmup)
            rows.append((desc, name, (t_f, flop / t_f * 1e-6, t_fb,
                                      3 * flop / t_fb * 1e-6)))
    steps = [("fp32", _net_step(None, dev, args.reps, args.warmup)),
             ("bf16", _net_step(torch.bfloat16, dev, args.reps,
                                args.warmup))]

    if args.markdown:
        print("| shape | path | fwd us | fwd TFLOP/s | fwd+bwd us "
              "| fwd+bwd TFLOP/s |")
        print("|---|---|---|---|---|---|")
        for desc, name, r in rows:
            if r is None:
                print(f"| {desc} | {name} | n/a | n/a | n/a | n/a |")
            else:
                print("| %s | %s | %.1f | %.3f | %.1f | %.3f |"
                      % ((desc, name) + r))
        print()
        print(f"| Net modular step, B={NET_STEP_B} | us |")
        print("|---|---|")
        for mode, t in steps:
            print(f"| {mode} | {t:.1f} |")
    else:
        print(f"{'shape':<46} {'path':<24} {'fwd us':>10} {'TF/s':>8} "
              f"{'fwd+bwd us':>11} {'TF/s':>8}")
        for desc, name, r in rows:
            if r is None:
                print(f"{desc:<46} {name:<24} {'n/a':>10} {'n/a':>8} "
                      f"{'n/a':>11} {'n/a':>8}")
            else:
                print("%-46s %-24s %10.1f %8.3f %11.1f %8.3f"
                      % ((desc, name) + r))
        for mode, t in steps:
            print(f"Net modular step B={NET_STEP_B} {mode}: {t:.1f} us")


if __name__ == "__main__":
    main()
