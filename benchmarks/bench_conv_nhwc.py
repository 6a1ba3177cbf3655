#!/usr/bin/env python3
"""Micro-benchmark of the channels-last bf16 MFMA convolution
(csrc/conv_nhwc_bf16.hip) against the NCHW one (csrc/conv_bf16.hip) and
MIOpen, at ResNet-50's convolution shapes for B=32 (hipEvent timing, 1 GPU).

For each shape (B,C,H,W, K,R,S, stride, padding) and each product (forward,
gx, gw+gb) it times
  (a) ops.conv2d_bf16                               NCHW
  (b) ops.conv2d_bf16(memory_format=channels_last)  channels-last
  (c) F.conv2d on bf16 channels_last tensors        MIOpen, for the record
with bf16 activations, an fp32 master weight and bias for (a) and (b), and a
bf16 output.  The backward products are timed through torch.autograd.grad
on a retained graph in which x alone (gx) or w and b alone (gw) require a
gradient.

--direct times the native launchers of (a) and (b) on preallocated buffers
instead: no allocation, cast, weight packing or autograd, the kernels alone
(gw includes its combine kernel).

Every cell is measured --rounds times, the paths alternating inside a
round, and reported as median (min-max), with the ratio of the medians
(b)/(a).  (b) counts as faster than (a) where its median is below (a)'s by
more than the larger of the two min-max spreads; that verdict is given for
forward and gx at the shapes with C % 8 == 0, every other row is
"recorded".

Run on a GPU box:  python benchmarks/bench_conv_nhwc.py [--direct] [--markdown]
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.utils.native import load_native  # noqa: E402

CL = torch.channels_last
SHAPES = [
    # (B, C, H, W, K, R, S, stride, padding, label)
    (32, 64, 56, 56, 64, 3, 3, 1, 1, "3x3 p1"),
    (32, 256, 56, 56, 64, 1, 1, 1, 0, "1x1"),
    (32, 128, 28, 28, 128, 3, 3, 1, 1, "3x3 p1"),
    (32, 256, 14, 14, 256, 3, 3, 1, 1, "3x3 p1"),
    (32, 512, 7, 7, 512, 3, 3, 1, 1, "3x3 p1"),
    (32, 1024, 14, 14, 256, 1, 1, 1, 0, "1x1"),
    (32, 256, 56, 56, 512, 1, 1, 2, 0, "1x1 s2"),
    (32, 3, 224, 224, 64, 7, 7, 2, 3, "stem"),
]
PRODUCTS = ("fwd", "gx", "gw")
PATHS = ("NCHW", "channels_last", "MIOpen")


def time_fn(fn, reps, warmup):
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


def _inputs(shape, dev):
    B, C, H, W, K, R, S, stride, padding, _ = shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, H, W, generator=g).bfloat16().to(dev)
    w = (torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5).to(dev)
    b = torch.randn(K, generator=g).to(dev)
    OH = (H + 2 * padding - R) // stride + 1
    OW = (W + 2 * padding - S) // stride + 1
    gy = torch.randn(B, K, OH, OW, generator=g).bfloat16().to(dev)
    return x, w, b, gy, OH, OW


def _autograd_fns(shape, dev):
    """{path: {product: fn}} through the public interface."""
    _, _, _, _, _, _, _, stride, padding, _ = shape
    x, w, b, gy, _, _ = _inputs(shape, dev)

    def make(fn, x, w, b, gy):
        # an autograd.Function computes the gradient of every input that
        # required one in forward, so each product gets a graph of its own
        xg = x.clone().requires_grad_(True)
        wg = w.clone().requires_grad_(True)
        bg = b.clone().requires_grad_(True)
        out_x = fn(xg, w, b)
        out_w = fn(x, wg, bg)

        def fwd():
            with torch.no_grad():
                fn(x, w, b)

        return {
            "fwd": fwd,
            "gx": lambda: torch.autograd.grad(out_x, xg, gy,
                                              retain_graph=True),
            "gw": lambda: torch.autograd.grad(out_w, (wg, bg), gy,
                                              retain_graph=True),
        }

    def nchw(x, w, b):
        return ops.conv2d_bf16(x, w, b, stride=stride, padding=padding)

    def nhwc(x, w, b):
        return ops.conv2d_bf16(x, w, b, stride=stride, padding=padding,
                               memory_format=CL)

    def miopen(x, w, b):
        return F.conv2d(x, w, b, stride, padding)

    xc, gyc = x.contiguous(memory_format=CL), gy.contiguous(memory_format=CL)
    return {
        "NCHW": make(nchw, x, w, b, gy),
        "channels_last": make(nhwc, xc, w, b, gyc),
        "MIOpen": make(miopen, xc,
                       w.bfloat16().contiguous(memory_format=CL),
                       b.bfloat16(), gyc),
    }


def _direct_fns(shape, dev):
    """{path: {product: fn}}: the native launchers on preallocated buffers."""
    B, C, H, W, K, R, S, stride, padding, _ = shape
    k = load_native("_kernels")
    x, w, b, gy, OH, OW = _inputs(shape, dev)
    st = torch.cuda.current_stream().cuda_stream
    dims = (B, C, H, W, K, R, S, stride, stride, padding, padding)
    bf16, f32 = torch.bfloat16, torch.float32
    gw = torch.empty(K, C, R, S, device=dev, dtype=f32)
    gb = torch.empty(K, device=dev, dtype=f32)

    def part(splits):
        return torch.empty(max(splits, 1) * (gw.numel() + K), device=dev,
                           dtype=f32)

    # NCHW
    wb = w.bfloat16()
    out = torch.empty(B, K, OH, OW, device=dev, dtype=bf16)
    gx = torch.empty(B, C, H, W, device=dev, dtype=bf16)
    s1 = k.conv2d_bf16_gw_splits(*dims)
    p1 = part(s1)
    nchw = {
        "fwd": lambda: k.conv2d_bf16_fwd(
            x.data_ptr(), wb.data_ptr(), b.data_ptr(), out.data_ptr(), *dims,
            False, st),
        "gx": lambda: k.conv2d_bf16_bwd_x(
            gy.data_ptr(), wb.data_ptr(), gx.data_ptr(), *dims, False, st),
        "gw": lambda: k.conv2d_bf16_bwd_w(
            gy.data_ptr(), x.data_ptr(), gw.data_ptr(), gb.data_ptr(),
            p1.data_ptr() if s1 > 1 else 0, s1, *dims, st),
    }
    # channels-last: the same values, stored [B][H][W][C]
    xc = x.permute(0, 2, 3, 1).contiguous()
    gyc = gy.permute(0, 2, 3, 1).contiguous()
    wf = torch.empty(K, R, S, C, device=dev, dtype=bf16)
    wx = torch.empty(C, R, S, K, device=dev, dtype=bf16)
    k.conv2d_nhwc_bf16_pack_w(w.data_ptr(), wf.data_ptr(), K, C, R, S, True,
                              False, st)
    k.conv2d_nhwc_bf16_pack_w(w.data_ptr(), wx.data_ptr(), K, C, R, S, True,
                              True, st)
    outc = torch.empty(B, OH, OW, K, device=dev, dtype=bf16)
    gxc = torch.empty(B, H, W, C, device=dev, dtype=bf16)
    s2 = k.conv2d_nhwc_bf16_gw_splits(*dims)
    p2 = part(s2)
    nhwc = {
        "fwd": lambda: k.conv2d_nhwc_bf16_fwd(
            xc.data_ptr(), wf.data_ptr(), b.data_ptr(), outc.data_ptr(),
            *dims, False, st),
        "gx": lambda: k.conv2d_nhwc_bf16_bwd_x(
            gyc.data_ptr(), wx.data_ptr(), gxc.data_ptr(), *dims, False, st),
        "gw": lambda: k.conv2d_nhwc_bf16_bwd_w(
            gyc.data_ptr(), xc.data_ptr(), gw.data_ptr(), gb.data_ptr(),
            p2.data_ptr() if s2 > 1 else 0, s2, *dims, st),
    }
    return {"NCHW": nchw, "channels_last": nhwc}


def verdict(shape, prod, a, b):
    """(b) against (a), each a list of round timings.  Only forward and gx
    at shapes with C % 8 == 0 are judged; the rest is recorded."""
    if prod == "gw" or shape[1] % 8:
        return "recorded"
    spread = max(max(a) - min(a), max(b) - min(b))
    return "faster" if statistics.median(b) < statistics.median(a) - spread \
        else "NOT faster"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--direct", action="store_true",
                    help="time the native launchers on preallocated buffers")
    ap.add_argument("--markdown", action="store_true",
                    help="print the table as markdown")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_nhwc needs a GPU"
    dev = torch.device("cuda:0")
    load_native("_kernels")

    rows = []
    for shape in SHAPES:
        B, C, H, W, K, R, S, stride, padding, label = shape
        desc = (f"{label}: {B}x{C}x{H}x{W}, {K}x{R}x{S}, s{stride} "
                f"p{padding}")
        print(f"timing {desc}", file=sys.stderr, flush=True)
        fns = (_direct_fns if args.direct else _autograd_fns)(shape, dev)
        for prod in PRODUCTS:
            t = {p: [] for p in fns}
            for _ in range(args.rounds):
                for p in fns:  # the paths alternate inside a round
                    t[p].append(time_fn(fns[p][prod], args.reps, args.warmup))
            rows.append((shape, desc, prod, t))
        del fns
        torch.cuda.empty_cache()

    def cell(v):
        return f"{statistics.median(v):.1f} ({min(v):.1f}-{max(v):.1f})"

    paths = [p for p in PATHS if p in rows[0][3]]  # no MIOpen with --direct
    if args.markdown:
        print("| shape | product | " + " us | ".join(paths)
              + " us | ratio | channels_last vs NCHW |")
        print("|---" * (len(paths) + 4) + "|")
    for shape, desc, prod, t in rows:
        cells = [cell(t[p]) for p in paths]
        a, b = t["NCHW"], t["channels_last"]
        ratio = f"{statistics.median(b) / statistics.median(a):.2f}"
        v = verdict(shape, prod, a, b)
        if args.markdown:
            print(f"| {desc} | {prod} | " + " | ".join(cells)
                  + f" | {ratio} | {v} |")
        else:
            print(f"{desc:<40} {prod:<4} "
                  + " ".join(f"{c:>24}" for c in cells) + f"  {ratio}  {v}")


if __name__ == "__main__":
    main()
