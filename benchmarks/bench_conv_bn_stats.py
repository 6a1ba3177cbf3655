#!/usr/bin/env python3
"""Micro-benchmark of the batch-norm statistics fused into the channels-last
convolution's epilogue, at ResNet-50's convolution shapes for B=32
(bench_conv_nhwc.py's), bf16 activations and output (hipEvent timing, 1 GPU).

The native launchers run on preallocated buffers, no allocation and no
autograd.  Four things are timed per shape:
  conv      conv2d_nhwc_bf16_fwd                        the parent's forward
  conv+ep   conv2d_nhwc_bf16_fwd_stats                  with the epilogue
  unfused   conv, then batchnorm2d_nhwc_fwd             stats, finalize, apply
  fused     conv+ep, then ..._fwd_from_partials         merge(s), apply
Both pairs end in the same apply kernel on the same tensor (plain training
batch norm with ReLU), so their difference is statistics + finalize against
epilogue + merge.

Every cell is measured --rounds times, the four alternating inside a round,
and reported as median (min-max).  The fused pair counts as faster where its
median is below the unfused one's by more than the larger of the two min-max
spreads, as SLOWER in the mirrored case, else as equal.

Run on a GPU box:  python benchmarks/bench_conv_bn_stats.py [--markdown]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd.utils.native import load_native  # noqa: E402
from bench_conv_nhwc import SHAPES, time_fn  # noqa: E402
from bench_nhwc_ops import verdict  # noqa: E402

WHAT = ("conv", "conv+ep", "unfused", "fused")


def fns(shape, dev):
    B, C, H, W, K, R, S, stride, padding, _ = shape
    k = load_native("_kernels")
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, H, W, C, generator=g).bfloat16().to(dev)
    w = (torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5).to(dev)
    OH = (H + 2 * padding - R) // stride + 1
    OW = (W + 2 * padding - S) // stride + 1
    rows = B * OH * OW
    dims = (B, C, H, W, K, R, S, stride, stride, padding, padding)
    wp = torch.empty(K, R, S, C, device=dev, dtype=torch.bfloat16)
    k.conv2d_nhwc_bf16_pack_w(w.data_ptr(), wp.data_ptr(), K, C, R, S, True,
                              False, st)
    out = torch.empty(B, OH, OW, K, device=dev, dtype=torch.bfloat16)
    y = torch.empty_like(out)
    gamma, beta, mean, inv = (torch.ones(K, device=dev) for _ in range(4))
    tiles = k.conv2d_nhwc_bf16_stats_tiles(rows)
    tws = torch.empty(tiles, K, 2, device=dev)
    mws = torch.empty(max(1, k.batchnorm2d_nhwc_merge_ws(rows, K)),
                      device=dev)
    splits = k.batchnorm2d_nhwc_splits(rows, K)
    ws = torch.empty(K * splits * 3, device=dev)

    def conv():
        k.conv2d_nhwc_bf16_fwd(x.data_ptr(), wp.data_ptr(), 0,
                               out.data_ptr(), *dims, False, st)

    def conv_ep():
        k.conv2d_nhwc_bf16_fwd_stats(x.data_ptr(), wp.data_ptr(), 0,
                                     out.data_ptr(), tws.data_ptr(), *dims,
                                     False, st)

    def unfused():
        conv()
        k.batchnorm2d_nhwc_fwd(
            out.data_ptr(), 0, y.data_ptr(), gamma.data_ptr(),
            beta.data_ptr(), 0, 0, mean.data_ptr(), inv.data_ptr(),
            ws.data_ptr(), splits, rows, K, True, 0.1, 1e-5, True, True, st)

    def fused():
        conv_ep()
        k.batchnorm2d_nhwc_fwd_from_partials(
            out.data_ptr(), 0, y.data_ptr(), gamma.data_ptr(),
            beta.data_ptr(), 0, 0, mean.data_ptr(), inv.data_ptr(),
            tws.data_ptr(), mws.data_ptr(), rows, K, 0.1, 1e-5, True, True,
            st)

    return dict(zip(WHAT, (conv, conv_ep, unfused, fused))), tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_bn_stats needs a GPU"
    dev = torch.device("cuda:0")

    def cell(v):
        return f"{statistics.median(v):.1f} ({min(v):.1f}-{max(v):.1f})"

    if args.markdown:
        print("| shape | row tiles | " + " us | ".join(WHAT)
              + " us | fused - unfused us | ratio | fused is |")
        print("|---" * (len(WHAT) + 5) + "|")
    for shape in SHAPES:
        B, C, H, W, K, R, S, stride, padding, label = shape
        desc = f"{label}: {B}x{C}x{H}x{W}, {K}x{R}x{S}, s{stride} p{padding}"
        print(f"timing {desc}", file=sys.stderr, flush=True)
        f, tiles = fns(shape, dev)
        t = {p: [] for p in WHAT}
        for _ in range(args.rounds):
            for p in WHAT:      # the four alternate inside a round
                t[p].append(time_fn(f[p], args.reps, args.warmup))
        a, b = t["unfused"], t["fused"]
        ma, mb = statistics.median(a), statistics.median(b)
        cols = [desc, str(tiles), *(cell(t[p]) for p in WHAT),
                f"{mb - ma:+.1f}", f"{mb / ma:.2f}", verdict(a, b)]
        print("| " + " | ".join(cols) + " |" if args.markdown
              else "  ".join(cols), flush=True)
        del f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
