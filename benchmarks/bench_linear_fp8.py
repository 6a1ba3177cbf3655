#!/usr/bin/env python3
"""Micro-benchmark of the fp8 linear (K22, csrc/linear_fp8.hip) against the
bf16 MFMA linear (K16) of the same build (hipEvent timing, 1 GPU).

Per shape (B, K, N) it times the three products of a layer, each two ways:
  fp8 +q   the GEMM with the quantiser passes it needs in a training step:
           forward quantises x and w (both copies each), gx and gw quantise
           gy (one copy each; a real backward quantises gy once for both)
  fp8      the GEMM kernel alone on pre-quantised operands (gw with its
           split combine)
  bf16     K16's kernel on bf16 operands (gw with its split combine)
The sides alternate and every cell is the median (min-max) of three
measurements, in microseconds.  A second table gives the MLP training step
in its three modes.  --probe prints what the 128-deep instruction keeps of
small terms next to a large one.

--scaling mx compares K23's MXFP8 path with the per-tensor path instead of
bf16: `tensor +q` / `mx +q` and `tensor` / `mx` (GEMM alone) per product, and
the MLP step in bf16, fp8 per-tensor and fp8 MX.  With it, --probe prints
which stored scale byte the scaled instruction applies to which data.

Run on a GPU box:
    python benchmarks/bench_linear_fp8.py [--scaling mx] [--probe]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.models import MLP  # noqa: E402
from dist_tuto_pth_amd.optim import FusedSGD  # noqa: E402
from dist_tuto_pth_amd.utils.native import load_native  # noqa: E402

SHAPES = [
    (128, 784, 256),      # MLP layer 1, one rank's batch
    (4096, 784, 256),     # MLP layer 1, large batch
    (4096, 256, 128),     # MLP layer 2
    (2048, 2048, 2048),
    (4096, 4096, 4096),   # GEMM-bound
]
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


def time_fn(fn, reps, warmup=5):
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


def alternate(fns, reps, rounds=3):
    """median (min-max) of ``rounds`` measurements per function, the
    functions taking turns."""
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t[i].append(time_fn(fn, reps))
    return ["%.1f (%.1f-%.1f)" % (statistics.median(v), min(v), max(v))
            for v in t]


def layer_fns(B, K, N, dev):
    k = load_native("_kernels")
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, K, generator=g).bfloat16().to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    wb = w.bfloat16()
    b = torch.randn(N, generator=g).to(dev)
    gy = torch.randn(B, N, generator=g).bfloat16().to(dev)
    out = torch.empty(B, N, device=dev, dtype=torch.bfloat16)
    gx = torch.empty(B, K, device=dev, dtype=torch.bfloat16)
    gw = torch.empty(N, K, device=dev)
    gb = torch.empty(N, device=dev)
    quant = ops._fp8_quantize_gpu
    xq, xqT, sx, _ = quant(x, E4M3, want_qT=True)
    wq, wqT, sw, _ = quant(w, E4M3, want_qT=True)
    gq, gqT, sg, _ = quant(gy, E5M2, want_qT=True)
    s8 = k.linear_fp8_gw_splits(B, K, N)
    p8 = torch.empty(s8 * N * K, device=dev)
    s16 = k.linear_bf16_gw_splits(B, K, N)
    p16 = torch.empty(s16 * (N * K + N), device=dev)

    def fwd8():
        k.linear_fp8_fwd(xq.data_ptr(), wq.data_ptr(), sx.data_ptr(),
                         sw.data_ptr(), b.data_ptr(), out.data_ptr(), B, K, N,
                         True, False, st)

    def fwd8q():
        quant(x, E4M3, want_qT=True)
        quant(w, E4M3, want_qT=True)
        fwd8()

    def fwd16():
        k.linear_bf16_fwd(x.data_ptr(), wb.data_ptr(), b.data_ptr(),
                          out.data_ptr(), B, K, N, True, False, st)

    def gx8():
        k.linear_fp8_bwd_x(gq.data_ptr(), wqT.data_ptr(), sg.data_ptr(),
                           sw.data_ptr(), gx.data_ptr(), B, K, N, False, st)

    def gx8q():
        quant(gy, E5M2, mask=out)
        gx8()

    def gx16():
        k.linear_bf16_bwd_x(gy.data_ptr(), wb.data_ptr(), out.data_ptr(),
                            False, gx.data_ptr(), B, K, N, False, st)

    def gw8():
        k.linear_fp8_bwd_w(gqT.data_ptr(), xqT.data_ptr(), sg.data_ptr(),
                           sx.data_ptr(), gw.data_ptr(), p8.data_ptr(), s8,
                           B, K, N, st)

    def gw8q():
        quant(gy, E5M2, mask=out, want_q=False, want_qT=True, want_gb=True)
        gw8()

    def gw16():
        k.linear_bf16_bwd_w(gy.data_ptr(), x.data_ptr(), out.data_ptr(),
                            False, gw.data_ptr(), gb.data_ptr(),
                            p16.data_ptr(), s16, B, K, N, st)

    return [("forward", (fwd8q, fwd8, fwd16)), ("gx", (gx8q, gx8, gx16)),
            ("gw", (gw8q, gw8, gw16))]


def mx_layer_fns(B, K, N, dev):
    """per product: (tensor +q, mx +q, tensor, mx); the per-tensor entries
    are layer_fns' own"""
    k = load_native("_kernels")
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, K, generator=g).bfloat16().to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    gy = torch.randn(B, N, generator=g).bfloat16().to(dev)
    out = torch.empty(B, N, device=dev, dtype=torch.bfloat16)
    gx = torch.empty(B, K, device=dev, dtype=torch.bfloat16)
    gw = torch.empty(N, K, device=dev)
    quant = ops._mxfp8_quantize_gpu
    xq, sx, xqT, sxT, _ = quant(x, E4M3, want_qT=True)
    wq, sw, wqT, swT, _ = quant(w, E4M3, want_qT=True)
    gq, sg, gqT, sgT, _ = quant(gy, E5M2, want_qT=True)
    s8 = k.linear_fp8_gw_splits(B, K, N)
    p8 = torch.empty(s8 * N * K, device=dev)

    def fwd():
        k.linear_mxfp8_fwd(xq.data_ptr(), wq.data_ptr(), sx.data_ptr(),
                           sw.data_ptr(), b.data_ptr(), out.data_ptr(), B, K,
                           N, True, False, st)

    def fwdq():
        quant(x, E4M3, want_qT=True)
        quant(w, E4M3, want_qT=True)
        fwd()

    def gxf():
        k.linear_mxfp8_bwd_x(gq.data_ptr(), wqT.data_ptr(), sg.data_ptr(),
                             swT.data_ptr(), gx.data_ptr(), B, K, N, False, st)

    def gxq():
        quant(gy, E5M2, mask=out)
        gxf()

    def gwf():
        k.linear_mxfp8_bwd_w(gqT.data_ptr(), xqT.data_ptr(), sgT.data_ptr(),
                             sxT.data_ptr(), gw.data_ptr(), p8.data_ptr(), s8,
                             B, K, N, st)

    def gwq():
        quant(gy, E5M2, mask=out, want_q=False, want_qT=True, want_gb=True)
        gwf()

    mx = [(fwdq, fwd), (gxq, gxf), (gwq, gwf)]
    return [(name, (t[0], m[0], t[1], m[1]))
            for (name, t), m in zip(layer_fns(B, K, N, dev), mx)]


def mlp_step_fns(batch, dev, modes=((None, "tensor"),
                                    (torch.bfloat16, "tensor"),
                                    (E4M3, "tensor"))):
    fns = []
    for mode, scaling in modes:
        torch.manual_seed(0)
        model = MLP(compute_dtype=mode, fp8_scaling=scaling).to(dev)
        opt = FusedSGD(model.parameters(), lr=0.01, momentum=0.5)
        x = torch.randn(batch, 784, device=dev)
        tgt = torch.randint(0, 10, (batch,), device=dev)

        def step(model=model, opt=opt, x=x, tgt=tgt):
            opt.zero_grad()
            ops.log_softmax_nll(model.forward_logits(x), tgt).backward()
            opt.step()

        fns.append(step)
    return fns


def probe(dev):
    """Row m of A is [2^15, 127 x 2^(15-m)] in e5m2, B is all ones: what the
    instruction returns against the exact sum."""
    k = load_native("_kernels")
    st = torch.cuda.current_stream().cuda_stream
    rows = torch.stack([torch.full((128,), 2.0 ** (15 - m))
                        for m in range(1, 32)])
    rows[:, 0] = 2.0 ** 15
    aq = rows.to(E5M2).view(torch.uint8).to(dev)
    ones = torch.ones(1, 128).to(E4M3).view(torch.uint8).to(dev)
    unit = torch.ones(2, device=dev)
    c = torch.empty(31, 1, device=dev)
    k.linear_fp8_bwd_x(aq.data_ptr(), ones.data_ptr(), unit.data_ptr(),
                       unit.data_ptr(), c.data_ptr(), 31, 1, 128, True, st)
    exact = rows.double().sum(1)
    print("| m | returned | exact | small terms counted (of 127) |")
    print("|---|---|---|---|")
    for i, m in enumerate(range(1, 32)):
        got = float(c[i, 0])
        print("| %d | %r | %r | %.2f |"
              % (m, got, float(exact[i]), (got - 2.0 ** 15) / 2.0 ** (15 - m)))


def probe_mx(dev):
    """Which stored scale byte does the instruction apply to which data?
    (B, K, N) = (16, 128, 16), one instruction per fragment.  The probed
    operand's byte at (row r, block c) is 127 + 4r + c, the other operand's
    are 127; elements are 1 in one k block at a time and 0 elsewhere, so
    every result is 32 * 2^code of the byte that was applied."""
    k = load_native("_kernels")
    st = torch.cuda.current_stream().cuda_stream
    one = int(torch.ones(()).to(E4M3).view(torch.uint8))
    codes = (127 + torch.arange(64).view(16, 4)).to(torch.uint8).to(dev)
    unit = torch.full((16, 4), 127, dtype=torch.uint8, device=dev)
    ones = torch.full((16, 128), one, dtype=torch.uint8, device=dev)
    c = torch.empty(16, 16, device=dev)
    for side in ("A (x, second source)", "B (w, first source)"):
        wrong = 0
        for kb in range(4):
            data = torch.zeros(16, 128, dtype=torch.uint8, device=dev)
            data[:, 32 * kb:32 * kb + 32] = one
            a, sa, b, sb = (data, codes, ones, unit) if side[0] == "A" \
                else (ones, unit, data, codes)
            k.linear_mxfp8_fwd(a.data_ptr(), b.data_ptr(), sa.data_ptr(),
                               sb.data_ptr(), 0, c.data_ptr(), 16, 128, 16,
                               False, True, st)
            code = torch.log2(c / 32).cpu()       # [m][n]
            code = code if side[0] == "A" else code.t()
            for r in range(16):
                got = sorted(set(code[r].tolist()))
                ok = got == [4.0 * r + kb]
                wrong += not ok
                if not ok or r in (0, 5, 15):
                    print("%s: data at row %2d, k block %d scaled by the byte "
                          "stored at %s" % (side, r, kb, [
                              "(row %d, block %d)" % divmod(int(v), 4)
                              if v == int(v) and 0 <= v < 64 else repr(v)
                              for v in got]))
        print("%s: %d of 64 (row, block) pairs off the identity mapping"
              % (side, wrong))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--scaling", choices=("tensor", "mx"), default="tensor")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    load_native("_kernels")
    if args.probe:
        return probe_mx(dev) if args.scaling == "mx" else probe(dev)
    if args.scaling == "mx":
        print("| B | K | N | product | tensor +q us | mx +q us | tensor us "
              "| mx us |")
        print("|---|---|---|---|---|---|---|---|")
        for B, K, N in SHAPES:
            reps = 20 if 2.0 * B * K * N > 1e10 else 200
            for name, fns in mx_layer_fns(B, K, N, dev):
                cells = alternate(fns, reps)
                print("| %d | %d | %d | %s | %s |"
                      % (B, K, N, name, " | ".join(cells)), flush=True)
        print()
        print("| MLP 784-256-128-10 step, batch | bf16 us | fp8 tensor us "
              "| fp8 mx us |")
        print("|---|---|---|---|")
        modes = ((torch.bfloat16, "tensor"), (E4M3, "tensor"), (E4M3, "mx"))
        for batch in (128, 4096):
            cells = alternate(mlp_step_fns(batch, dev, modes), 100)
            print("| %d | %s |" % (batch, " | ".join(cells)), flush=True)
        return

    print("| B | K | N | product | fp8 +q us | fp8 us | bf16 us |")
    print("|---|---|---|---|---|---|---|")
    for B, K, N in SHAPES:
        reps = 20 if 2.0 * B * K * N > 1e10 else 200
        for name, fns in layer_fns(B, K, N, dev):
            cells = alternate(fns, reps)
            print("| %d | %d | %d | %s | %s |"
                  % (B, K, N, name, " | ".join(cells)), flush=True)
    print()
    print("| MLP 784-256-128-10 step, batch | fp32 us | bf16 us | fp8 us |")
    print("|---|---|---|---|")
    for batch in (128, 4096):
        cells = alternate(mlp_step_fns(batch, dev), 100)
        print("| %d | %s |" % (batch, " | ".join(cells)), flush=True)


if __name__ == "__main__":
    main()
