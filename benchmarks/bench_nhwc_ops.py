#!/usr/bin/env python3
"""Micro-benchmark of the channels-last batch norm and pools
(csrc/batchnorm_nhwc.hip, csrc/pool_nhwc.hip) against the NCHW kernels of
the same build (csrc/batchnorm.hip, csrc/pool.hip), at ResNet-50's shapes
for B=32 (hipEvent timing, 1 GPU).

Batch norm rows are profiles/batchnorm_numbers.md's: both dtypes, plain and
+add+ReLU, training forward and backward (gx, the residual's gradient where
there is one, dgamma, dbeta).  Pool rows are the stem max-pool and the head
average pool.  GB/s uses that document's minimum-traffic count, in tensors
of B*C*H*W elements: plain forward 3, plain backward 5, fused forward 4,
fused backward 7; a pool moves its input and its output once each (and the
max-pool one slot byte per output).

--direct times the native launchers on preallocated buffers: no allocation
and no autograd, the kernels alone.  Without it the public ops are timed,
the backward through torch.autograd.grad on a retained graph.

Every cell is measured --rounds times, the two paths alternating inside a
round, and reported as median (min-max) with the ratio of the medians.
Channels-last counts as faster where its median is below NCHW's by more than
the larger of the two min-max spreads, as slower in the mirrored case, else
as equal.

Run on a GPU box:  python benchmarks/bench_nhwc_ops.py [--direct] [--markdown]
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd import ops  # noqa: E402
from dist_tuto_pth_amd.utils.native import load_native  # noqa: E402
from bench_conv_nhwc import time_fn  # noqa: E402

CL = torch.channels_last
BN_SHAPES = [(32, 64, 112, 112), (32, 256, 56, 56), (32, 512, 28, 28),
             (32, 1024, 14, 14), (32, 2048, 7, 7)]
MAXPOOL = ((32, 64, 112, 112), 3, 2, 1)
AVGPOOL = (32, 2048, 7, 7)
PATHS = ("NCHW", "channels_last")


def _rand(shape, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(dev)


def bn_fns(shape, dtype, fused, direct, dev):
    """{path: {"fwd": fn, "bwd": fn}} and the bytes each product moves."""
    B, C, H, W = shape
    k = load_native("_kernels")
    st = torch.cuda.current_stream().cuda_stream
    es, n = torch.empty(0, dtype=dtype).element_size(), B * C * H * W
    nbytes = {"fwd": (3 + fused) * n * es,
              "bwd": (5 + 2 * fused) * n * es}
    gamma, beta = _rand((C,), torch.float32, dev, 1), \
        _rand((C,), torch.float32, dev, 2)
    out = {}
    for path in PATHS:
        nhwc = path == "channels_last"
        mf = CL if nhwc else torch.contiguous_format
        x, res, gy = (_rand(shape, dtype, dev, s).contiguous(memory_format=mf)
                      for s in (3, 4, 5))
        res = res if fused else None
        kw = dict(training=True, residual=res, fuse_relu=bool(fused),
                  memory_format=mf)
        if not direct:
            xg = x.clone(memory_format=torch.preserve_format)
            xg.requires_grad_(True)
            rg = res.clone(memory_format=torch.preserve_format)\
                .requires_grad_(True) if fused else None
            wg, bg = gamma.clone().requires_grad_(True), \
                beta.clone().requires_grad_(True)
            y = ops.batchnorm2d(xg, wg, bg, **dict(kw, residual=rg))
            wrt = (xg, wg, bg) + ((rg,) if fused else ())

            def fwd(x=x, kw=kw):
                with torch.no_grad():
                    ops.batchnorm2d(x, gamma, beta, **kw)

            out[path] = {"fwd": fwd,
                         "bwd": lambda y=y, wrt=wrt, gy=gy:
                         torch.autograd.grad(y, wrt, gy, retain_graph=True)}
            continue
        if nhwc:
            dims = (B * H * W, C)
            splits = k.batchnorm2d_nhwc_splits(*dims)
            f, b = k.batchnorm2d_nhwc_fwd, k.batchnorm2d_nhwc_bwd
        else:
            dims = (B, C, H * W)
            splits = k.batchnorm2d_splits(*dims)
            f, b = k.batchnorm2d_fwd, k.batchnorm2d_bwd
        y, gx = torch.empty_like(x), torch.empty_like(x)
        gres = torch.empty_like(x) if fused else None
        mean, inv, dg, db = (torch.empty(C, device=dev) for _ in range(4))
        ws = torch.empty(C * splits * 3, device=dev)
        bf = dtype == torch.bfloat16
        p = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731

        def fwd(f=f, x=x, res=res, y=y, mean=mean, inv=inv, ws=ws,
                splits=splits, dims=dims):
            f(x.data_ptr(), p(res), y.data_ptr(), gamma.data_ptr(),
              beta.data_ptr(), 0, 0, mean.data_ptr(), inv.data_ptr(),
              ws.data_ptr(), splits, *dims, True, 0.1, 1e-5, bool(fused), bf,
              st)

        def bwd(b=b, x=x, gy=gy, y=y, mean=mean, inv=inv, dg=dg, db=db,
                gx=gx, gres=gres, ws=ws, splits=splits, dims=dims):
            b(x.data_ptr(), gy.data_ptr(), y.data_ptr() if fused else 0,
              gamma.data_ptr(), mean.data_ptr(), inv.data_ptr(),
              dg.data_ptr(), db.data_ptr(), gx.data_ptr(), p(gres),
              ws.data_ptr(), splits, *dims, True, 1e-5, bf, st)

        fwd()   # the backward reads the saved statistics and y
        out[path] = {"fwd": fwd, "bwd": bwd}
    return out, nbytes


def pool_fns(which, dtype, dev):
    """The public ops (their launchers take no workspace, so there is
    nothing to preallocate besides the outputs)."""
    out = {}
    if which == "maxpool":
        shape, ksz, s, pad = MAXPOOL
        B, C, H, W = shape
        n_out = B * C * ((H + 2 * pad - ksz) // s + 1) ** 2
    else:
        shape = AVGPOOL
        B, C, H, W = shape
        n_out = B * C
    es, n = torch.empty(0, dtype=dtype).element_size(), B * C * H * W
    # max-pool also writes and reads one slot byte per output
    slots = n_out if which == "maxpool" else 0
    nbytes = {"fwd": (n + n_out) * es + slots, "bwd": (n + n_out) * es + slots}
    for path in PATHS:
        mf = CL if path == "channels_last" else torch.contiguous_format
        x = _rand(shape, dtype, dev, 3).contiguous(memory_format=mf)
        op = (lambda t, mf=mf: ops.maxpool2d(t, ksz, s, pad, memory_format=mf)
              ) if which == "maxpool" else \
            (lambda t, mf=mf: ops.global_avgpool2d(t, memory_format=mf))
        xg = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = op(xg)
        gy = torch.randn_like(y)

        def fwd(op=op, x=x):
            with torch.no_grad():
                op(x)

        out[path] = {"fwd": fwd,
                     "bwd": lambda y=y, xg=xg, gy=gy:
                     torch.autograd.grad(y, xg, gy, retain_graph=True)}
    return out, nbytes


def verdict(a, b):
    spread = max(max(a) - min(a), max(b) - min(b))
    ma, mb = statistics.median(a), statistics.median(b)
    return "faster" if mb < ma - spread else \
        "SLOWER" if mb > ma + spread else "equal"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--direct", action="store_true",
                    help="batch norm: time the native launchers on "
                         "preallocated buffers")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nhwc_ops needs a GPU"
    dev = torch.device("cuda:0")
    load_native("_kernels")

    cases = []
    for dtype in (torch.bfloat16, torch.float32):
        name = "bf16" if dtype == torch.bfloat16 else "fp32"
        for shape in BN_SHAPES:
            for fused in (0, 1):
                desc = (f"bn {name} {'x'.join(map(str, shape))}"
                        + (" +add+ReLU" if fused else ""))
                cases.append((desc, lambda s=shape, d=dtype, f=fused:
                              bn_fns(s, d, f, args.direct, dev)))
        for which in ("maxpool", "avgpool"):
            shape = MAXPOOL[0] if which == "maxpool" else AVGPOOL
            cases.append((f"{which} {name} {'x'.join(map(str, shape))}",
                          lambda w=which, d=dtype: pool_fns(w, d, dev)))

    def cell(v):
        return f"{statistics.median(v):.1f} ({min(v):.1f}-{max(v):.1f})"

    if args.markdown:
        print("| case | product | NCHW us | channels_last us | ratio | "
              "NCHW GB/s | channels_last GB/s | channels_last is |")
        print("|---" * 8 + "|")
    for desc, make in cases:
        print(f"timing {desc}", file=sys.stderr, flush=True)
        fns, nbytes = make()
        for prod in ("fwd", "bwd"):
            t = {p: [] for p in PATHS}
            for _ in range(args.rounds):
                for p in PATHS:     # the paths alternate inside a round
                    t[p].append(time_fn(fns[p][prod], args.reps, args.warmup))
            a, b = t["NCHW"], t["channels_last"]
            ma, mb = statistics.median(a), statistics.median(b)
            gbs = [f"{nbytes[prod] / m / 1e3:.0f}" for m in (ma, mb)]
            cols = [desc, prod, cell(a), cell(b), f"{mb / ma:.2f}", *gbs,
                    verdict(a, b)]
            print("| " + " | ".join(cols) + " |" if args.markdown
                  else "  ".join(cols), flush=True)
        del fns
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
