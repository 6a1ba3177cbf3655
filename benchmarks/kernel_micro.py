#!/usr/bin/env python3
"""Per-kernel microbenchmark of the fused ConvNet training step
(hipEvent timing, 1 GPU).  Pinpoints where the step's microseconds go:
fwd (with its prologue, and alone: both kernels with one and two
workgroups per sample), data-bwd (bundled with gw, and alone: both
kernels at each sibling-split), the four weight-gradient tile
segments separately, combine, sgd, prologue.

Run on a GPU box:  python benchmarks/kernel_micro.py [--batch 128]
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd.models import Net  # noqa: E402
from dist_tuto_pth_amd.optim import FusedSGD  # noqa: E402
from dist_tuto_pth_amd.ops import _seed_ptr, _stream  # noqa: E402
from dist_tuto_pth_amd.ops.fused import (_params, _ptrs, _ws,  # noqa: E402
                                         attach_flat_grads)
from dist_tuto_pth_amd.utils.native import load_native  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = args.batch

    k = load_native("_kernels")
    net = Net().to(dev)
    net.train()
    ws = _ws(B, dev)
    flat = attach_flat_grads(net)  # noqa: F841 (keeps the grads alive)
    opt = FusedSGD(net.parameters(), lr=0.01, momentum=0.5,
                   zero_grad_in_step=True)
    x = torch.randn(B, 1, 28, 28, device=dev)
    tgt = torch.randint(0, 10, (B,), device=dev)
    params = _params(net)
    pp = _ptrs(params)
    gp = _ptrs(p.grad for p in params)
    s = _stream()

    def fwd():
        k.net_fused_fwd(x.data_ptr(), pp, tgt.data_ptr(), ws.ptrs, False,
                        _seed_ptr(dev), B, True, s)

    def bwd():
        k.net_fused_bwd(x.data_ptr(), pp[2], pp[4], pp[6], tgt.data_ptr(),
                        ws["one"].data_ptr(), ws.ptrs, gp, [], [], 0.0, 0.0,
                        B, True, False, 0, s)

    fwd()
    bwd()
    torch.cuda.synchronize()

    # raw segment launches use the chunk plan the fused step runs
    pl = k.gw_plan(B)
    chunks = (pl["nch"], pl["nch1"], pl["nch2"])

    def seg(base, ntiles):
        def f():
            k.net_gw_partial_raw(
                x.data_ptr(), ws["p1"].data_ptr(), ws["p2"].data_ptr(),
                ws["d3"].data_ptr(), ws["ga1"].data_ptr(),
                ws["ga2"].data_ptr(), ws["gh1"].data_ptr(),
                ws["glog"].data_ptr(), ws["part"].data_ptr(), B,
                pl["bchunk"], pl["bchunk1"], pl["bchunk2"], base, ntiles,
                *chunks, s)
        return f

    results = {}
    results["fwd"] = time_fn(fwd)

    # the forward alone (loss_part mode, no prologue dispatch): the tiled
    # kernel and the 256-thread one, one and two workgroups per sample
    def fwd_raw(tiled, split):
        return lambda: k.net_fwd_raw(
            x.data_ptr(), pp, tgt.data_ptr(), ws.ptrs, _seed_ptr(dev), B,
            True, tiled, split, 60000, s)

    for tiled in (True, False):
        for sp in (1, 2):
            if sp == 2 and B > 2048:
                continue
            name = "tiled" if tiled else "old"
            results[f"fwd {name} (split={sp})"] = time_fn(fwd_raw(tiled, sp))
    # full bwd+gw+combine bundle is what bwd() launches; time the pieces
    for sp in (1, 2, 4, 8):
        os.environ["DTP_BWD_SPLIT"] = str(sp)
        results[f"bwd+gw (split={sp})"] = time_fn(bwd)
    os.environ.pop("DTP_BWD_SPLIT", None)

    # the data backward alone, both kernels (DTP_BWD_TILED=0: the
    # 256-thread strip loop) at each sibling split; "auto" is the default
    def bwd_data():
        k.net_bwd_data_raw(pp[2], pp[4], pp[6], tgt.data_ptr(),
                           ws["one"].data_ptr(), ws.ptrs, B, True, s)

    for tiled in (1, 0):
        os.environ["DTP_BWD_TILED"] = str(tiled)
        for sp in ("auto", 1, 2, 4, 8):
            if sp == "auto":
                os.environ.pop("DTP_BWD_SPLIT", None)
            else:
                os.environ["DTP_BWD_SPLIT"] = str(sp)
            name = "tiled" if tiled else "strip"
            results[f"bwd data {name} (split={sp})"] = time_fn(bwd_data)
    os.environ.pop("DTP_BWD_SPLIT", None)
    os.environ.pop("DTP_BWD_TILED", None)
    base = 0
    for name, ntiles in k.gw_tiles:  # walk order of the partial kernel
        results[f"gw {name} tiles"] = time_fn(seg(base, ntiles))
        base += ntiles
    results["gw all tiles"] = time_fn(seg(0, base))
    results["gw combine"] = time_fn(lambda: k.net_gw_combine_raw(
        ws["part"].data_ptr(), gp, *chunks, s))
    results["gw combine+sgd+loss"] = time_fn(
        lambda: k.net_gw_combine_sgd_raw(
            ws["part"].data_ptr(), gp, pp, _ptrs(opt._bufs), *chunks, 0.01,
            0.5, ws["loss_part"].data_ptr(), ws["loss"].data_ptr(), 128, s))
    results["sgd"] = time_fn(opt.step)

    for name, us in results.items():
        print(f"{name:24s} {us:8.2f} us")


if __name__ == "__main__":
    main()
