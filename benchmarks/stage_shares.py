#!/usr/bin/env python3
"""Where the fused forward and data-backward workgroups spend their time:
per-stage SHARES from the in-kernel shader-clock stamps of the diagnostic
build (python build.py --stage-stamps -> _native/_kernels_stamps.so).

The stamped kernels are slower than the default build's, so only the
shares are meaningful, not the cycle counts.  Stamp indices and stage
names are listed beside STAGE_STAMP in csrc/net_fused.hip.

Run on a GPU box:  python benchmarks/stage_shares.py [--batch 128]
"""

import argparse
import importlib.util
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dist_tuto_pth_amd.utils import native  # noqa: E402

BWD = ["w2 staging", "g_logits", "g_h1", "g_p2 (wf1)", "tile zero+scatter",
       "ga2 stash", "conv2 bwd_x FMAs", "k-group sum + pool1 bwd"]
FWD = ["staging", "conv1+pool1", "conv2+pool2", "sibling hand-off", "fc1",
       "fc2+softmax"]


def load_stamped():
    """Put the stamped build where load_native("_kernels") finds it."""
    path = native.native_path("_kernels_stamps")
    if not os.path.exists(path):
        sys.exit(f"{path} not built: run `python build.py --stage-stamps`")
    spec = importlib.util.spec_from_file_location("_kernels", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["_kernels"] = mod
    spec.loader.exec_module(mod)
    native._cache["_kernels"] = mod
    return mod


def shares(st, lo, names, title):
    """st: [blocks, NSTAMP] int64; stages are consecutive stamps from lo.
    Only workgroups that passed every boundary count (a forward sibling 1
    leaves after the hand-off; the strip kernel has no stamp 7)."""
    hi = lo + len(names)
    cols = st[:, lo:hi + 1]
    full = (cols != 0).all(dim=1)
    if not bool(full.any()):      # the strip loop: fold stamps 7 into 8
        keep = [i for i in range(lo, hi + 1) if i != 7]
        cols, names = st[:, keep], names[:-2] + ["conv2 bwd_x + pool1 bwd"]
        full = (cols != 0).all(dim=1)
    d = (cols[full][:, 1:] - cols[full][:, :-1]).double()
    tot = d.sum(dim=1, keepdim=True)
    sh = (d / tot).mean(dim=0) * 100.0
    print(f"{title}  ({int(full.sum())} workgroups, median "
          f"{int(tot.median())} clocks stamped)")
    for n, v in zip(names, sh.tolist()):
        print(f"  {n:28s} {v:5.1f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available()
    k = load_stamped()
    from dist_tuto_pth_amd.models import Net
    from dist_tuto_pth_amd.ops.fused import net_fused_step
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = args.batch
    net = Net().to(dev).train()
    x = torch.randn(B, 1, 28, 28, device=dev)
    tgt = torch.randint(0, 10, (B,), device=dev)
    n = k.STAGE_NSTAMP
    for tiled in ("1", "0"):
        os.environ["DTP_BWD_TILED"] = tiled
        for _ in range(20):
            net_fused_step(net, x, tgt)
        k.stage_stamps_clear()
        net_fused_step(net, x, tgt)
        st = torch.tensor(k.stage_stamps(), dtype=torch.int64).view(-1, n)
        shares(st, 0, BWD, f"data backward, B={B}, "
               + ("tiled kernel" if tiled == "1" else "strip kernel"))
    os.environ.pop("DTP_BWD_TILED", None)
    for tiled in ("1", "0"):
        os.environ["DTP_FWD_TILED"] = tiled
        for _ in range(20):
            net_fused_step(net, x, tgt)
        k.stage_stamps_clear()
        net_fused_step(net, x, tgt)
        st = torch.tensor(k.stage_stamps(), dtype=torch.int64).view(-1, n)
        shares(st, 9, FWD, f"forward, B={B}, "
               + ("tiled kernel" if tiled == "1" else "256-thread kernel"))
    os.environ.pop("DTP_FWD_TILED", None)


if __name__ == "__main__":
    main()
