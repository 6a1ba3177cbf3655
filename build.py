#!/usr/bin/env python3
"""Build every native extension in-tree for gfx950 (MI355X).

Outputs land in ``dist_tuto_pth_amd/_native/*.so`` so they travel with
the repo snapshot to GPU machines.  hipcc cross-compiles without a GPU.
"""

import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "dist_tuto_pth_amd", "csrc")
OUT = os.path.join(ROOT, "dist_tuto_pth_amd", "_native")

ARCH = os.environ.get("DTP_AMD_ARCH", "gfx950")


def _includes():
    import pybind11
    import sysconfig
    return [
        pybind11.get_include(),
        sysconfig.get_paths()["include"],
        "/opt/rocm/include",
    ]


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def _needs_build(out, srcs):
    if not os.path.exists(out):
        return True
    ot = os.path.getmtime(out)
    return any(os.path.getmtime(s) > ot for s in srcs)


def build(force: bool = False, stage_stamps: bool = False):
    """Build the extensions.  ``stage_stamps`` builds, instead, the
    diagnostic ``_kernels_stamps.so`` (net_fused.hip's DTP_STAGE_STAMPS:
    shader-clock stamps at the stage boundaries of the fused forward and
    data backward) next to the default ``_kernels.so``, which it leaves
    alone; only benchmarks/stage_shares.py loads it."""
    os.makedirs(OUT, exist_ok=True)
    inc = sum([["-I", p] for p in _includes()], [])
    common = ["hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17",
              "-fPIC", "-shared", "-fvisibility=hidden"] + inc

    src = lambda *names: [os.path.join(CSRC, n) for n in names]  # noqa: E731
    targets = [
        # (output, sources, headers, extra flags)
        ("_rcclx.so", src("rcclx.cpp"), [], ["-L/opt/rocm/lib", "-lrccl"]),
        ("_kernels.so", src("kernels.hip", "pointwise.hip", "net_fused.hip",
                            "linear_bf16.hip", "conv_bf16.hip",
                            "batchnorm.hip", "pool.hip",
                            "cross_entropy.hip"),
         src("common.h", "gemm_bf16.h"), []),
    ]
    if stage_stamps:
        targets = [("_kernels_stamps.so", targets[1][1], targets[1][2],
                    ["-DDTP_STAGE_STAMPS"])]
    for out_name, srcs, hdrs, extra in targets:
        out = os.path.join(OUT, out_name)
        if force or _needs_build(out, srcs + hdrs):
            _run(common + srcs + extra + ["-o", out])
        else:
            print(f"{out_name}: up to date")


if __name__ == "__main__":
    build(force="--force" in sys.argv,
          stage_stamps="--stage-stamps" in sys.argv)
