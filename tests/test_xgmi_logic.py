"""Fake-comm unit tests for the hand-tuned xGMI all-reduce algorithms
(VERDICT r1 next-round #2).

``algorithms.xgmi.fullmesh_all_reduce`` / ``ring_all_reduce`` are pure
functions of an injected ``comm`` (RCCL grouped-p2p surface) and
``kern`` (reduction kernels on raw pointers).  Here a pure-Python
fabric of per-pair queues plus ctypes/numpy kernels drives the EXACT
production code — same chunk/offset math, same padding, same pipeline
schedule — at worlds 2-8, fp32+bf16, divisible/non-divisible sizes and
pipeline depths 1..5, asserting exact sums against a torch reference.
The only untested part left is the wire (RCCL) and the device (HIP),
covered by tests/test_rccl_gpu.py on the GPU box.
"""

import ctypes
import os
import queue
import sys
import threading

import numpy as np
import pytest
import torch

from dist_tuto_pth_amd.algorithms.xgmi import (_sub_splits,
                                               fullmesh_all_reduce,
                                               ring_all_reduce)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_bounds as fb  # noqa: E402

# ---------------------------------------------------------------------------
# fakes
# ---------------------------------------------------------------------------

_ESZ = {7: 4, 9: 2}


class Fabric:
    def __init__(self, size):
        self.queues = {(s, d): queue.Queue()
                       for s in range(size) for d in range(size)}


class FakeComm:
    """Implements the native Comm's grouped p2p surface over in-memory
    queues.  Sends snapshot bytes at group_end; recvs block (so a
    mismatched schedule across ranks times out instead of hanging)."""

    def __init__(self, fabric: Fabric, rank: int):
        self.fabric = fabric
        self.rank = rank
        self.ops = None
        self.trace = []          # for schedule assertions

    def group_start(self):
        assert self.ops is None, "nested group"
        self.ops = []
        self.trace.append("gs")

    def group_end(self):
        sends = [o for o in self.ops if o[0] == "s"]
        recvs = [o for o in self.ops if o[0] == "r"]
        self.ops = None
        self.trace.append("ge")
        for _, ptr, nbytes, peer in sends:
            self.fabric.queues[(self.rank, peer)].put(
                ctypes.string_at(ptr, nbytes))
        for _, ptr, nbytes, peer in recvs:
            data = self.fabric.queues[(peer, self.rank)].get(timeout=20)
            assert len(data) == nbytes, \
                f"rank {self.rank}: recv {nbytes}B from {peer}, " \
                f"got {len(data)}B"
            ctypes.memmove(ptr, data, nbytes)

    def send(self, ptr, count, dt, peer, stream):
        nbytes = count * _ESZ[dt]
        self.trace.append(("s", peer, count))
        if self.ops is None:
            self.fabric.queues[(self.rank, peer)].put(
                ctypes.string_at(ptr, nbytes))
        else:
            self.ops.append(("s", ptr, nbytes, peer))

    def recv(self, ptr, count, dt, peer, stream):
        nbytes = count * _ESZ[dt]
        self.trace.append(("r", peer, count))
        if self.ops is None:
            data = self.fabric.queues[(peer, self.rank)].get(timeout=20)
            ctypes.memmove(ptr, data, nbytes)
        else:
            self.ops.append(("r", ptr, nbytes, peer))


def _f32(ptr, n):
    return np.ctypeslib.as_array(
        ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), shape=(n,))


def _u16(ptr, n):
    return np.ctypeslib.as_array(
        ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint16)), shape=(n,))


def _tensor(ptr, n, dt):
    """The ``n`` elements at ``ptr`` as a torch tensor sharing the memory."""
    if dt == 7:
        return torch.from_numpy(_f32(ptr, n))
    if dt == 9:
        return torch.from_numpy(_u16(ptr, n)).view(torch.bfloat16)
    raise ValueError(dt)


class FakeKernels:
    """The reduction kernels' CONTRACT (csrc/kernels.hip) on raw host
    pointers: reduce_columns accumulates fp32 and rounds once; add_inplace
    is an elementwise add.  The arithmetic is tests/fp32_bounds.py's
    contract model, the one tests/test_fp32_kernels_gpu.py holds the real
    kernels to, bit for bit."""

    def reduce_columns(self, dst, src, P, stride, n, scale, dt, stream):
        s = _tensor(src, (P - 1) * stride + n, dt) if P > 0 else None
        fb.reduce_columns_model(_tensor(dst, n, dt), s, P, stride, n, scale)

    def add_inplace(self, dst, src, n, dt, stream):
        fb.add_inplace_model(_tensor(dst, n, dt), _tensor(src, n, dt), n)

    def scale_f32(self, dst, scale, n, stream):
        fb.scale_f32_model(_tensor(dst, n, 7), scale, n)


def _per_rank_buf():
    cache = {}

    def buf(key, numel, dtype, device):
        t = cache.get(key)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.empty(numel, dtype=dtype, device=device)
            cache[key] = t
        return t
    return buf


def _run_world(size, fn):
    """Run ``fn(rank, comm)`` on one thread per rank; re-raise the
    first failure."""
    fabric = Fabric(size)
    comms = [FakeComm(fabric, r) for r in range(size)]
    errs = [None] * size

    def worker(r):
        try:
            fn(r, comms[r])
        except BaseException as e:  # noqa: BLE001
            errs[r] = e

    threads = [threading.Thread(target=worker, args=(r,), daemon=True)
               for r in range(size)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
        assert not t.is_alive(), "rank thread hung (schedule deadlock?)"
    for e in errs:
        if e is not None:
            raise e
    return comms


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("size", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("numel", [64, 1000, 4096, 12345])
@pytest.mark.parametrize("depth", [1, 4])
def test_fullmesh_worlds_fp32(size, numel, depth):
    torch.manual_seed(size * 1000 + numel)
    inputs = [torch.randn(numel) for _ in range(size)]
    expect = torch.stack(inputs).sum(0)
    outs = [t.clone() for t in inputs]
    kern = FakeKernels()

    def fn(r, comm):
        fullmesh_all_reduce(outs[r], comm, kern, r, size, depth=depth,
                            buf=_per_rank_buf())

    _run_world(size, fn)
    for r in range(size):
        torch.testing.assert_close(outs[r], expect, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("size", [2, 6, 8])
@pytest.mark.parametrize("numel", [1000, 8192])
@pytest.mark.parametrize("depth", [2, 3, 5])
def test_fullmesh_depths(size, numel, depth):
    torch.manual_seed(7)
    inputs = [torch.randn(numel) for _ in range(size)]
    expect = torch.stack(inputs).sum(0)
    outs = [t.clone() for t in inputs]
    kern = FakeKernels()

    def fn(r, comm):
        fullmesh_all_reduce(outs[r], comm, kern, r, size, depth=depth,
                            buf=_per_rank_buf())

    _run_world(size, fn)
    for r in range(size):
        torch.testing.assert_close(outs[r], expect, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("size", [2, 4, 8])
@pytest.mark.parametrize("numel", [1024, 999])
@pytest.mark.parametrize("depth", [1, 4])
def test_fullmesh_bf16(size, numel, depth):
    torch.manual_seed(42)
    inputs = [torch.randn(numel).bfloat16() for _ in range(size)]
    # the bf16 contract: accumulate fp32, round ONCE at the owner —
    # so the expected value is the fp32 sum rounded to bf16
    expect = torch.stack([t.float() for t in inputs]).sum(0).bfloat16()
    outs = [t.clone() for t in inputs]
    kern = FakeKernels()

    def fn(r, comm):
        fullmesh_all_reduce(outs[r], comm, kern, r, size, depth=depth,
                            buf=_per_rank_buf())

    _run_world(size, fn)
    for r in range(size):
        torch.testing.assert_close(outs[r].float(), expect.float(),
                                   rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("size", [3, 8])
@pytest.mark.parametrize("numel", [1000, 4096])
def test_fullmesh_average(size, numel):
    torch.manual_seed(3)
    inputs = [torch.randn(numel) for _ in range(size)]
    expect = torch.stack(inputs).mean(0)
    outs = [t.clone() for t in inputs]
    kern = FakeKernels()

    def fn(r, comm):
        fullmesh_all_reduce(outs[r], comm, kern, r, size, average=True,
                            depth=3, buf=_per_rank_buf())

    _run_world(size, fn)
    for r in range(size):
        torch.testing.assert_close(outs[r], expect, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("size", [2, 3, 5, 8])
@pytest.mark.parametrize("numel", [64, 1000, 12345])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ring_worlds(size, numel, dtype):
    torch.manual_seed(size + numel)
    inputs = [torch.randn(numel).to(dtype) for _ in range(size)]
    expect = torch.stack([t.float() for t in inputs]).sum(0)
    outs = [t.clone() for t in inputs]
    kern = FakeKernels()

    def fn(r, comm):
        ring_all_reduce(outs[r], comm, kern, r, size,
                        buf=_per_rank_buf())

    _run_world(size, fn)
    tol = 1e-5 if dtype == torch.float32 else 0.15
    for r in range(size):
        torch.testing.assert_close(outs[r].float(), expect, rtol=tol,
                                   atol=tol)


def test_fullmesh_schedule_is_grouped_and_identical():
    """Every transfer sits inside a group, and the global group order
    (X_0..X_{D-1}, G_0..G_{D-1}) is IDENTICAL on every rank — the
    property that makes RCCL's grouped matching deadlock-free."""
    size, numel, depth = 4, 4096, 4
    outs = [torch.randn(numel) for _ in range(size)]
    kern = FakeKernels()

    def fn(r, comm):
        fullmesh_all_reduce(outs[r], comm, kern, r, size, depth=depth,
                            buf=_per_rank_buf())

    comms = _run_world(size, fn)
    for c in comms:
        depth_groups = 0
        in_group = False
        for ev in c.trace:
            if ev == "gs":
                assert not in_group
                in_group = True
                depth_groups += 1
            elif ev == "ge":
                in_group = False
            else:
                assert in_group, f"bare p2p op outside a group: {ev}"
        assert depth_groups == 2 * depth
    # group "shapes" (sorted peer/count multiset per group) must agree
    # across ranks after normalizing peers out — compare counts only
    def shapes(c):
        out, cur = [], None
        for ev in c.trace:
            if ev == "gs":
                cur = []
            elif ev == "ge":
                out.append(tuple(sorted(n for _, _, n in cur)))
                cur = None
            else:
                cur.append(ev)
        return out
    s0 = shapes(comms[0])
    for c in comms[1:]:
        assert shapes(c) == s0


def test_sub_splits():
    assert _sub_splits(100, 1, 4) == [(0, 100)]
    s = _sub_splits(100, 4, 4)
    assert sum(c for _, c in s) == 100
    assert all(o % 4 == 0 for o, _ in s)
    # all but last equal-sized
    sizes = [c for _, c in s]
    assert len(set(sizes[:-1])) <= 1
    # degenerate: chunk smaller than alignment
    assert _sub_splits(3, 8, 4) == [(0, 3)]


def test_rccl_sendrecv_posts_one_group(monkeypatch):
    """Regression for the r1 un-grouped-p2p deadlock: the rccl
    backend's paired exchange must post send+recv inside ONE
    group_start/group_end."""
    from dist_tuto_pth_amd.dist import rccl_backend as rb

    calls = []

    class RecComm:
        def group_start(self):
            calls.append("gs")

        def group_end(self):
            calls.append("ge")

        def send(self, *a):
            calls.append("send")

        def recv(self, *a):
            calls.append("recv")

    class FakeT:
        is_cuda = True
        dtype = torch.float32

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 0

        def numel(self):
            return 8

    class FakeStream:
        cuda_stream = 0

        def synchronize(self):
            pass

    monkeypatch.setattr(rb.torch.cuda, "current_stream",
                        lambda *a, **k: FakeStream())
    b = rb._RcclBackend.__new__(rb._RcclBackend)
    b._comm = RecComm()
    b.sendrecv(FakeT(), 1, FakeT(), 0)
    assert calls == ["gs", "send", "recv", "ge"]
