"""The head of Net's data backward run by the tiled forward (the step
paths' default) against the head run by the backward (DTP_HEAD_IN_FWD=0,
and always the autograd path).

Batches: 3 (bwd split 8, odd grid), 64 (split 4) and 128 (split 2), all
three on the split forward; 130 (split 2) and 256 (split 1) on the unsplit
forward.  Eval and train.

The forward's head uses the backward head's expressions and summation
orders on the same fp32 values, so the two paths must agree bit for bit:
every comparison of the two here is torch.equal.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.models import Net
from dist_tuto_pth_amd.ops import fused
from dist_tuto_pth_amd.utils.native import load_native

DEV = torch.device("cuda:0")
BATCHES = [3, 64, 128, 130, 256]
SEED = 424242           # the dropout seed every step here starts from
WS_READ = ("idx2", "glog", "gh1", "ga2", "ga1")

# What the child processes and this one run: the inputs of one (batch,
# mode) and one net_fused_step from the fixed seed, read back to the CPU.
_COMMON = r"""
import torch
from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.models import Net
from dist_tuto_pth_amd.ops import fused
from dist_tuto_pth_amd.utils.native import load_native
DEV = torch.device("cuda:0")
SEED = %d
WS_READ = %r


def mk(B):
    g = torch.Generator().manual_seed(7717 + B)
    net = Net()
    with torch.no_grad():
        for p in net.parameters():      # biases away from zero as well
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    x = torch.randn(B, 1, 28, 28, generator=g)
    tgt = torch.randint(0, 10, (B,), generator=g)
    return net.to(DEV), x.to(DEV), tgt.to(DEV)


def set_seed():
    ops._seed_ptr(DEV)      # creates it
    ops._seed_bufs[DEV.index].fill_(SEED)


def one_step(B, training):
    net, x, tgt = mk(B)
    net.train(training)
    set_seed()
    ws = fused._ws(B, DEV)
    for n in ("glog", "gh1", "ga2", "ga1"):     # nothing may be left over
        ws[n].fill_(float("nan"))
    loss = fused.net_fused_step(net, x, tgt).clone()
    torch.cuda.synchronize()
    out = {n: ws[n].cpu().clone() for n in WS_READ}
    out["loss"] = loss.cpu()
    out["grads"] = [p.grad.cpu().clone() for p in net.parameters()]
    # what a step's forward answers when it is given the loss gradient
    # (a forward alone leaves the seed where it is)
    out["head_in_fwd"] = load_native("_kernels").net_fused_fwd(
        x.data_ptr(), fused._ptrs(fused._params(net)), tgt.data_ptr(),
        ws.ptrs, True, ops._seed_ptr(DEV), B, training, ops._stream(),
        ws["one"].data_ptr())
    torch.cuda.synchronize()
    return out
""" % (SEED, WS_READ)
exec(_COMMON)       # mk, set_seed, one_step

_CHILD = _COMMON + r"""
import sys
out = {}
for B in %r:
    for training in (False, True):
        out[(B, training)] = one_step(B, training)
torch.save(out, sys.argv[1])
""" % (BATCHES,)


def _both_paths(tmp):
    """Every (batch, mode) once with the head in the backward ("0") and
    once with the default ("default"), each in a fresh process: the
    variable is read on every call, the processes are fresh so that both
    start from the same state."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for v in ("0", "default"):
        path = os.path.join(tmp, f"head{v}.pt")
        env = dict(os.environ)
        env.pop("DTP_HEAD_IN_FWD", None)
        if v == "0":
            env["DTP_HEAD_IN_FWD"] = "0"
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env,
                           capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr[-2000:]
        got[v] = torch.load(path)
    return got


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    return _both_paths(str(tmp_path_factory.mktemp("head_in_fwd")))


def test_the_default_step_runs_the_head_in_the_forward(both):
    """Both tiled kernels are the default at every batch here, so the
    default forward answers that it ran the head, and with
    DTP_HEAD_IN_FWD=0 that it did not."""
    assert sorted(both["default"]) == sorted(
        (B, t) for B in BATCHES for t in (False, True))
    for key in both["default"]:
        assert both["default"][key]["head_in_fwd"] is True, key
        assert both["0"][key]["head_in_fwd"] is False, key


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_head_in_forward_equals_head_in_backward(both, B, training):
    """glog, gh1, ga2, ga1, the loss and all 8 gradients, bit for bit."""
    new, old = both["default"][(B, training)], both["0"][(B, training)]
    diffs = []
    for n in WS_READ + ("loss",):
        a, b = new[n], old[n]
        assert bool(torch.isfinite(a.float()).all()), n
        worst = (a.double() - b.double()).abs().max().item()
        print(f"{n} [{a.numel()}]: worst |new - old| = {worst:.3e}")
        if not torch.equal(a, b):
            diffs.append((n, a.numel(), worst))
    assert len(new["grads"]) == 8
    for i, (a, b) in enumerate(zip(new["grads"], old["grads"])):
        worst = (a - b).abs().max().item()
        print(f"grad {i} [{a.numel()}]: worst |new - old| = {worst:.3e}")
        if not torch.equal(a, b):
            diffs.append((f"grad {i}", a.numel(), worst))
    assert not diffs, f"first array that differs: {diffs[0]}; all: {diffs}"


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", [3, 64])
def test_forced_fallback_gives_the_same_head(B, training):
    """Split 2 with poll bound 0: sibling 0 never sees its sibling's token,
    computes that half of conv2 and its index bytes itself and runs the
    head from those.  Same values by construction."""
    k = load_native("_kernels")
    net, x, tgt = mk(B)                         # noqa: F821
    net.train(training)
    ws = fused._ws(B, DEV)
    prm = fused._ptrs(fused._params(net))
    names = ("glog", "gh1", "ga2", "idx2")
    got = {}
    for poll in (60000, 0):
        set_seed()                              # noqa: F821
        for n in names[:3]:
            ws[n].fill_(float("nan"))
        ws["idx2"].fill_(255)
        k.net_fwd_raw(x.data_ptr(), prm, tgt.data_ptr(), ws.ptrs,
                      ops._seed_ptr(DEV), B, training, True, 2, poll,
                      ops._stream(), gl=ws["one"].data_ptr())
        torch.cuda.synchronize()
        got[poll] = {n: ws[n].cpu().clone() for n in names}
    for n in names:
        assert bool(torch.isfinite(got[0][n].float()).all()), n
        assert torch.equal(got[0][n], got[60000][n]), n
    assert int(got[0]["idx2"].max()) < 8
    assert float(got[0]["ga2"].abs().sum()) > 0


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_ga2_is_fully_written_and_routed_by_idx2(B, training):
    """ga2 starts as NaN (one_step fills it).  Afterwards no NaN, at most
    one non-zero per 2x2 pooling window, and that one in the slot the
    forward's index byte names (none where the ReLU was dead)."""
    s = one_step(B, training)                   # noqa: F821
    ga2 = s["ga2"].view(B, 20, 4, 2, 4, 2)      # [b, k, ph, a, pw, c]
    assert not bool(torch.isnan(ga2).any())
    win = ga2.permute(0, 1, 2, 4, 3, 5).reshape(B, 20, 4, 4, 4)  # slot 2a+c
    nz = win != 0
    assert int(nz.sum(dim=-1).max()) <= 1
    idx2 = s["idx2"].view(B, 20, 4, 4).long()
    live = (idx2 & 4) == 0
    slot = torch.nn.functional.one_hot(idx2 & 3, 4).bool()
    allowed = slot & live.unsqueeze(-1)
    assert not bool((nz & ~allowed).any())
    assert bool(nz.any())


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", [3, 128])
def test_autograd_path_takes_an_upstream_gradient(B, training):
    """net_fused_loss cannot know its upstream gradient in the forward, so
    its backward runs the head: glog / gh1 / ga2 are NaN when it starts
    and the gradients of (3 * loss) are 3x those of loss."""
    net, x, tgt = mk(B)                         # noqa: F821
    net.train(training)
    ws = fused._ws(B, DEV)
    grads = {}
    for up in (1.0, 3.0):
        set_seed()                              # noqa: F821
        for p in net.parameters():
            p.grad = None
        loss = fused.net_fused_loss(net, x, tgt)
        for n in ("glog", "gh1", "ga2"):
            ws[n].fill_(float("nan"))
        (up * loss).backward()
        torch.cuda.synchronize()
        for n in ("glog", "gh1", "ga2"):
            assert bool(torch.isfinite(ws[n]).all()), n
        grads[up] = [p.grad.cpu().clone() for p in net.parameters()]
    top = max(float(g.abs().max()) for g in grads[3.0])
    assert top > 0
    for i, (g1, g3) in enumerate(zip(grads[1.0], grads[3.0])):
        worst = float((g3 - 3.0 * g1).abs().max())
        print(f"grad {i}: worst |g(3 loss) - 3 g(loss)| / top = "
              f"{worst / top:.3e}")
        assert worst <= 1e-6 * top, (i, worst, top)
