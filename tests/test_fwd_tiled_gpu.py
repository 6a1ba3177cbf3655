"""The re-blocked forward of the fused Net step (net_fused_fwd_tiled_kernel),
stage by stage against float64 references computed from the GPU's OWN
previous stage (read back from the workspace), then against the
net_fwd_sample kernels (DTP_FWD_TILED=0, a fresh child process), the forced
hand-off fallback and the legacy loss mode.

Batches: 3 (tiny, odd), 64 and 128 (sibling split), 130 (first unsplit
batch), 256.  One step per (batch, mode) is run once and shared.

Bounds are the project's rule (tests/fp32_bounds.py): an fp32 sum of L terms
is within 2*L*u*sum|terms|.  A 2x2 max and a ReLU are 1-Lipschitz, so a
pooled value obeys the largest bound of its window whichever slot won.
"""

import functools
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fp32_bounds import T, U, within

from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.models import Net
from dist_tuto_pth_amd.ops import fused
from dist_tuto_pth_amd.utils.native import load_native

DEV = torch.device("cuda:0")
BATCHES = [3, 64, 128, 130, 256]
SEED = 12345            # the dropout seed every step here starts from
WS_READ = ("p1", "idx1", "m2", "p2", "idx2", "h1", "m3", "d3", "logp",
           "glog", "gh1", "ga2", "ga1")
GRAD_ATOL, LOSS_ATOL = 2e-4, 1e-5       # the fused tests' tolerances

# What both processes run: the inputs of one (batch, mode) and one
# net_fused_step from the fixed seed, everything read back to the CPU.
_COMMON = r"""
import torch
from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.models import Net
from dist_tuto_pth_amd.ops import fused
DEV = torch.device("cuda:0")
SEED = %d
WS_READ = %r


def mk(B):
    g = torch.Generator().manual_seed(4021 + B)
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
    loss = fused.net_fused_step(net, x, tgt).clone()
    torch.cuda.synchronize()
    ws = fused._ws(B, DEV)
    out = {n: ws[n].cpu().clone() for n in WS_READ}
    out["loss"] = loss.cpu()
    out["grads"] = [p.grad.cpu().clone() for p in net.parameters()]
    return out, net, x, tgt
""" % (SEED, WS_READ)
exec(_COMMON)       # mk, set_seed, one_step

_OLD_PROG = _COMMON + r"""
import sys
out = {}
for B in %r:
    for training in (False, True):
        out[(B, training)] = one_step(B, training)[0]
torch.save(out, sys.argv[1])
""" % (BATCHES,)


@functools.lru_cache(maxsize=None)
def _step(B, training):
    """One net_fused_step on the default (tiled) forward, and what the
    legacy autograd path gives from the same seed."""
    out, net, x, tgt = one_step(B, training)    # noqa: F821
    out["x"] = x.cpu()
    out["tgt"] = tgt.cpu()
    out["prm"] = [p.detach().cpu().clone() for p in net.parameters()]
    set_seed()                                  # noqa: F821
    for p in net.parameters():
        p.grad = None
    loss_l = fused.net_fused_loss(net, x, tgt)
    loss_l.backward()
    torch.cuda.synchronize()
    out["legacy_loss"] = loss_l.detach().cpu()
    out["legacy_grads"] = [p.grad.cpu().clone() for p in net.parameters()]
    return out


@functools.lru_cache(maxsize=None)
def _old(tmp):
    """Every (batch, mode) on the net_fwd_sample kernels: DTP_FWD_TILED=0
    in one fresh child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(tmp, "old.pt")
    env = dict(os.environ, DTP_FWD_TILED="0")
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", _OLD_PROG, path], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    return torch.load(path)


@pytest.fixture(scope="module")
def old(tmp_path_factory):
    return _old(str(tmp_path_factory.mktemp("fwd_old")))


def _windows(a):
    """[B,C,2H,2W] -> [B,C,H,W,4], slots in the kernels' order
    (0,0) (0,1) (1,0) (1,1)."""
    return torch.stack([a[:, :, 0::2, 0::2], a[:, :, 0::2, 1::2],
                        a[:, :, 1::2, 0::2], a[:, :, 1::2, 1::2]], dim=-1)


def _conv_stage(name, got, idx, xin, w, b, scale=None):
    """One conv + (channel scale) + 2x2 max + ReLU stage: the pooled
    output and its index bytes against float64 from `xin`.  Returns the
    float64 windows, their bound and the pooled bound."""
    xd, wd, bd = xin.double(), w.double(), b.double()
    L = w.shape[1] * w.shape[2] * w.shape[3] + 1        # taps + bias
    a = F.conv2d(xd, wd, bd)
    ab = 2 * L * U * F.conv2d(xd.abs(), wd.abs(), bd.abs())
    if scale is not None:       # 0 or 2: exact in fp32
        a, ab = a * scale, ab * scale
    wa, wb = _windows(a), _windows(ab)
    bound = wb.max(dim=-1).values
    within(name, got, wa.max(dim=-1).values.clamp_min(0.0), bound)
    # the named slot is a maximum of its window as far as fp32 can tell
    slot = (idx & 3).long().unsqueeze(-1)
    named = wa.gather(-1, slot).squeeze(-1)
    gap = wa.max(dim=-1).values - named
    worst = float((gap / (2 * bound + 2.0 ** -126)).max())
    print(f"{name}.idx: worst (max - named)/(2*bound) = {worst:.3f}")
    assert bool((gap <= 2 * bound).all()), worst
    # bit 2 <=> the output is zero, and consistent with the float64 sign
    dead = (idx & 4) != 0
    assert bool(((idx & ~7) == 0).all())
    assert torch.equal(dead, got == 0)
    assert bool((named[dead] <= bound[dead]).all())
    assert bool((named[~dead] >= -bound[~dead]).all())
    return wa, wb


def _p2_inputs(s, B, training):
    scale = None
    if training:
        scale = 2.0 * (s["m2"] != 0).double().view(B, 20, 1, 1)
    return s["p1"].view(B, 10, 12, 12), scale


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_p1_and_idx1_from_x(B, training):
    s = _step(B, training)
    _conv_stage("fwd_tiled.p1", s["p1"].view(B, 10, 12, 12),
                s["idx1"].view(B, 10, 12, 12), s["x"], s["prm"][0],
                s["prm"][1])


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_p2_and_idx2_from_own_p1(B, training):
    s = _step(B, training)
    p1, scale = _p2_inputs(s, B, training)
    if training:    # about half of the channels dropped, not all or none
        kept = float((s["m2"] != 0).double().mean())
        assert 0.2 < kept < 0.8 or B == 3, kept
        assert bool((s["m2"] <= 1).all())
    _conv_stage("fwd_tiled.p2", s["p2"].view(B, 20, 4, 4),
                s["idx2"].view(B, 20, 4, 4), p1, s["prm"][2], s["prm"][3],
                scale)


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_head_from_own_p2(B, training):
    """h1 from the GPU's p2; d3 from h1 and m3, exactly; logp from d3; the
    loss from logp."""
    s = _step(B, training)
    wf1, bf1, wf2, bf2 = (t.double() for t in s["prm"][4:8])
    p2 = s["p2"].double()
    within("fwd_tiled.h1", s["h1"], (p2 @ wf1.t() + bf1).clamp_min(0.0),
           2 * 321 * U * (p2.abs() @ wf1.abs().t() + bf1.abs()))

    assert bool((s["m3"] <= 1).all())
    if training:
        assert torch.equal(s["d3"], s["h1"] * 2.0 * s["m3"].float())
    else:
        assert bool((s["m3"] == 1).all())
        assert torch.equal(s["d3"], s["h1"])

    # fc2 within E (the linear rule); log_softmax moves an entry by at most
    # its own input error plus the largest one of its row, and adds the
    # log_softmax bound By of fp32_bounds (N = 10 classes)
    d3 = s["d3"].double()
    z = d3 @ wf2.t() + bf2
    E = 2 * 51 * U * (d3.abs() @ wf2.abs().t() + bf2.abs())
    lse = torch.logsumexp(z, dim=1, keepdim=True)
    y = z - lse
    By = 2 * U * (3 * 10 + T + 1 + T * math.log(10) + lse.abs() + y.abs())
    within("fwd_tiled.logp", s["logp"], y,
           By + E + E.max(dim=1, keepdim=True).values)

    # B terms -logp[b, tgt]/B, each rounded once and summed in fp32: within
    # B*u of their float64 sum, u relative to the summed magnitudes
    lt = s["logp"].double()[torch.arange(B), s["tgt"]]
    within("fwd_tiled.loss", s["loss"], -lt.mean(), B * U * lt.abs().mean())


def _assert_close(name, a, b, atol):
    worst = (a.double() - b.double()).abs().max().item()
    print(f"{name}: worst |new - old| = {worst:.3e}")
    assert worst <= atol, (name, worst)


def _pool_vs_old(name, s, o, shape, idx_name, xin, w, b, scale=None):
    """A pooled array and its index bytes against the old kernel's: values
    within the stage's bound; where an index byte differs, the two named
    slots tie within twice that bound."""
    wa, wb = _conv_stage(f"fwd_tiled.{name}", s[name].view(shape),
                         s[idx_name].view(shape), xin, w, b, scale)
    bound = wb.max(dim=-1).values
    within(f"fwd_tiled.{name}_vs_old", s[name].view(shape),
           o[name].double().view(shape), bound)
    differ = (s[idx_name] != o[idx_name]).view(shape)
    print(f"{idx_name} differs from the old kernel's at "
          f"{int(differ.sum())} cells")
    if bool(differ.any()):
        a = wa.gather(-1, (s[idx_name] & 3).long().view(*shape, 1))
        c = wa.gather(-1, (o[idx_name] & 3).long().view(*shape, 1))
        gap = (a - c).abs().squeeze(-1)
        assert bool((gap <= 2 * bound)[differ].all())


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_against_the_old_forward(B, training, old):
    """Same weights, inputs and dropout seed on the net_fwd_sample kernels:
    the masks bit for bit; the forward's arrays within the bounds of the
    stage tests; where an index byte differs, a tie within those bounds;
    the backward's arrays, the loss and the eight gradients within the
    fused tests' tolerances."""
    s, o = _step(B, training), old[(B, training)]
    assert torch.equal(s["m3"], o["m3"])
    if training:        # eval mode does not write m2
        assert torch.equal(s["m2"], o["m2"])
    _pool_vs_old("p1", s, o, (B, 10, 12, 12), "idx1", s["x"], s["prm"][0],
                 s["prm"][1])
    p1, scale = _p2_inputs(s, B, training)
    _pool_vs_old("p2", s, o, (B, 20, 4, 4), "idx2", p1, s["prm"][2],
                 s["prm"][3], scale)

    wf1, bf1, wf2, bf2 = (t.double() for t in s["prm"][4:8])
    p2 = s["p2"].double()
    bh = 2 * 321 * U * (p2.abs() @ wf1.abs().t() + bf1.abs())
    within("fwd_tiled.h1_vs_old", s["h1"], o["h1"].double(), bh)
    within("fwd_tiled.d3_vs_old", s["d3"], o["d3"].double(),
           bh * (2 if training else 1))
    _assert_close("logp", s["logp"], o["logp"], LOSS_ATOL)
    _assert_close("loss", s["loss"], o["loss"], LOSS_ATOL)
    for n in ("glog", "gh1", "ga2", "ga1"):
        _assert_close(n, s[n], o[n], GRAD_ATOL)
    assert len(s["grads"]) == 8
    for i, (a, b) in enumerate(zip(s["grads"], o["grads"])):
        _assert_close(f"grad {i}", a, b, GRAD_ATOL)


@pytest.mark.parametrize("B", [3, 64])
def test_forced_fallback_gives_the_same_bits(B):
    """Split 2 with poll bound 0: sibling 0 never sees its sibling's token
    and computes that half of conv2 itself.  Same values by construction,
    so p2, h1 and logp equal the normal run's exactly."""
    k = load_native("_kernels")
    net, x, tgt = mk(B)                         # noqa: F821
    net.train()
    ws = fused._ws(B, DEV)
    prm = fused._ptrs(fused._params(net))
    got = {}
    for poll in (60000, 0):
        set_seed()                              # noqa: F821
        for n in ("p2", "h1", "logp"):
            ws[n].fill_(float("nan"))
        k.net_fwd_raw(x.data_ptr(), prm, tgt.data_ptr(), ws.ptrs,
                      ops._seed_ptr(DEV), B, True, True, 2, poll,
                      ops._stream())
        torch.cuda.synchronize()
        got[poll] = {n: ws[n].cpu().clone() for n in ("p2", "h1", "logp")}
    for n in ("p2", "h1", "logp"):
        assert bool(torch.isfinite(got[0][n]).all()), n
        assert torch.equal(got[0][n], got[60000][n]), n


def test_raw_forward_refuses_bad_arguments():
    k = load_native("_kernels")
    ws = fused._ws(3, DEV)
    for B, split, poll in ((0, 1, 0), (3, 3, 0), (3, 2, -1), (2049, 2, 0)):
        with pytest.raises(ValueError):
            k.net_fwd_raw(0, [0] * 8, 0, ws.ptrs, 0, B, True, True, split,
                          poll, 0)


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_step_path_matches_legacy_loss_mode(B, training):
    """net_fused_loss(...).backward() (the forward adds its loss atomically,
    no partials) against net_fused_step from the same seed."""
    s = _step(B, training)
    assert torch.allclose(s["loss"], s["legacy_loss"], atol=1e-6), \
        (s["loss"].item(), s["legacy_loss"].item())
    for i, (a, b) in enumerate(zip(s["grads"], s["legacy_grads"])):
        worst = (a - b).abs().max().item()
        print(f"grad {i}: worst |step - legacy| = {worst:.3e}")
        assert torch.allclose(a, b, atol=1e-6), (i, worst)
