"""The data backward of the fused Net step, stage by stage against float64
references computed from the GPU's OWN stage inputs (read back from the
workspace), then path against path.

Batches cover every sibling split of the data-backward kernel and both
forward kernels: 3 (split 8, odd), 64 (split 4, split fwd), 128 (split 2,
split fwd), 130 (split 2, plain fwd), 256 (split 1, two tile rounds).
One step per (batch, mode) is run once and shared by the tests.

Bounds are the project's rule (tests/fp32_bounds.py): an fp32 sum of L
terms is within 2*L*u*sum|terms|.
"""

import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fp32_bounds import T, U, within

from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.models import Net
from dist_tuto_pth_amd.ops import fused

DEV = torch.device("cuda:0")
BATCHES = [3, 64, 128, 130, 256]
WS_READ = ("idx1", "m2", "idx2", "h1", "m3", "logp", "glog", "gh1", "ga2",
           "ga1")


def _seed_buf():
    ops._seed_ptr(DEV)      # creates it
    return ops._seed_bufs[DEV.index]


def _mk(B):
    g = torch.Generator().manual_seed(977 + B)
    net = Net()
    with torch.no_grad():
        for p in net.parameters():      # biases away from zero as well
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    x = torch.randn(B, 1, 28, 28, generator=g)
    tgt = torch.randint(0, 10, (B,), generator=g)
    return net.to(DEV), x.to(DEV), tgt.to(DEV)


@functools.lru_cache(maxsize=None)
def _step(B, training):
    """One net_fused_step; the workspace, loss and gradients on the CPU,
    and what the legacy autograd path gives from the same seed."""
    net, x, tgt = _mk(B)
    net.train(training)
    seed = _seed_buf()
    seed0 = seed.clone()
    loss = fused.net_fused_step(net, x, tgt).clone()
    torch.cuda.synchronize()
    ws = fused._ws(B, DEV)
    out = {n: ws[n].cpu().clone() for n in WS_READ}
    out["loss"] = loss.cpu()
    out["grads"] = [p.grad.cpu().clone() for p in net.parameters()]
    out["w2"] = net.conv2.weight.detach().cpu()
    out["wf1"] = net.fc1.weight.detach().cpu()
    out["wf2"] = net.fc2.weight.detach().cpu()
    out["tgt"] = tgt.cpu()

    # the legacy path (a real upstream gradient) with the same masks
    seed.copy_(seed0)
    for p in net.parameters():
        p.grad = None
    loss_l = fused.net_fused_loss(net, x, tgt)
    loss_l.backward()
    torch.cuda.synchronize()
    out["legacy_loss"] = loss_l.detach().cpu()
    out["legacy_grads"] = [p.grad.cpu().clone() for p in net.parameters()]
    return out


def _route_pool(g, idx, scale=None):
    """Max-pool backward with the kernels' index bytes: bit 2 = the ReLU
    behind the pool is dead, bits 0-1 = the 2x2 window slot.  g and idx are
    [B,C,H,W]; returns [B,C,2H,2W] with every other slot exactly zero."""
    Bn, C, H, W = g.shape
    out = torch.zeros(Bn, C, 2 * H, 2 * W, dtype=torch.float64)
    live = (idx & 4) == 0
    am = (idx & 3).long()
    v = torch.where(live, g, torch.zeros_like(g))
    if scale is not None:
        v = v * scale
    for slot in range(4):
        out[:, :, slot >> 1::2, slot & 1::2] = torch.where(
            am == slot, v, torch.zeros_like(v))
    return out


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_conv2_input_gradient_from_own_ga2(B, training):
    """The hot loop alone: ga1 against the float64 conv2 input-gradient of
    the GPU's own ga2, routed through pool1/ReLU by the GPU's own idx1.
    No element is excluded; the slots a window does not route to must be
    exactly zero (their bound is 2^-126)."""
    s = _step(B, training)
    ga2 = s["ga2"].double().view(B, 20, 8, 8)
    w2 = s["w2"].double()
    idx1 = s["idx1"].view(B, 10, 12, 12)
    shape = (B, 10, 12, 12)
    ref = torch.nn.grad.conv2d_input(shape, w2, ga2)
    bound = 2 * 500 * U * torch.nn.grad.conv2d_input(shape, w2.abs(),
                                                     ga2.abs())
    assert float(ga2.abs().sum()) > 0
    within("bwd_data.ga1", s["ga1"].view(B, 10, 24, 24),
           _route_pool(ref, idx1), _route_pool(bound, idx1))


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_head_gradients_from_own_intermediates(B, training):
    """The head alone: glog from the GPU's logp (the `fused gx` rule with
    the log-prob taken as given, By = 0), gh1 from the GPU's glog and ga2
    from the GPU's gh1 (the `linear gx` rule), in float64 autograd.  The
    dropout masks are the ones the forward stored (m2 / m3)."""
    s = _step(B, training)
    tgt = s["tgt"]
    # glog = (exp(logp) - onehot) / B
    logp = s["logp"].double()
    p = logp.exp()
    onehot = torch.zeros(B, 10, dtype=torch.float64)
    onehot[torch.arange(B), tgt] = 1.0
    d = p - onehot
    within("bwd_data.glog", s["glog"], d / B,
           2 * (p * (T + 1) * U + 3 * U * d.abs()) / B)

    # gh1 = relu'(h1) * dropout(m3) * (glog @ wf2)
    glog = s["glog"].double()
    wf2 = s["wf2"].double()
    d3 = torch.zeros(B, 50, dtype=torch.float64, requires_grad=True)
    (d3 @ wf2.t()).backward(glog)
    keep = (s["h1"] > 0).double()
    if training:
        keep = keep * 2.0 * (s["m3"] != 0).double()
    within("bwd_data.gh1", s["gh1"], d3.grad * keep,
           2 * 10 * U * (glog.abs() @ wf2.abs()) * keep)

    # ga2 = pool2/ReLU routing of dropout2d(m2) * (gh1 @ wf1)
    gh1 = s["gh1"].double()
    wf1 = s["wf1"].double()
    p2 = torch.zeros(B, 320, dtype=torch.float64, requires_grad=True)
    (p2 @ wf1.t()).backward(gh1)
    gp2 = p2.grad.view(B, 20, 4, 4)
    bp2 = (2 * 50 * U * (gh1.abs() @ wf1.abs())).view(B, 20, 4, 4)
    scale = None
    if training:
        scale = 2.0 * (s["m2"] != 0).double().view(B, 20, 1, 1)
    idx2 = s["idx2"].view(B, 20, 4, 4)
    within("bwd_data.ga2", s["ga2"].view(B, 20, 8, 8),
           _route_pool(gp2, idx2, scale), _route_pool(bp2, idx2, scale))


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("B", BATCHES)
def test_step_path_matches_legacy_autograd_path(B, training):
    """Same weights, inputs and (restored) dropout seed: the step path's
    loss and all 8 gradients against net_fused_loss + backward."""
    s = _step(B, training)
    assert torch.allclose(s["loss"], s["legacy_loss"], atol=1e-6), \
        (s["loss"].item(), s["legacy_loss"].item())
    assert len(s["grads"]) == 8
    for i, (a, b) in enumerate(zip(s["grads"], s["legacy_grads"])):
        worst = (a - b).abs().max().item()
        print(f"grad {i}: worst |step - legacy| = {worst:.3e}")
        assert torch.allclose(a, b, atol=1e-6), (i, worst)


_SPLIT_PROG = r"""
import sys
import torch
from dist_tuto_pth_amd.models import Net
from dist_tuto_pth_amd.ops import fused
dev = torch.device("cuda:0")
out = {}
for B in (3, 64, 128, 130, 256):
    for training in (False, True):
        g = torch.Generator().manual_seed(31 + B)
        net = Net()
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        net = net.to(dev).train(training)
        x = torch.randn(B, 1, 28, 28, generator=g).to(dev)
        tgt = torch.randint(0, 10, (B,), generator=g).to(dev)
        loss = fused.net_fused_step(net, x, tgt)
        torch.cuda.synchronize()
        out["%d,%d" % (B, training)] = [loss.cpu()] + [p.grad.cpu()
                                             for p in net.parameters()]
torch.save(out, sys.argv[1])
"""


def test_forward_sibling_split_on_and_off_agree(tmp_path):
    """The forward's sibling hand-off against the one-workgroup forward
    (what the hand-off's fallback computes): DTP_FWD_SPLIT=1 and =2 in two
    fresh processes (the variable is read once per process), every batch,
    eval and train; each process starts from the same dropout seed."""
    got = {}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for v in ("1", "2"):
        path = tmp_path / f"split{v}.pt"
        env = dict(os.environ, DTP_FWD_SPLIT=v)
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "-c", _SPLIT_PROG, str(path)],
                           env=env, capture_output=True, text=True,
                           timeout=180)
        assert r.returncode == 0, r.stderr[-2000:]
        got[v] = torch.load(path)
    assert got["1"].keys() == got["2"].keys() and len(got["1"]) == 10
    for key, a in got["1"].items():
        for i, (u, w) in enumerate(zip(a, got["2"][key])):
            assert torch.allclose(u, w, atol=1e-6), \
                (key, i, (u - w).abs().max().item())
