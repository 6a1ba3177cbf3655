"""Fused whole-Net kernels vs the modular HIP pipeline and the CPU
torch reference (eval mode => deterministic, exact comparison)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from dist_tuto_pth_amd.models import Net
from dist_tuto_pth_amd.ops.fused import (attach_flat_grads, net_fused_loss,
                                         net_fused_step)

DEV = "cuda:0"


def _mk(seed=0, B=64):
    torch.manual_seed(seed)
    net_c = Net().eval()
    net_g = Net().eval().to(DEV)
    net_g.load_state_dict({k: v.to(DEV)
                           for k, v in net_c.state_dict().items()})
    x = torch.randn(B, 1, 28, 28)
    tgt = torch.randint(0, 10, (B,))
    return net_c, net_g, x, tgt


def test_fused_loss_matches_cpu_reference_eval():
    net_c, net_g, x, tgt = _mk(0)
    loss_c = F.nll_loss(net_c(x), tgt)
    loss_g = net_fused_loss(net_g, x.to(DEV), tgt.to(DEV))
    torch.cuda.synchronize()
    assert torch.allclose(loss_g.cpu(), loss_c, atol=1e-5), \
        (loss_g.item(), loss_c.item())


def test_fused_grads_match_cpu_reference_eval():
    net_c, net_g, x, tgt = _mk(1)
    loss_c = F.nll_loss(net_c(x), tgt)
    loss_c.backward()
    loss_g = net_fused_loss(net_g, x.to(DEV), tgt.to(DEV))
    loss_g.backward()
    for (n, pc), pg in zip(net_c.named_parameters(), net_g.parameters()):
        assert torch.allclose(pg.grad.cpu(), pc.grad, atol=2e-4), \
            (n, (pg.grad.cpu() - pc.grad).abs().max())


def test_fused_step_overwrites_grads():
    net_c, net_g, x, tgt = _mk(2)
    flat = attach_flat_grads(net_g)
    loss1 = net_fused_step(net_g, x.to(DEV), tgt.to(DEV)).clone()
    g1 = flat.clone()
    # run again: grads must be identical (overwrite, not accumulate)
    loss2 = net_fused_step(net_g, x.to(DEV), tgt.to(DEV)).clone()
    torch.cuda.synchronize()
    assert torch.allclose(loss1, loss2)
    assert torch.allclose(flat, g1)
    # and match the CPU reference
    loss_c = F.nll_loss(net_c(x), tgt)
    loss_c.backward()
    for pc, pg in zip(net_c.parameters(), net_g.parameters()):
        assert torch.allclose(pg.grad.cpu(), pc.grad, atol=2e-4)


def test_fused_step_matches_modular_gpu_eval():
    from dist_tuto_pth_amd import ops
    _, net_g, x, tgt = _mk(3)
    xg, tg = x.to(DEV), tgt.to(DEV)
    loss_mod = ops.nll_loss(net_g(xg), tg)
    loss_mod.backward()
    g_mod = [p.grad.clone() for p in net_g.parameters()]
    for p in net_g.parameters():
        p.grad = None
    loss_f = net_fused_loss(net_g, xg, tg)
    loss_f.backward()
    torch.cuda.synchronize()
    assert torch.allclose(loss_f, loss_mod, atol=1e-5)
    for a, p in zip(g_mod, net_g.parameters()):
        assert torch.allclose(a, p.grad, atol=1e-4)


def test_fused_training_mode_statistics():
    """Train mode: dropout active; loss finite, grads nonzero, and the
    dropout masks advance across STEPS.  Seed convention is bump-AFTER
    (r2): a full step's combine kernel advances the device seed, so
    two consecutive steps draw different masks, while a forward
    WITHOUT a backward reuses the current seed by design."""
    _, net_g, x, tgt = _mk(4, B=256)
    net_g.train()
    flat = attach_flat_grads(net_g)
    l1 = float(net_fused_step(net_g, x.to(DEV), tgt.to(DEV)))
    l2 = float(net_fused_step(net_g, x.to(DEV), tgt.to(DEV)))
    assert l1 == l1 and l2 == l2
    assert l1 != l2   # the first step's combine advanced the seed
    torch.cuda.synchronize()
    assert flat.abs().sum() > 0


def test_fused_step_opt_matches_separate_sgd_eval():
    """combine+SGD fused into one kernel == combine then sgd_step
    (same update formula; eval mode => deterministic)."""
    from dist_tuto_pth_amd.optim import FusedSGD
    from dist_tuto_pth_amd.ops.fused import net_fused_step_opt
    _, net_a, x, tgt = _mk(9)
    _, net_b, _, _ = _mk(9)
    xg, tg = x.to(DEV), tgt.to(DEV)

    attach_flat_grads(net_a)
    opt_a = FusedSGD(net_a.parameters(), lr=0.01, momentum=0.5)
    loss_a = net_fused_step(net_a, xg, tg).clone()
    opt_a.step()

    attach_flat_grads(net_b)
    opt_b = FusedSGD(net_b.parameters(), lr=0.01, momentum=0.5)
    loss_b = net_fused_step_opt(net_b, xg, tg, opt_b).clone()
    torch.cuda.synchronize()

    assert torch.allclose(loss_a, loss_b, atol=1e-6)
    for (n, pa), pb in zip(net_a.named_parameters(), net_b.parameters()):
        assert torch.allclose(pa, pb, atol=1e-6), n
        assert torch.allclose(pa.grad, pb.grad, atol=1e-6), n
    for ba, bb in zip(opt_a._bufs, opt_b._bufs):
        assert torch.allclose(ba, bb, atol=1e-6)


def test_fused_step_large_batch_matches_cpu():
    """B > 512 now runs the same segmented-partial gw path (the
    adaptive per-op path measured 4x slower at B=4096; profiles/)."""
    net_c, net_g, x, tgt = _mk(11, B=1024)
    flat = attach_flat_grads(net_g)
    loss_g = net_fused_step(net_g, x.to(DEV), tgt.to(DEV)).clone()
    torch.cuda.synchronize()
    loss_c = F.nll_loss(net_c(x), tgt)
    loss_c.backward()
    assert torch.allclose(loss_g.cpu(), loss_c, atol=1e-5)
    for (n, pc), pg in zip(net_c.named_parameters(), net_g.parameters()):
        assert torch.allclose(pg.grad.cpu(), pc.grad, atol=5e-4), n


def test_megakernel_matches_fused_eval():
    """Single-launch cooperative step == 6-dispatch fused path, exactly
    (same shared __device__ code, eval mode => deterministic)."""
    from dist_tuto_pth_amd.optim import FusedSGD
    from dist_tuto_pth_amd.ops.fused import (net_fused_train_step,
                                             net_step_available)
    if not net_step_available():
        pytest.skip("cooperative launch unavailable")
    _, net_a, x, tgt = _mk(6)
    _, net_b, _, _ = _mk(6)
    xg, tg = x.to(DEV), tgt.to(DEV)

    attach_flat_grads(net_a)
    opt_a = FusedSGD(net_a.parameters(), lr=0.01, momentum=0.5)
    loss_a = net_fused_step(net_a, xg, tg).clone()
    opt_a.step()

    attach_flat_grads(net_b)
    opt_b = FusedSGD(net_b.parameters(), lr=0.01, momentum=0.5)
    loss_b = net_fused_train_step(net_b, xg, tg, opt_b).clone()
    torch.cuda.synchronize()

    assert torch.allclose(loss_a, loss_b, atol=1e-6), \
        (loss_a.item(), loss_b.item())
    for (n, pa), pb in zip(net_a.named_parameters(), net_b.parameters()):
        assert torch.allclose(pa, pb, atol=1e-6), \
            (n, (pa - pb).abs().max().item())
        assert torch.allclose(pa.grad, pb.grad, atol=1e-6), n
    for ba, bb in zip(opt_a._bufs, opt_b._bufs):
        assert torch.allclose(ba, bb, atol=1e-6)


def test_megakernel_no_sgd_leaves_params():
    """do_sgd=False (the DP mode): grads written, params untouched."""
    from dist_tuto_pth_amd.ops.fused import (net_fused_train_step,
                                             net_step_available)
    if not net_step_available():
        pytest.skip("cooperative launch unavailable")
    _, net_g, x, tgt = _mk(7)
    p0 = [p.clone() for p in net_g.parameters()]
    flat = attach_flat_grads(net_g)
    net_fused_train_step(net_g, x.to(DEV), tgt.to(DEV), do_sgd=False)
    torch.cuda.synchronize()
    assert flat.abs().sum() > 0
    for a, p in zip(p0, net_g.parameters()):
        assert torch.equal(a, p)


def test_megakernel_training_convergence():
    """A few single-launch steps reduce the loss on a fixed batch."""
    from dist_tuto_pth_amd.optim import FusedSGD
    from dist_tuto_pth_amd.ops.fused import (net_fused_train_step,
                                             net_step_available)
    if not net_step_available():
        pytest.skip("cooperative launch unavailable")
    _, net_g, x, tgt = _mk(8, B=256)
    net_g.train()
    attach_flat_grads(net_g)
    opt = FusedSGD(net_g.parameters(), lr=0.05, momentum=0.5)
    xg, tg = x.to(DEV), tgt.to(DEV)
    losses = []
    for _ in range(150):
        losses.append(net_fused_train_step(net_g, xg, tg, opt).item())
    first = sum(losses[:10]) / 10
    last = sum(losses[-10:]) / 10
    assert last < first - 0.12, (first, last)


def test_fused_training_convergence():
    """A few fused steps reduce the loss on a fixed batch."""
    from dist_tuto_pth_amd.optim import FusedSGD
    _, net_g, x, tgt = _mk(5, B=256)
    net_g.train()
    attach_flat_grads(net_g)
    opt = FusedSGD(net_g.parameters(), lr=0.05, momentum=0.5)
    xg, tg = x.to(DEV), tgt.to(DEV)
    losses = []
    for _ in range(150):
        loss = net_fused_step(net_g, xg, tg)
        opt.step()
        losses.append(loss.item())
    # CPU reference with identical hyperparameters drops ~0.24 over 150
    # steps (2.30 -> 2.06); require at least half that improvement
    first = sum(losses[:10]) / 10
    last = sum(losses[-10:]) / 10
    assert last < first - 0.12, (first, last)


def test_fused_step_tiny_odd_batch():
    """B=3: odd, smaller than every tile/chunk constant — exercises the
    split/bchunk/nch edge paths."""
    net_c, net_g, x, tgt = _mk(12, B=3)
    attach_flat_grads(net_g)
    loss_g = net_fused_step(net_g, x.to(DEV), tgt.to(DEV)).clone()
    torch.cuda.synchronize()
    loss_c = F.nll_loss(net_c(x), tgt)
    loss_c.backward()
    assert torch.allclose(loss_g.cpu(), loss_c, atol=1e-5)
    for (n, pc), pg in zip(net_c.named_parameters(), net_g.parameters()):
        assert torch.allclose(pg.grad.cpu(), pc.grad, atol=2e-4), n


def test_fwdbwd_matches_fused_eval():
    """The combined fwd+bwd single-kernel step must produce identical
    loss and grads to the separate fwd/bwd dispatch path (eval mode:
    bit-deterministic)."""
    from dist_tuto_pth_amd.ops.fused import net_fused_step_fb
    net_c, net_g, x, tgt = _mk(11)
    flat = attach_flat_grads(net_g)
    loss_a = net_fused_step(net_g, x.to(DEV), tgt.to(DEV)).clone()
    g_a = flat.clone()
    loss_b = net_fused_step_fb(net_g, x.to(DEV), tgt.to(DEV)).clone()
    torch.cuda.synchronize()
    assert torch.allclose(loss_a, loss_b, atol=1e-6)
    assert torch.equal(flat, g_a) or torch.allclose(flat, g_a, atol=1e-6)


def test_fwdbwd_sgd_matches_separate_eval():
    """fwdbwd with the fused SGD combine == fwd/bwd + separate SGD."""
    from dist_tuto_pth_amd.optim import FusedSGD
    from dist_tuto_pth_amd.ops.fused import net_fused_step_fb
    net_c, net_a, x, tgt = _mk(12)
    torch.manual_seed(12)
    net_b = Net().eval().to(DEV)
    net_b.load_state_dict(net_a.state_dict())
    attach_flat_grads(net_a)
    attach_flat_grads(net_b)
    opt_a = FusedSGD(net_a.parameters(), lr=0.01, momentum=0.5)
    opt_b = FusedSGD(net_b.parameters(), lr=0.01, momentum=0.5)
    xg, tg = x.to(DEV), tgt.to(DEV)
    for _ in range(3):
        net_fused_step(net_a, xg, tg)
        opt_a.step()
        net_fused_step_fb(net_b, xg, tg, opt_b)
    torch.cuda.synchronize()
    for pa, pb in zip(net_a.parameters(), net_b.parameters()):
        assert torch.allclose(pa, pb, atol=1e-6), \
            (pa - pb).abs().max()


def test_fwdbwd_training_convergence():
    """Same statistical bar as the other training-mode convergence
    tests: 150 steps with dropout on, mean-of-10 loss drops >= 0.12
    (the CPU reference drops ~0.24 with these hyperparameters)."""
    from dist_tuto_pth_amd.optim import FusedSGD
    from dist_tuto_pth_amd.ops.fused import net_fused_step_fb
    _, net_g, x, tgt = _mk(13, B=256)
    net_g.train()
    attach_flat_grads(net_g)
    opt = FusedSGD(net_g.parameters(), lr=0.05, momentum=0.5)
    xg, tg = x.to(DEV), tgt.to(DEV)
    losses = []
    for _ in range(150):
        losses.append(float(net_fused_step_fb(net_g, xg, tg, opt)))
    first = sum(losses[:10]) / 10
    last = sum(losses[-10:]) / 10
    assert last < first - 0.12, (first, last)


def _one_step_state(kind):
    """One eval-mode training step at B=64 through entry point `kind`;
    returns grads, parameters and momentum buffers as flat lists.
    Self-contained: its source also runs in the fold subprocess."""
    import torch
    from dist_tuto_pth_amd.models import Net
    from dist_tuto_pth_amd.ops import fused
    from dist_tuto_pth_amd.optim import FusedSGD
    torch.manual_seed(11)
    net_c = Net().eval()
    net_g = Net().eval().to("cuda:0")
    net_g.load_state_dict({k: v.to("cuda:0")
                           for k, v in net_c.state_dict().items()})
    x = torch.randn(64, 1, 28, 28).to("cuda:0")
    tgt = torch.randint(0, 10, (64,)).to("cuda:0")
    bufs = []
    if kind == "step":
        fused.net_fused_step(net_g, x, tgt)
    else:
        opt = FusedSGD(net_g.parameters(), lr=0.01, momentum=0.5)
        step = {"opt": fused.net_fused_step_opt,
                "fb": fused.net_fused_step_fb}[kind]
        step(net_g, x, tgt, opt)
        bufs = opt._bufs
    torch.cuda.synchronize()
    out = {}
    for n, p in net_g.named_parameters():
        out["grad " + n] = p.grad.cpu().flatten().tolist()
        out["param " + n] = p.detach().cpu().flatten().tolist()
    for i, b in enumerate(bufs):
        out["momentum %d" % i] = b.cpu().flatten().tolist()
    return out


@pytest.mark.parametrize("kind", ["step", "opt", "fb"])
def test_fold_optin_matches_default_subprocess(kind):
    """The opt-in in-launch gw fold (DTP_GW_FOLD=1, a documented
    measured-negative kept for the record — see
    profiles/convnet_step_history.md) must stay numerically correct at
    every call site of the gw launch: run one step (plain, with the
    fused optimizer, and through the combined fwd+bwd kernel with the
    fused optimizer) in a subprocess with the flag set (it is read once
    per process) and compare grads, updated parameters and momentum
    buffers against this process's default combine path."""
    import inspect
    import json
    import os
    import subprocess
    import sys

    want = _one_step_state(kind)
    assert len(want) == (16 if kind == "step" else 24)

    prog = (inspect.getsource(_one_step_state) +
            "\nimport json, sys\n"
            "print(json.dumps(_one_step_state(sys.argv[1])))\n")
    env = dict(os.environ, DTP_GW_FOLD="1")
    r = subprocess.run([sys.executable, "-c", prog, kind], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got.keys() == want.keys()
    for n, w in want.items():
        g, w = torch.tensor(got[n]), torch.tensor(w)
        assert torch.allclose(g, w, atol=1e-6), \
            (n, (g - w).abs().max().item())


@pytest.mark.parametrize("B", [6, 193])
def test_interleaved_entry_points_share_workspace(B):
    """Every entry point runs on the ONE cached per-(B, device)
    workspace and pointer vector: calling them in turn on one net (eval
    mode) must give the same loss and gradients each time.  B=6 is below
    every gw chunk count (nch = B) and takes the split forward; B=193
    has no split, nch=24 / nch2=32 and chunks that do not divide B."""
    from dist_tuto_pth_amd.ops.fused import (net_fused_step_fb,
                                             net_fused_train_step,
                                             net_step_available)
    _, net_g, x, tgt = _mk(30 + B, B=B)
    xg, tg = x.to(DEV), tgt.to(DEV)
    params = list(net_g.named_parameters())

    loss0 = net_fused_loss(net_g, xg, tg)
    loss0.backward()
    torch.cuda.synchronize()
    loss0 = loss0.detach().clone()
    want = [p.grad.clone() for _, p in params]
    assert all(w.abs().sum() > 0 for w in want)

    steps = [("step", lambda: net_fused_step(net_g, xg, tg)),
             ("fb", lambda: net_fused_step_fb(net_g, xg, tg))]
    if net_step_available():
        steps.append(("train_step", lambda: net_fused_train_step(
            net_g, xg, tg, do_sgd=False)))
    for name, step in steps:
        loss = step().clone()
        torch.cuda.synchronize()
        assert torch.allclose(loss, loss0, atol=1e-6), \
            (name, loss.item(), loss0.item())
        for (n, p), w in zip(params, want):
            assert torch.allclose(p.grad, w, atol=1e-6), \
                (name, n, (p.grad - w).abs().max().item())
            p.grad.zero_()  # the next entry point must rewrite it


@pytest.mark.parametrize("B", [33, 100, 257])
def test_fused_step_odd_batch_sizes(B):
    """Non-divisible batch sizes produce EMPTY tail chunk rows in the
    gw partial grid (ceil rounding) and exercise the family-specific
    conv2 chunk count — regression for the unguarded staging prologue
    that read past the workspaces for such rows."""
    net_c, net_g, x, tgt = _mk(20 + B, B=B)
    loss_c = F.nll_loss(net_c(x), tgt)
    loss_c.backward()
    net_fused_step(net_g, x.to(DEV), tgt.to(DEV))
    torch.cuda.synchronize()
    for (n, pc), pg in zip(net_c.named_parameters(), net_g.parameters()):
        assert torch.allclose(pg.grad.cpu(), pc.grad, atol=5e-4), \
            (n, (pg.grad.cpu() - pc.grad).abs().max())
