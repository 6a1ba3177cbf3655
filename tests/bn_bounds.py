"""Float64 references and derived elementwise bounds for ops.batchnorm2d,
shared by tests/test_batchnorm_cpu.py and tests/test_batchnorm_gpu.py.

Notation: u = 2^-24 (fp32 unit roundoff), h = 2^-8 (bf16 half-ulp,
relative).  The project's rule: an fp32 sum of L terms is within
L*u*sum|terms|, doubled for summation order.  References are float64 on the
same input values.  Per channel, n = B*H*W, mu is the float64 mean, v the
biased variance, r = 1/sqrt(v + eps).

  mean      Bm = 2*n*u*mean|x|
  variance  Bv = 2*(n+4)*u*v + Bm^2      (scales with the CENTRED moment,
                                          so E[x^2]-E[x]^2 fails it on
                                          offset inputs)
  forward   dr = r*Bv/(2(v+eps)) + 2u*r
            A  = |g|*(Bm*r + |x-mu|*dr) + 4u*(|g|*|x-mu|*r + |b| + |res|)
            fp32: A;  bf16: A + h*(|y_ref| + A);  ReLU is 1-Lipschitz
  eval fwd  6u*(|g|*|x-rm|*r + |b| + |res|), plus the bf16 term
  backward  reference = float64 evaluation of
              dbeta = sum g, dgamma = sum g*xhat,
              gx = gamma*rs*(g - dbeta/n - xhat*dgamma/n)   (training)
              gx = gamma*rs*g                               (eval)
            with g = gy*(y > 0) masked by the op's OWN output, and
            xhat = (x - ms)*rs on the op's OWN saved fp32 statistics
            (ms, rs), which the tests read from
            ops._batchnorm2d_forward (the function the autograd op calls;
            it is deterministic, so these are the saved values bit for
            bit).  Running buffers with momentum=1.0 give the same mean
            but only var*n/(n-1), not invstd, hence this route.
            Bdb = 2*n*u*sum|g|,  Bdg = 2*(n+3)*u*sum|g*xhat|
            gx within |gamma|*rs*(Bdb/n + |xhat|*Bdg/n)
                      + 6u*|gamma|*rs*(|g| + |dbeta|/n + |xhat*dgamma|/n),
            plus the bf16 term; g_residual equals g exactly.
"""

import torch
import torch.nn.functional as F

from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.models.resnet import ResNet

U = 2.0 ** -24
H = 2.0 ** -8
EPS = 1e-5


def chan(t):
    return t.view(1, -1, 1, 1)


def within(name, got, ref, bound):
    err = (got.detach().double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: worst error/bound = {ratio:.3f}")
    assert bool((err <= bound).all()), \
        f"{name}: worst error/bound ratio {ratio:.3f}"


def make_case(shape, dtype, residual, offset=0.0, seed=0):
    """CPU inputs whose values are representable in ``dtype``."""
    B, C, Hh, W = shape
    g = torch.Generator().manual_seed(seed + 7 * B + 11 * C + 13 * Hh + W)
    x = (offset + torch.randn(B, C, Hh, W, generator=g)).to(dtype)
    gamma = 0.5 + torch.rand(C, generator=g)
    gamma[::2] *= -1.0            # both signs
    beta = torch.randn(C, generator=g)
    res = torch.randn(B, C, Hh, W, generator=g).to(dtype) if residual \
        else None
    gy = torch.randn(B, C, Hh, W, generator=g).to(dtype)
    return x, gamma, beta, res, gy


def _bf16_term(dtype, ref, A):
    return A + H * (ref.abs() + A) if dtype == torch.bfloat16 else A


def forward_reference(x, gamma, beta, res, relu, eps=EPS):
    """float64 training forward and its bounds."""
    xd, gd, bd = x.double(), gamma.double(), beta.double()
    n = x.numel() // x.shape[1]
    mu = xd.mean(dim=(0, 2, 3))
    d = xd - chan(mu)
    v = (d * d).mean(dim=(0, 2, 3))
    r = 1.0 / torch.sqrt(v + eps)
    y = d * chan(gd * r) + chan(bd)
    rabs = torch.zeros_like(y)
    if res is not None:
        y = y + res.double()
        rabs = res.double().abs()
    if relu:
        y = y.clamp_min(0.0)
    Bm = 2 * n * U * xd.abs().mean(dim=(0, 2, 3))
    Bv = 2 * (n + 4) * U * v + Bm * Bm
    dr = r * Bv / (2 * (v + eps)) + 2 * U * r
    A = chan(gd.abs()) * (chan(Bm * r) + d.abs() * chan(dr)) \
        + 4 * U * (chan(gd.abs() * r) * d.abs() + chan(bd.abs()) + rabs)
    return {"n": n, "mu": mu, "v": v, "y": y, "Bm": Bm, "Bv": Bv,
            "By": _bf16_term(x.dtype, y, A)}


def eval_forward_reference(x, gamma, beta, rm, rv, res, relu, eps=EPS):
    xd, gd, bd = x.double(), gamma.double(), beta.double()
    d = xd - chan(rm.double())
    r = 1.0 / torch.sqrt(rv.double() + eps)
    y = d * chan(gd * r) + chan(bd)
    rabs = torch.zeros_like(y)
    if res is not None:
        y = y + res.double()
        rabs = res.double().abs()
    if relu:
        y = y.clamp_min(0.0)
    A = 6 * U * (chan(gd.abs() * r) * d.abs() + chan(bd.abs()) + rabs)
    return y, _bf16_term(x.dtype, y, A)


def backward_reference(x, gamma, gy, mean, invstd, y_op, relu, training):
    """float64 backward on the op's own fp32 statistics (``mean``,
    ``invstd``) and its own output mask; returns references and bounds."""
    xd, gd = x.double(), gamma.double()
    n = x.numel() // x.shape[1]
    ms, rs = mean.double().cpu(), invstd.double().cpu()
    g = gy.double()
    if relu:
        g = g * (y_op.detach().double().cpu() > 0)
    xhat = (xd - chan(ms)) * chan(rs)
    db = g.sum(dim=(0, 2, 3))
    dg = (g * xhat).sum(dim=(0, 2, 3))
    Bdb = 2 * n * U * g.abs().sum(dim=(0, 2, 3))
    Bdg = 2 * (n + 3) * U * (g * xhat).abs().sum(dim=(0, 2, 3))
    sc = chan(gd.abs() * rs)
    if training:
        gx = chan(gd * rs) * (g - chan(db / n) - xhat * chan(dg / n))
        A = sc * (chan(Bdb / n) + xhat.abs() * chan(Bdg / n)) \
            + 6 * U * sc * (g.abs() + chan(db.abs() / n)
                            + (xhat * chan(dg)).abs() / n)
    else:
        gx = chan(gd * rs) * g
        A = 6 * U * sc * g.abs()
    return {"g": g, "gx": gx, "Bgx": _bf16_term(x.dtype, gx, A),
            "db": db, "Bdb": Bdb, "dg": dg, "Bdg": Bdg}


# ---------------------------------------------------------------------------
# case runners, shared by the CPU and the GPU file
# ---------------------------------------------------------------------------
def train_case(shape, dtype, residual, relu, offset=0.0, dev="cpu"):
    """Runs one training forward+backward of the op on ``dev`` and checks
    every output against its bound."""
    x, gamma, beta, res, gy = make_case(shape, dtype, residual, offset)
    C = shape[1]
    ref = forward_reference(x, gamma, beta, res, relu)
    n = ref["n"]

    xt = x.clone().to(dev).requires_grad_(True)
    wt = gamma.clone().to(dev).requires_grad_(True)
    bt = beta.clone().to(dev).requires_grad_(True)
    rt = res.clone().to(dev).requires_grad_(True) if residual else None
    rm = torch.full((C,), 3.0, device=dev)
    rv = torch.full((C,), 7.0, device=dev)
    y = ops.batchnorm2d(xt, wt, bt, rm, rv, training=True, momentum=1.0,
                        eps=EPS, residual=rt, fuse_relu=relu)
    assert y.dtype == dtype and y.shape == x.shape
    within("y", y, ref["y"], ref["By"])
    # momentum=1.0: the running buffers now hold the batch statistics
    within("mean", rm, ref["mu"], ref["Bm"])
    within("var", rv, ref["v"] * n / (n - 1), ref["Bv"] * n / (n - 1))

    with torch.no_grad():
        y2, mean, invstd = ops._batchnorm2d_forward(
            x.to(dev), gamma.to(dev), beta.to(dev), None, None, True, 0.1,
            EPS, res.to(dev) if residual else None, relu)
    assert torch.equal(y2, y.detach())
    assert torch.equal(mean, rm)
    assert mean.dtype == invstd.dtype == torch.float32

    y.backward(gy.to(dev))
    bref = backward_reference(x, gamma, gy, mean, invstd, y, relu, True)
    assert xt.grad.dtype == dtype and xt.grad.shape == x.shape
    assert wt.grad.dtype == torch.float32 and wt.grad.shape == (C,)
    assert bt.grad.dtype == torch.float32 and bt.grad.shape == (C,)
    within("gx", xt.grad, bref["gx"], bref["Bgx"])
    within("gweight", wt.grad, bref["dg"], bref["Bdg"])
    within("gbias", bt.grad, bref["db"], bref["Bdb"])
    if residual:
        assert rt.grad.dtype == dtype and rt.grad.shape == x.shape
        assert torch.equal(rt.grad.double().cpu(), bref["g"])


def eval_case(shape, dtype, residual, relu, dev):
    x, gamma, beta, res, gy = make_case(shape, dtype, residual)
    C = shape[1]
    g = torch.Generator().manual_seed(5)
    rm = torch.randn(C, generator=g)
    rv = 0.5 + torch.rand(C, generator=g)
    yref, By = eval_forward_reference(x, gamma, beta, rm, rv, res, relu)
    xt = x.clone().to(dev).requires_grad_(True)
    wt = gamma.clone().to(dev).requires_grad_(True)
    bt = beta.clone().to(dev).requires_grad_(True)
    rt = res.clone().to(dev).requires_grad_(True) if residual else None
    rmt, rvt = rm.clone().to(dev), rv.clone().to(dev)
    y = ops.batchnorm2d(xt, wt, bt, rmt, rvt, training=False, momentum=0.5,
                        eps=EPS, residual=rt, fuse_relu=relu)
    assert y.dtype == dtype
    within("y", y, yref, By)
    y.backward(gy.to(dev))
    # the running buffers are not touched, bit for bit
    assert torch.equal(rmt.cpu(), rm) and torch.equal(rvt.cpu(), rv)
    inv = (1.0 / torch.sqrt(rv.double() + EPS))
    bref = backward_reference(x, gamma, gy, rm, inv, y, relu, False)
    assert xt.grad.dtype == dtype
    within("gx", xt.grad, bref["gx"], bref["Bgx"])
    within("gweight", wt.grad, bref["dg"], bref["Bdg"])
    within("gbias", bt.grad, bref["db"], bref["Bdb"])
    if residual:
        assert torch.equal(rt.grad.double().cpu(), bref["g"])


def tiny_resnet_batch(B=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    T = torch.randn(10, 3, 32, 32, generator=g)
    tgt = torch.arange(B) % 10
    x = T[tgt] + 0.3 * torch.randn(B, 3, 32, 32, generator=g)
    return x, tgt


# Chosen on the CPU: the fp32 (compute_dtype=None) model goes 2.870 -> 1.323
# -> 0.056 -> 0.003 in three plain-SGD steps on this batch, far below half
# its initial loss; more steps would only make the test slower.
TINY_STEPS = 3
TINY_LR = 0.05


def tiny_resnet_losses(compute_dtype, dev):
    torch.manual_seed(0)
    net = ResNet((1, 1, 1, 1), num_classes=10, compute_dtype=compute_dtype)
    net = net.to(dev).train()
    x, tgt = tiny_resnet_batch()
    x, tgt = x.to(dev), tgt.to(dev)
    opt = torch.optim.SGD(net.parameters(), lr=TINY_LR)
    losses = []
    for _ in range(TINY_STEPS + 1):
        opt.zero_grad()
        loss = F.cross_entropy(net(x), tgt)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    return losses


def check_tiny_resnet_convergence(dev):
    ref = tiny_resnet_losses(None, dev)
    got = tiny_resnet_losses(torch.bfloat16, dev)
    l0, l_ref, l_bf16 = ref[0], ref[-1], got[-1]
    print(f"fp32 {l0:.4f} -> {l_ref:.4f}; bf16 {got[0]:.4f} -> {l_bf16:.4f}")
    assert l_ref < 0.5 * l0, ref
    assert l_bf16 <= l0 - 0.5 * (l0 - l_ref), (ref, got)
