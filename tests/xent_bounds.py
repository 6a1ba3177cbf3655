"""Float64 references, case lists and derived bounds for ops.cross_entropy
(K21, csrc/cross_entropy.hip) and for FusedSGD's weight decay and Nesterov
momentum, shared by tests/test_cross_entropy_{cpu,gpu}.py and
tests/test_sgd_decay_{cpu,gpu}.py.  The rules are those of
tests/fp32_bounds.py: u = 2^-24, an fp32 sum of L terms is within
L*u*sum|terms|, doubled for summation order, T = 4 stands for the hardware
exp and log, and 2^-126 is added to every bound.

cross_entropy.  The reference is F.cross_entropy in float64 on the same
values with the same label_smoothing (eps), ignore_index and reduction; its
gradient comes from autograd with a non-unit upstream gradient
((3*loss).backward() for "mean" and "sum", a random [B] vector for "none").

  lse   Blse = 2u*(3N + T + 1 + T*ln N + |lse|).
        The kernel takes s = sum exp(x_i - m) in one pass with a running
        maximum (online softmax).  Relative to s (which is >= 1, the
        maximum contributes exp(0)), the error has these parts, in units of
        u: N for the sum of N terms in any order; T + 1 for each term's
        exp; and, for the online form, the chain of rescalings
        s <- s*exp(m_old - m_new) a term goes through.  A rescaling is
        skipped (factor exactly 1) when the maximum does not move and when
        one side of a merge is empty, so a chain has at most K real steps
        with K <= (number of 8-element chunks) - 1 < N/8, each costing
        T + 2 (one exp, one product): below 0.75*N.  The rounding of an
        exponent d = x_i - m, and of log2(e)*d inside exp, is a relative
        error u*|d| on a term of size e^-|d|, at most u/e per term however
        the distance is split over a chain: below 0.74*N for both.  Sum:
        N*(1 + 0.75 + 0.74) + T + 1 <= 3N + T + 1, the figure the two-pass
        kernel of fp32_bounds.py already has, so the online rescaling
        needs no term of its own.  log(s) adds T*u*|log s| <= T*u*ln N and
        m + log(s) one rounding of |lse|; all doubled.
  row   Brow = Blse + 2u*(|lse| + 2(1-eps)|x_t| + eps*sum|x_i|
                          + 3(eps/N)*sum|x_i|)
        (the subtraction; the product (1-eps)*x_t and its rounding; the
        N-term sum of x scaled by eps/N; the roundings of eps/N, of its
        product and of the second subtraction).  The smoothing terms are
        absent for eps = 0.  An ignored row is exactly 0.
  sum   sum Brow + 2B*u*sum|row|
  mean  the sum bound over the count, plus 2u*|loss| for the division
  gx    2*(p*((T+1)u + By) + 3u*|p - q| + 2u*q*[eps > 0])*|g|
        + 2^-126*|g|,
        with By = Blse + 2u*|x - lse| the error of the exponent, p the
        softmax, q = (1-eps)*onehot + eps/N and g the upstream gradient
        (over the count for "mean"; the division is one of the three
        roundings beside |p - q|).  This is the fused form of
        fp32_bounds.py with q for the one-hot, plus one term of its own:
        for eps > 0, q is computed in fp32 (a division and an addition,
        relative error 2u), which |p - q| does not cover where p is close
        to q.  And the flush: the hardware exp returns 0 for a subnormal
        p (below 2^-126) BEFORE the product with g, so the 2^-126 that
        every bound gets for a flushed result becomes 2^-126*|g| here
        (the "wide" regime has such p, with g = 3).  The plain 2^-126
        that fp32_bounds.within() adds to every bound, for a flush of the
        result itself, is still added on top.
        A -inf logit gives exactly 0; an ignored row exact zeros.

FusedSGD with weight decay wd and Nesterov momentum, reference
torch.optim.SGD on float64 copies, extending the SGD rows of fp32_bounds.py:
  g' = g + wd*p        Bg' = 2u*(|g| + |wd*p|)
  buf' = mu*buf + g'   Bb = 2u*(|mu*buf| + |g'|) + Bg'
  Nesterov direction d = g' + mu*buf'
                       Bd = 2u*(|g'| + |mu*buf'|) + Bg' + mu*Bb
  otherwise d = buf', Bd = Bb
  p' = p - lr*d        2u*(|p| + |lr*d|) + lr*Bd
lr = 3/64, mu = 1/2 and wd = 2^-7 are exact in fp32.
"""

import contextlib
import functools
import io
import itertools
import math

import torch
import torch.nn.functional as F

from fp32_bounds import (SGD_BIG, SGD_LR, T, TINY, U, _gen, _leaf,
                         _poison_free_blocks, sgd_sizes, within)
import fp32_bounds as fb

from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.optim import FusedSGD

# ---------------------------------------------------------------------------
# cross_entropy
# ---------------------------------------------------------------------------
WAVE_MAX_N = 2048       # csrc/cross_entropy.hip: above, a block per row
# every width at which the mapping changes, each with the width above it:
# the lanes per row double at 8, 16, ..., 512 (a full wave from 257 on) and
# the block per row starts above WAVE_MAX_N
XENT_THRESHOLDS = [8, 16, 32, 64, 128, 256, 512, WAVE_MAX_N]
THRESHOLD_N = sorted(n + d for n in XENT_THRESHOLDS for d in (0, 1))
# the issue's widths and both sides of every threshold
XENT_N = sorted(set([1, 2, 10, 63, 64, 65, 255, 257, 1000, 4097, 32771]
                    + THRESHOLD_N))
XENT_SHAPES = [(3, n) for n in XENT_N] + \
    [(b, n) for b in (1, 257) for n in (10, 1000)]
# the rows are never split and the grids are not capped: no B past a cap
XENT_REGIMES = ["randn", "wide", "offset", "neginf"]
XENT_EPS = [0.0, 0.125]
XENT_IGNORE_INDEX = [-100, 1]
XENT_IGNORED = ["none", "third", "all"]
XENT_REDUCTIONS = ["mean", "sum", "none"]
UPSTREAM = 3.0


@functools.lru_cache(maxsize=None)
def xent_inputs(shape, regime):
    """Logits, labels in [0, N) and the upstream vector for "none", made
    once per case and never modified."""
    B, N = shape
    g = _gen(B, N, XENT_REGIMES.index(regime), 21)
    x = torch.randn(B, N, generator=g)
    tgt = torch.randint(0, N, (B,), generator=g)
    if regime == "wide":
        x = 50.0 * x
    elif regime == "offset":
        x = x + 1e4
    elif regime == "neginf":
        x[:, 2::3] = float("-inf")       # column 0 stays finite
        tgt = torch.zeros(B, dtype=torch.int64)
    gvec = torch.randn(B, generator=g)
    return x, tgt, gvec


def xent_target(tgt, ignore_index, ignored):
    """The labels with the rows of the pattern set to ``ignore_index``.
    With the in-range index 1, rows that carry label 1 anyway are ignored
    too, as torch ignores them."""
    t = tgt.clone()
    if ignored == "third":
        t[::3] = ignore_index
    elif ignored == "all":
        t[:] = ignore_index
    return t


def xent_reference(x, t, gvec, eps, ignore_index, reduction):
    """float64 loss and gradient of F.cross_entropy, and their bounds."""
    B, N = x.shape
    xd = x.double().requires_grad_(True)
    loss = F.cross_entropy(xd, t, label_smoothing=eps,
                           ignore_index=ignore_index, reduction=reduction)
    keep = t != ignore_index
    count = int(keep.sum())
    if reduction == "none":
        loss.backward(gvec.double())
        g = gvec.double()[:, None]
    elif reduction == "mean" and count == 0:
        g = None                 # NaN loss; the gradient is all zeros
    else:
        (UPSTREAM * loss).backward()
        g = torch.full((B, 1), UPSTREAM / (count if reduction == "mean"
                                           else 1), dtype=torch.float64)
    grad, xd = xd.grad, xd.detach()
    lse = torch.logsumexp(xd, dim=1)
    Blse = 2 * U * (3 * N + T + 1 + T * math.log(N) + lse.abs())
    ts = torch.where(keep, t, torch.zeros_like(t))
    x_t = xd[torch.arange(B), ts]
    Brow = Blse + 2 * U * (lse.abs() + 2 * (1 - eps) * x_t.abs())
    if eps:
        sa = xd.abs().sum(dim=1)
        Brow = Brow + 2 * U * (eps * sa + 3 * (eps / N) * sa)
    Brow = torch.where(keep, Brow, torch.zeros_like(Brow))
    row = F.cross_entropy(xd, t, label_smoothing=eps,
                          ignore_index=ignore_index, reduction="none")
    if reduction == "none":
        Bloss = Brow
    else:
        Bloss = Brow.sum() + 2 * B * U * row.abs().sum()
        if reduction == "mean" and count:
            Bloss = Bloss / count + 2 * U * loss.detach().abs()
    gx = Bgx = None
    if g is not None:
        y = xd - lse[:, None]
        fin = torch.isfinite(y)
        yf = torch.where(fin, y, torch.zeros_like(y))
        p = torch.where(fin, y.exp(), torch.zeros_like(y))
        By = torch.where(fin, Blse[:, None] + 2 * U * yf.abs(),
                         torch.zeros_like(y))
        q = torch.full((B, N), eps / N, dtype=torch.float64)
        q[torch.arange(B), ts] += 1 - eps
        Bgx = 2 * (p * ((T + 1) * U + By) + 3 * U * (p - q).abs()
                   + (2 * U * q if eps else 0.0)) * g.abs() \
            + TINY * g.abs()
        Bgx = torch.where(keep[:, None], Bgx, torch.zeros_like(Bgx))
        gx = grad
    return {"loss": loss.detach(), "Bloss": Bloss, "gx": gx, "Bgx": Bgx,
            "keep": keep, "count": count}


def xent_options(regime):
    eps_list = [0.0] if regime == "neginf" else XENT_EPS
    return itertools.product(eps_list, XENT_IGNORE_INDEX, XENT_IGNORED,
                             XENT_REDUCTIONS)


def xent_run(x, t, gvec, eps, ignore_index, reduction, dev, dtype=None):
    """One forward and backward of the op under test; returns the loss and
    gx on the CPU."""
    xt = x.to(dev) if dtype is None else x.to(dev).to(dtype)
    xt = xt.clone().requires_grad_(True)
    loss = ops.cross_entropy(xt, t.to(dev), label_smoothing=eps,
                             ignore_index=ignore_index, reduction=reduction)
    assert loss.dtype == torch.float32
    assert loss.shape == ((x.shape[0],) if reduction == "none" else ())
    _poison_free_blocks(dev, x.numel())
    if reduction == "none":
        loss.backward(gvec.to(dev))
    else:
        (UPSTREAM * loss).backward()
    assert xt.grad.shape == x.shape and xt.grad.dtype == xt.dtype
    return loss.detach().cpu(), xt.grad.cpu()


def xent_case(shape, regime, dev):
    """Every option of one (shape, regime) against float64, within the
    bounds; prints the worst error/bound ratio of the case."""
    x, tgt, gvec = xent_inputs(shape, regime)
    worst = 0.0
    for eps, ii, ignored, reduction in xent_options(regime):
        t = xent_target(tgt, ii, ignored)
        ref = xent_reference(x, t, gvec, eps, ii, reduction)
        loss, gx = xent_run(x, t, gvec, eps, ii, reduction, dev)
        keep = ref["keep"]
        tag = f"{shape},{regime},eps={eps},ii={ii},{ignored},{reduction}"
        # ignored rows: stored zeros, whatever the allocator held
        assert bool((gx[~keep] == 0).all()), tag
        assert not bool(torch.signbit(gx[~keep]).any()), tag
        if reduction == "none":
            assert bool((loss[~keep] == 0).all()), tag
        if reduction == "mean" and ref["count"] == 0:
            assert bool(torch.isnan(loss)), tag
            assert bool(torch.isnan(ref["loss"])), tag
            assert bool((gx == 0).all()), tag
            continue
        assert bool(torch.isfinite(loss).all()), tag
        assert bool(torch.isfinite(gx).all()), tag
        if regime == "neginf":      # p is exactly 0 at a -inf logit
            assert bool((gx[:, 2::3] == 0).all()), tag
        with contextlib.redirect_stdout(io.StringIO()):
            worst = max(worst,
                        within(f"cross_entropy_{reduction}.loss[{tag}]",
                               loss, ref["loss"], ref["Bloss"]),
                        within(f"cross_entropy_gx.gx[{tag}]", gx, ref["gx"],
                               ref["Bgx"]))
    print(f"cross_entropy[{shape},{regime}]: worst error/bound = "
          f"{worst:.3f}")
    return worst


XENT_KEYS = ("cross_entropy_mean", "cross_entropy_sum", "cross_entropy_none",
             "cross_entropy_gx")


def xent_report():
    for op in XENT_KEYS:
        if op in fb.WORST:
            print(f"SUMMARY {op}: largest error/bound = {fb.WORST[op]:.3f}")
    assert all(fb.WORST[op] <= 1.0 for op in XENT_KEYS if op in fb.WORST)


# inputs the wrapper must refuse before anything is launched:
# (id, exception, needs a GPU, call(dev))
def _x(*shape, dev, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).to(dev)


def _t(*shape, dev, dtype=torch.int64):
    return torch.zeros(*shape, dtype=dtype).to(dev)


def _ce(x, t, **kw):
    return ops.cross_entropy(x, t, **kw)


XENT_VALIDATION = [
    ("rank-1", ValueError, False, lambda d: _ce(_x(10, dev=d), _t(10, dev=d))),
    ("rank-3", ValueError, False,
     lambda d: _ce(_x(4, 5, 2, dev=d), _t(4, dev=d))),
    ("no-rows", ValueError, False,
     lambda d: _ce(_x(0, 5, dev=d), _t(0, dev=d))),
    ("no-classes", ValueError, False,
     lambda d: _ce(_x(4, 0, dev=d), _t(4, dev=d))),
    ("logits-not-a-tensor", TypeError, False,
     lambda d: _ce([[0.0, 1.0]], _t(1, dev=d))),
    ("logits-int", TypeError, False,
     lambda d: _ce(_x(4, 5, dev=d, dtype=torch.int32), _t(4, dev=d))),
    ("target-length", ValueError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(3, dev=d))),
    ("target-rank", ValueError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, 1, dev=d))),
    ("target-soft", TypeError, False,
     lambda d: _ce(_x(4, 5, dev=d), _x(4, 5, dev=d))),
    ("target-int32", TypeError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d, dtype=torch.int32))),
    ("target-not-a-tensor", TypeError, False,
     lambda d: _ce(_x(2, 5, dev=d), [0, 1])),
    ("smoothing-negative", ValueError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d), label_smoothing=-0.1)),
    ("smoothing-above-one", ValueError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d), label_smoothing=1.5)),
    ("smoothing-nan", ValueError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d),
                   label_smoothing=float("nan"))),
    ("smoothing-bool", ValueError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d), label_smoothing=True)),
    ("smoothing-string", ValueError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d), label_smoothing="0.1")),
    ("ignore-index-float", TypeError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d), ignore_index=1.0)),
    ("ignore-index-bool", TypeError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d), ignore_index=True)),
    ("reduction-unknown", ValueError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d), reduction="batchmean")),
    ("reduction-none-object", ValueError, False,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev=d), reduction=None)),
    ("logits-fp16", TypeError, True,
     lambda d: _ce(_x(4, 5, dev=d, dtype=torch.float16), _t(4, dev=d))),
    ("logits-fp64", TypeError, True,
     lambda d: _ce(_x(4, 5, dev=d, dtype=torch.float64), _t(4, dev=d))),
    ("target-device", ValueError, True,
     lambda d: _ce(_x(4, 5, dev=d), _t(4, dev="cpu"))),
]


def xent_validation_cases(gpu):
    return [(i, e, c) for i, e, needs_gpu, c in XENT_VALIDATION
            if gpu or not needs_gpu]


# ---------------------------------------------------------------------------
# FusedSGD with weight decay and Nesterov momentum
# ---------------------------------------------------------------------------
SGD_MU = 0.5     # and 0 in decay_no_momentum_case
SGD_WD = 2.0 ** -7
# the size pattern of fp32_bounds.SGD_LISTS: 1, 33 and 70 tensors plus the
# long one past the grid cap, every 9th of those without a gradient
DECAY_LISTS = {
    "1": (sgd_sizes(1), None),
    "33": (sgd_sizes(33), None),
    "70+big": (sgd_sizes(70, big_at=40), 9),
}


def _decay_check(tag, ps, bufs, p0, b0, grads, nesterov):
    worst = 0.0
    mu, wd, lr = SGD_MU, SGD_WD, SGD_LR
    for i, (p, g) in enumerate(zip(ps, grads)):
        got_p, got_b = p.detach().cpu(), bufs[i].cpu()
        if g is None:           # skipped: untouched, bit for bit
            assert torch.equal(got_p, p0[i]), (tag, i)
            assert torch.equal(got_b, b0[i]), (tag, i)
            continue
        # torch.optim.SGD on float64 copies, one step from (p0, b0)
        pr = p0[i].double().clone().requires_grad_(True)
        ref = torch.optim.SGD([pr], lr=lr, momentum=mu, weight_decay=wd,
                              nesterov=nesterov)
        ref.state[pr]["momentum_buffer"] = b0[i].double().clone()
        pr.grad = g.double()
        ref.step()
        bref = ref.state[pr]["momentum_buffer"]
        gd, pd, bd = g.double(), p0[i].double(), b0[i].double()
        g1 = gd + wd * pd
        Bg = 2 * U * (gd.abs() + (wd * pd).abs())
        Bb = 2 * U * ((mu * bd).abs() + g1.abs()) + Bg
        if nesterov:
            d = g1 + mu * bref
            Bd = 2 * U * (g1.abs() + (mu * bref).abs()) + Bg + mu * Bb
        else:
            d, Bd = bref, Bb
        worst = max(worst,
                    within(f"sgd_decay.buf[{tag}]", got_b, bref, Bb),
                    within(f"sgd_decay.p[{tag}]", got_p, pr.detach(),
                           2 * U * (pd.abs() + (lr * d).abs()) + lr * Bd))
    return worst


def decay_case(which, nesterov, zero_grad, dev):
    sizes, none_every = DECAY_LISTS[which]
    g = _gen(len(sizes), nesterov, zero_grad, 13)
    has_grad = [none_every is None or i % none_every != none_every - 1
                for i in range(len(sizes))]
    assert has_grad[sizes.index(SGD_BIG)] if SGD_BIG in sizes else True
    ps = [torch.randn(n, generator=g).to(dev).requires_grad_(True)
          for n in sizes]
    opt = FusedSGD(ps, lr=SGD_LR, momentum=SGD_MU,
                   zero_grad_in_step=zero_grad, weight_decay=SGD_WD,
                   nesterov=nesterov)
    bufs = opt._bufs
    assert len(bufs) == len(ps)
    for b in bufs:
        b.copy_(torch.randn(b.shape, generator=g))
    worst = 0.0
    for step in range(2):
        # the second step continues from the device's own state
        p0 = [p.detach().cpu().clone() for p in ps]
        b0 = [b.cpu().clone() for b in bufs]
        grads = [torch.randn(n, generator=g) if h else None
                 for n, h in zip(sizes, has_grad)]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone().to(dev) if gr is not None else None
        opt.step()
        with contextlib.redirect_stdout(io.StringIO()):
            worst = max(worst, _decay_check(
                f"{which},nesterov={nesterov}", ps, bufs, p0, b0, grads,
                nesterov))
        for p, gr in zip(ps, grads):
            if gr is None:
                assert p.grad is None
            elif zero_grad:
                assert bool((p.grad == 0).all())
            else:
                assert torch.equal(p.grad.cpu(), gr)
    print(f"sgd_decay[{which},nesterov={nesterov},zero_grad={zero_grad}]: "
          f"worst error/bound = {worst:.3f}")
    assert worst <= 1.0


def decay_no_momentum_case(zero_grad, dev):
    """Weight decay without momentum (no buffers): p' = p - lr*(g + wd*p),
    within 2u*(|p| + |lr*g'|) + lr*Bg', two steps on the 33-tensor list."""
    sizes, _ = DECAY_LISTS["33"]
    g = _gen(len(sizes), zero_grad, 17)
    ps = [torch.randn(n, generator=g).to(dev).requires_grad_(True)
          for n in sizes]
    opt = FusedSGD(ps, lr=SGD_LR, momentum=0.0, zero_grad_in_step=zero_grad,
                   weight_decay=SGD_WD)
    assert opt._bufs is None
    worst = 0.0
    for step in range(2):
        p0 = [p.detach().cpu().clone() for p in ps]
        grads = [torch.randn(n, generator=g) for n in sizes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone().to(dev)
        opt.step()
        with contextlib.redirect_stdout(io.StringIO()):
            for p, a, gr in zip(ps, p0, grads):
                pr = a.double().clone().requires_grad_(True)
                ref = torch.optim.SGD([pr], lr=SGD_LR, momentum=0.0,
                                      weight_decay=SGD_WD)
                pr.grad = gr.double()
                ref.step()
                pd, gd = a.double(), gr.double()
                g1 = gd + SGD_WD * pd
                Bg = 2 * U * (gd.abs() + (SGD_WD * pd).abs())
                worst = max(worst, within(
                    "sgd_decay.p[mu=0]", p.detach().cpu(), pr.detach(),
                    2 * U * (pd.abs() + (SGD_LR * g1).abs()) + SGD_LR * Bg))
        for p, gr in zip(ps, grads):
            if zero_grad:
                assert bool((p.grad == 0).all())
            else:
                assert torch.equal(p.grad.cpu(), gr)
    print(f"sgd_decay[33,mu=0,zero_grad={zero_grad}]: worst error/bound = "
          f"{worst:.3f}")
    assert worst <= 1.0


def nan_case(N, dev, dtype=torch.float32):
    """An aligned chunk of 8 NaN logits, the target elsewhere: the row's
    loss is NaN, as in torch, and the other rows are untouched by it."""
    x, tgt, _ = xent_inputs((3, N), "randn")
    x = x.clone()
    lo = 8 if N >= 16 else 0
    x[1, lo:lo + 8] = float("nan")
    t = tgt.clone()
    t[1] = N - 1 if N > 8 else 0
    want = F.cross_entropy(x.double(), t, reduction="none")
    assert bool(torch.isnan(want[1])) and bool(torch.isfinite(want[::2]).all())
    got = ops.cross_entropy(x.to(dev).to(dtype), t.to(dev),
                            reduction="none").cpu()
    assert bool(torch.isnan(got[1])), N
    assert bool(torch.isfinite(got[::2]).all()), N
    mean = ops.cross_entropy(x.to(dev).to(dtype), t.to(dev)).cpu()
    assert bool(torch.isnan(mean)), N


NAN_N = [8, 64, 512, 1000, WAVE_MAX_N + 1]
