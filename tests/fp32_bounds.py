"""Float64 references, case lists and derived elementwise bounds for the
fp32 kernels of csrc/kernels.hip (conv2d, linear, log_softmax, nll_loss,
log_softmax_nll, sgd_step, add_inplace, reduce_columns, scale_f32), shared
by tests/test_fp32_kernels_cpu.py and tests/test_fp32_kernels_gpu.py; the
contract model of the three reduction helpers is also what
tests/test_xgmi_logic.py's FakeKernels runs.

Notation: u = 2^-24 (fp32 unit roundoff).  The project's rule: an fp32 sum
of L terms is within L*u*sum|terms|, doubled for summation order;
sum|terms| comes from running the float64 reference on absolute values.
Every bound gets 2^-126 added, because the GPU may flush a subnormal
result.  References are float64 on the same input values.

  conv y    2*(C*R*S+1)*u*conv(|x|, |w|, |b|)
  conv gx   2*K*R*S*u*conv_input(|w|, |gy|)
  conv gw   2*B*OH*OW*u*conv_weight(|x|, |gy|)
  conv gb   2*B*OH*OW*u*sum|gy|
  linear    the same with the summed dimension K+1 / N / B / B.  With the
            fused ReLU the forward bound holds as it is (ReLU is
            1-Lipschitz) and the gradient reference is masked with the
            op's OWN output (y > 0), as in the batchnorm tests.
  log_softmax y   By = 2u*(3N + T + 1 + T*ln N + |lse| + |y_ref|), where
                  y_ref is finite; a -inf entry must give -inf
  log_softmax gx  2*(p*2N*u*sum|g| + p*|S|*((T+1)u + By)
                     + 2u*(|g| + p*|S|)),  p = exp(y_ref), S = sum g
  fused gx        2*(p*((T+1)u + By) + 3u*|p - onehot|)/B, times the
                  upstream gradient (everything is linear in it)
  mean loss       mean By[target] + 2*B*u*mean|y_ref[target]|
  SGD buf'        Bb = 2u*(|mu*buf| + |g|)      (ref mu*buf + g)
  SGD p'          2u*(|p| + |lr*buf'|) + lr*Bb  (ref p - lr*buf')
  SGD, mu = 0     the same with buf' = g and Bb = 0
The SGD bounds exist because the device may contract to FMA, so bit
equality with the CPU formula is not required; lr and mu are chosen exactly
representable in fp32, so their conversion adds nothing.

The reduction helpers are held to their contract model bit for bit: the
order of additions is fixed and nothing can contract.
"""

import contextlib
import functools
import math

import torch
import torch.nn.functional as F

from dist_tuto_pth_amd import ops
from dist_tuto_pth_amd.optim import FusedSGD

U = 2.0 ** -24
TINY = 2.0 ** -126
# The one assumed number: the error constant of the hardware exp and log.
# One ulp (2u) per instruction, as AMD's ISA manual states for v_exp_f32 /
# v_log_f32, doubled for margin.  (__expf is exp2(log2e * x); the rounding
# of its argument is the "+1" beside T in the formulas.)
T = 4.0

WORST = {}      # op -> largest error/bound ratio seen in this process


def within(name, got, ref, bound):
    err = (got.detach().double().cpu() - ref).abs()
    bound = bound + TINY
    ratio = float((err / bound).max()) if err.numel() else 0.0
    print(f"{name}: worst error/bound = {ratio:.3f}")
    op = name.split(".")[0]
    WORST[op] = max(WORST.get(op, 0.0), ratio)
    assert bool((err <= bound).all()), \
        f"{name}: worst error/bound ratio {ratio:.3f}"
    return ratio


def report():
    for op in sorted(WORST):
        print(f"SUMMARY {op}: largest error/bound = {WORST[op]:.3f}")


def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 131 + int(v) + 7) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def _poison_free_blocks(dev, numel):
    """Fills the allocator's free blocks of this size with NaN, so that an
    output which a kernel only adds into, where it should store, cannot
    come out right by luck."""
    if torch.device(dev).type == "cuda":
        junk = [torch.full((numel,), float("nan"), device=dev)
                for _ in range(64)]
        del junk


def _leaf(t, dev):
    return None if t is None else t.clone().to(dev).requires_grad_(True)


# ---------------------------------------------------------------------------
# conv2d
# ---------------------------------------------------------------------------
CONV_SHAPES = [           # (B, C, H, W, K, R, S)
    (1, 1, 5, 5, 1, 5, 5),        # one output point, B = 1: plain-store gw
    (1, 2, 6, 7, 3, 3, 2),        # B = 1, R != S, H != W
    (3, 2, 7, 9, 3, 3, 2),        # the same filter, atomically added gw
    (2, 3, 6, 6, 4, 1, 1),        # 1x1 filter
    (5, 1, 9, 6, 2, 2, 5),        # S > R, wide filter
    (4, 3, 12, 12, 5, 5, 5),      # Net-like, more than one block
    (2, 16, 8, 7, 33, 6, 6),      # 76 KB of weights: the unstaged path
]


def conv_inputs(shape, bias):
    B, C, H, W, K, R, S = shape
    g = _gen(*shape, bias)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(K, C, R, S, generator=g)
    b = torch.randn(K, generator=g) if bias else None
    gy = torch.randn(B, K, H - R + 1, W - S + 1, generator=g)
    return x, w, b, gy


def conv_case(shape, bias, dev):
    B, C, H, W, K, R, S = shape
    OH, OW = H - R + 1, W - S + 1
    x, w, b, gy = conv_inputs(shape, bias)
    xd, wd, gd = x.double(), w.double(), gy.double()
    bd = b.double() if bias else None
    xa, wa, ga = xd.abs(), wd.abs(), gd.abs()

    xt, wt, bt = _leaf(x, dev), _leaf(w, dev), _leaf(b, dev)
    y = ops.conv2d(xt, wt, bt)
    assert y.shape == (B, K, OH, OW) and y.dtype == torch.float32
    within("conv2d.y", y, F.conv2d(xd, wd, bd),
           2 * (C * R * S + 1) * U
           * F.conv2d(xa, wa, bd.abs() if bias else None))
    gyt = gy.to(dev)
    _poison_free_blocks(dev, w.numel())
    y.backward(gyt)
    assert xt.grad.shape == x.shape and wt.grad.shape == w.shape
    within("conv2d.gx", xt.grad,
           torch.nn.grad.conv2d_input(x.shape, wd, gd),
           2 * K * R * S * U * torch.nn.grad.conv2d_input(x.shape, wa, ga))
    within("conv2d.gw", wt.grad,
           torch.nn.grad.conv2d_weight(xd, w.shape, gd),
           2 * B * OH * OW * U
           * torch.nn.grad.conv2d_weight(xa, w.shape, ga))
    if bias:
        assert bt.grad.shape == (K,)
        within("conv2d.gb", bt.grad, gd.sum(dim=(0, 2, 3)),
               2 * B * OH * OW * U * ga.sum(dim=(0, 2, 3)))


def _conv_grads(x, w, b, gy, dev):
    """One forward+backward; returns y, the gradients are on the leaves."""
    y = ops.conv2d(x, w, b)
    y.backward(gy.to(dev))
    return y.detach()


def _one_of(got, candidates):
    ok = torch.zeros(got.shape, dtype=torch.bool, device=got.device)
    for c in candidates:
        ok |= got == c
    return bool(ok.all())


NONCONTIG_CONV_SHAPE = (3, 2, 7, 9, 3, 3, 2)


def noncontig_conv_case(dev):
    """A channels-last weight and a strided bias give the results and
    gradients of their dense copies, bit for bit.  ``y`` and ``gx`` have a
    fixed order of operations.  On the GPU ``gw`` and ``gb`` are the sum of
    three per-sample partials in the order their atomic adds land, which
    is not fixed: there each element must equal, bit for bit, one of the
    three possible orders, built from the op's own B = 1 results (the
    plain-store branch, the same arithmetic per sample)."""
    shape = NONCONTIG_CONV_SHAPE
    B, K = shape[0], shape[4]
    x, w, b, gy = conv_inputs(shape, True)

    xa, wa, ba = _leaf(x, dev), _leaf(w, dev), _leaf(b, dev)
    ya = _conv_grads(xa, wa, ba, gy, dev)

    xb = _leaf(x, dev)
    wb = w.to(dev).to(memory_format=torch.channels_last).requires_grad_(True)
    assert not wb.is_contiguous()
    big = torch.zeros(2 * K, device=dev)
    big[::2] = b.to(dev)
    big.requires_grad_(True)
    bb = big[::2]
    assert not bb.is_contiguous()
    yb = _conv_grads(xb, wb, bb, gy, dev)

    assert torch.equal(ya, yb)
    assert torch.equal(xa.grad, xb.grad)
    # read through their own strides
    assert wb.grad.shape == w.shape and big.grad.shape == (2 * K,)
    assert torch.equal(big.grad[1::2], torch.zeros(K, device=dev))
    if torch.device(dev).type == "cpu":
        assert torch.equal(wa.grad, wb.grad)
        assert torch.equal(ba.grad, big.grad[::2])
    else:
        pw, pb = [], []
        for i in range(B):
            xi, wi, bi = _leaf(x[i:i + 1], dev), _leaf(w, dev), _leaf(b, dev)
            _conv_grads(xi, wi, bi, gy[i:i + 1], dev)
            pw.append(wi.grad)
            pb.append(bi.grad)
        for got_w, got_b in ((wa.grad, ba.grad), (wb.grad, big.grad[::2])):
            for got, p in ((got_w, pw), (got_b, pb)):
                orders = [(p[0] + p[1]) + p[2], (p[0] + p[2]) + p[1],
                          (p[1] + p[2]) + p[0]]
                assert _one_of(got, orders)
    # and against float64, so that "equal" cannot mean "equally wrong"
    xd, wd, gd = x.double(), w.double(), gy.double()
    within("conv2d.gw", wb.grad,
           torch.nn.grad.conv2d_weight(xd, w.shape, gd),
           2 * B * gy.shape[2] * gy.shape[3] * U
           * torch.nn.grad.conv2d_weight(xd.abs(), w.shape, gd.abs()))


# ---------------------------------------------------------------------------
# linear
# ---------------------------------------------------------------------------
LINEAR_SHAPES = [         # (B, K, N)
    (1, 1, 1),
    (3, 5, 7),            # K % 4 == 1
    (2, 6, 3),            # K % 4 == 2
    (5, 7, 2),            # K % 4 == 3
    (4, 8, 1),            # K % 4 == 0, N = 1
    (3, 129, 128),        # 66 KB of weights: unstaged, K % 4 == 1
    (4099, 3, 257),       # B*N > 4096*256: the grid-stride loop
    (64, 320, 50),        # Net's fc1
]


def linear_inputs(shape, bias, relu):
    B, K, N = shape
    g = _gen(*shape, bias, relu)
    x = torch.randn(B, K, generator=g)
    w = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g) if bias else None
    gy = torch.randn(B, N, generator=g)
    if relu:
        # pre-activations that are exactly zero: the whole of row 0
        # without a bias, entry [0, 0] with one
        if B > 1:
            x[0] = 0.0
        if bias:
            b[0] = 0.0
    return x, w, b, gy


def linear_case(shape, bias, relu, dev):
    B, K, N = shape
    x, w, b, gy = linear_inputs(shape, bias, relu)
    xd, wd, gd = x.double(), w.double(), gy.double()
    yref = xd @ wd.t()
    yabs = xd.abs() @ wd.abs().t()
    if bias:
        yref = yref + b.double()
        yabs = yabs + b.double().abs()
    if relu:
        yref = yref.clamp_min(0.0)

    xt, wt, bt = _leaf(x, dev), _leaf(w, dev), _leaf(b, dev)
    y = ops.linear(xt, wt, bt, fuse_relu=relu)
    assert y.shape == (B, N) and y.dtype == torch.float32
    within("linear.y", y, yref, 2 * (K + 1) * U * yabs)
    gyt = gy.to(dev)
    _poison_free_blocks(dev, w.numel())
    y.backward(gyt)

    g = gd
    if relu:
        yo = y.detach().cpu()
        g = gd * (yo > 0)
        if B > 1:
            zero = yo[0] if not bias else yo[0, :1]
            assert bool((zero == 0).all())
            if not bias:    # nothing of row 0 is active
                assert bool((xt.grad[0] == 0).all())
    ga = g.abs()
    assert xt.grad.shape == x.shape and wt.grad.shape == w.shape
    within("linear.gx", xt.grad, g @ wd, 2 * N * U * (ga @ wd.abs()))
    within("linear.gw", wt.grad, g.t() @ xd,
           2 * B * U * (ga.t() @ xd.abs()))
    if bias:
        assert bt.grad.shape == (N,)
        within("linear.gb", bt.grad, g.sum(0), 2 * B * U * ga.sum(0))


NONCONTIG_LINEAR_SHAPE = (2, 5, 7)     # two partials: any order, one sum


def noncontig_linear_case(dev):
    """``w = wt.t()`` over a dense ``wt`` [K,N] gives the results and
    gradients of its dense copy, bit for bit."""
    B, K, N = NONCONTIG_LINEAR_SHAPE
    x, w, b, gy = linear_inputs(NONCONTIG_LINEAR_SHAPE, True, False)
    for relu in (False, True):
        xa, wa, ba = _leaf(x, dev), _leaf(w, dev), _leaf(b, dev)
        ya = ops.linear(xa, wa, ba, fuse_relu=relu)
        ya.backward(gy.to(dev))

        xb, bb = _leaf(x, dev), _leaf(b, dev)
        wt = _leaf(w.t().contiguous(), dev)        # dense [K, N]
        wv = wt.t()
        assert wv.shape == (N, K) and not wv.is_contiguous()
        yb = ops.linear(xb, wv, bb, fuse_relu=relu)
        yb.backward(gy.to(dev))

        assert torch.equal(ya.detach(), yb.detach())
        assert torch.equal(xa.grad, xb.grad)
        assert torch.equal(ba.grad, bb.grad)
        assert wt.grad.shape == (K, N)
        assert torch.equal(wa.grad, wt.grad.t())
        if not relu:
            within("linear.gw", wt.grad.t(), gy.double().t() @ x.double(),
                   2 * B * U * (gy.double().abs().t() @ x.double().abs()))


# ---------------------------------------------------------------------------
# log_softmax, nll_loss, log_softmax_nll
# ---------------------------------------------------------------------------
SOFTMAX_SHAPES = [(1, 1), (1, 2), (3, 1000), (257, 10), (300, 17),
                  (1048579, 2)]       # the last: one row past the grid cap
REGIMES = ["randn", "wide", "offset", "neginf"]
UPSTREAM = 3.0      # (3*loss).backward(): the kernel reads it from memory


@functools.lru_cache(maxsize=None)
def softmax_reference(shape, regime):
    """Inputs and float64 references of one case, computed once and shared
    by the tests that use it (never modified)."""
    B, N = shape
    g = _gen(B, N, REGIMES.index(regime))
    x = torch.randn(B, N, generator=g)
    tgt = torch.randint(0, N, (B,), generator=g)
    if regime == "wide":
        x = 50.0 * x
    elif regime == "offset":
        x = x + 1e4
    elif regime == "neginf":
        x[:, 2::3] = float("-inf")       # column 0 stays finite
        tgt = torch.zeros(B, dtype=torch.int64)
    gy = torch.randn(B, N, generator=g)
    xd = x.double()
    lse = torch.logsumexp(xd, dim=1, keepdim=True)
    y = xd - lse
    fin = torch.isfinite(y)
    yf = torch.where(fin, y, torch.zeros_like(y))
    By = 2 * U * (3 * N + T + 1 + T * math.log(N) + lse.abs() + yf.abs())
    By = torch.where(fin, By, torch.zeros_like(By))
    p = torch.where(fin, y.exp(), torch.zeros_like(y))
    rows = torch.arange(B)
    onehot = torch.zeros(B, N, dtype=torch.float64)
    onehot[rows, tgt] = 1.0
    yt = y[rows, tgt]
    return {
        "x": x, "tgt": tgt, "gy": gy, "y": y, "fin": fin, "By": By, "p": p,
        "onehot": onehot,
        "loss": -yt.mean(),
        "Bloss": By[rows, tgt].mean() + 2 * B * U * yt.abs().mean(),
    }


def _logsoftmax_gx(ref, g):
    """float64 gradient of log_softmax for the upstream ``g`` [B,N], and
    its bound."""
    N = g.shape[1]
    p, By = ref["p"], ref["By"]
    S = g.sum(dim=1, keepdim=True)
    Sa = g.abs().sum(dim=1, keepdim=True)
    gx = g - p * S
    bound = 2 * (p * 2 * N * U * Sa + p * S.abs() * ((T + 1) * U + By)
                 + 2 * U * (g.abs() + p * S.abs()))
    return gx, bound


def _check_logp(name, logp, ref):
    got = logp.detach().cpu()
    fin = ref["fin"]
    # a -inf entry gives -inf, everything else is finite
    assert torch.equal(torch.isfinite(got), fin)
    assert bool((got[~fin] == float("-inf")).all())
    within(name, torch.where(fin, got, torch.zeros_like(got)),
           torch.where(fin, ref["y"], torch.zeros_like(ref["y"])),
           ref["By"])


def log_softmax_case(shape, regime, dev):
    ref = softmax_reference(shape, regime)
    xt = _leaf(ref["x"], dev)
    y = ops.log_softmax(xt)
    assert y.shape == shape and y.dtype == torch.float32
    _check_logp("log_softmax.y", y, ref)
    y.backward(ref["gy"].to(dev))
    gx, bound = _logsoftmax_gx(ref, ref["gy"].double())
    got = xt.grad.cpu()
    assert bool(torch.isfinite(got).all())
    # p is exactly 0 at a -inf entry: its gradient is the upstream one
    assert torch.equal(got[~ref["fin"]], ref["gy"][~ref["fin"]])
    within("log_softmax.gx", got, gx, bound)


def nll_loss_case(shape, regime, dev):
    """``nll_loss`` on ``log_softmax``'s output, then the whole chain back
    with a non-unit upstream gradient."""
    ref = softmax_reference(shape, regime)
    B = shape[0]
    xt = _leaf(ref["x"], dev)
    loss = ops.nll_loss(ops.log_softmax(xt), ref["tgt"].to(dev))
    assert loss.shape == () and loss.dtype == torch.float32
    within("nll_loss.loss", loss, ref["loss"], ref["Bloss"])
    (UPSTREAM * loss).backward()
    gx, bound = _logsoftmax_gx(ref, -UPSTREAM / B * ref["onehot"])
    got = xt.grad.cpu()
    assert bool(torch.isfinite(got).all())
    assert bool((got[~ref["fin"]] == 0).all())
    within("nll_loss.gx", got, gx, bound)


def log_softmax_nll_case(shape, regime, dev):
    ref = softmax_reference(shape, regime)
    B = shape[0]
    xt = _leaf(ref["x"], dev)
    loss = ops.log_softmax_nll(xt, ref["tgt"].to(dev))
    assert loss.shape == () and loss.dtype == torch.float32
    within("log_softmax_nll.loss", loss, ref["loss"], ref["Bloss"])
    (UPSTREAM * loss).backward()
    p, By = ref["p"], ref["By"]
    d = p - ref["onehot"]
    got = xt.grad.cpu()
    assert bool(torch.isfinite(got).all())
    assert bool((got[~ref["fin"]] == 0).all())
    within("log_softmax_nll.gx", got, d * (UPSTREAM / B),
           UPSTREAM * 2 * (p * ((T + 1) * U + By) + 3 * U * d.abs()) / B)


# ---------------------------------------------------------------------------
# FusedSGD
# ---------------------------------------------------------------------------
SGD_LR = 0.046875          # 3/64 and 1/2: exact in fp32, so converting
SGD_MOMENTA = [0.5, 0.0]   # them to float adds no error of its own
SGD_BIG = 4096 * 256 + 5   # longer than the capped grid of 4096 blocks
_SGD_CYCLE = (1, 3, 250, 257, 1024)


def sgd_sizes(count, big_at=None):
    sizes = [_SGD_CYCLE[i % len(_SGD_CYCLE)] for i in range(count)]
    if big_at is not None:
        sizes.insert(big_at, SGD_BIG)
    return sizes


# 70 small tensors and the long one, in the second launch's chunk; every
# 9th has no gradient, so the chunks of 32 do not fall on multiples of 32
SGD_LISTS = {
    "70+big": (sgd_sizes(70, big_at=40), 9),
    "32": (sgd_sizes(32), None),
    "33": (sgd_sizes(33), None),
}


def _sgd_check(tag, ps, bufs, p0, b0, grads, mu):
    """One step's result against float64 from (p0, b0, grads); returns the
    worst error/bound ratio."""
    worst = 0.0
    for i, (p, g) in enumerate(zip(ps, grads)):
        got_p = p.detach().cpu()
        got_b = bufs[i].cpu() if bufs is not None else None
        if g is None:           # skipped: untouched, bit for bit
            assert torch.equal(got_p, p0[i]), (tag, i)
            if bufs is not None:
                assert torch.equal(got_b, b0[i]), (tag, i)
            continue
        gd, pd = g.double(), p0[i].double()
        if bufs is not None:
            bref = mu * b0[i].double() + gd
            Bb = 2 * U * ((mu * b0[i].double()).abs() + gd.abs())
            worst = max(worst, within(f"sgd.buf[{tag}]", got_b, bref, Bb))
        else:
            bref, Bb = gd, 0.0
        worst = max(worst, within(
            f"sgd.p[{tag}]", got_p, pd - SGD_LR * bref,
            2 * U * (pd.abs() + (SGD_LR * bref).abs()) + SGD_LR * Bb))
    return worst


def sgd_case(which, mu, zero_grad, dev):
    sizes, none_every = SGD_LISTS[which]
    g = _gen(len(sizes), int(mu * 10), zero_grad)
    has_grad = [none_every is None or i % none_every != none_every - 1
                for i in range(len(sizes))]
    assert has_grad[sizes.index(SGD_BIG)] if SGD_BIG in sizes else True
    ps = [torch.randn(n, generator=g).to(dev).requires_grad_(True)
          for n in sizes]
    opt = FusedSGD(ps, lr=SGD_LR, momentum=mu, zero_grad_in_step=zero_grad)
    bufs = opt._bufs
    if mu != 0.0:
        assert len(bufs) == len(ps)
        for b in bufs:
            b.copy_(torch.randn(b.shape, generator=g))
    else:
        assert bufs is None
    worst = 0.0
    for step in range(2):
        # the second step continues from the device's own state
        p0 = [p.detach().cpu().clone() for p in ps]
        b0 = [b.cpu().clone() for b in bufs] if bufs is not None else None
        grads = [torch.randn(n, generator=g) if h else None
                 for n, h in zip(sizes, has_grad)]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone().to(dev) if gr is not None else None
        opt.step()
        with contextlib.redirect_stdout(None):    # one line per tensor
            worst = max(worst, _sgd_check(f"{which},mu={mu}", ps, bufs, p0,
                                          b0, grads, mu))
        for p, gr in zip(ps, grads):
            if gr is None:
                assert p.grad is None
            elif zero_grad:
                assert bool((p.grad == 0).all())
            else:
                assert torch.equal(p.grad.cpu(), gr)
    print(f"sgd[{which},mu={mu}]: worst error/bound = {worst:.3f}")


# ---------------------------------------------------------------------------
# the contract of the reduction helpers (csrc/kernels.hip, K14), on
# tensors.  tests/test_xgmi_logic.py's FakeKernels runs these, so the model
# the all-reduce algorithm tests trust is the one the kernels are held to.
# ---------------------------------------------------------------------------
NCCL_DTYPE = {torch.float32: 7, torch.bfloat16: 9}


def _f32_scalar(s):
    return torch.tensor(s, dtype=torch.float32)


def _round_once(acc, dtype):
    """fp32 to ``dtype``, rounded once to nearest even; a NaN becomes the
    quiet NaN 0x7fc0 in bf16, which is what the kernels store for the sum
    of a default NaN (0x7fc0, ``float("nan")``) and anything.  torch's own
    conversion on the CPU gives 0x7fc0 or 0xffff for it, depending on the
    host's vector instructions, so the model does not leave it to torch."""
    out = acc.to(dtype)
    if dtype == torch.bfloat16:
        out.view(torch.int16)[acc.isnan()] = 0x7FC0
    return out


def reduce_columns_model(dst, src, P, stride, n, scale):
    """``dst[j] = (dst[j] + sum_p src[p*stride + j]) * scale`` for j < n, in
    place on the 1-D tensors ``dst`` and ``src`` (fp32 or bf16): the sum
    runs in fp32 in the order p = 0..P-1, and the scaled result is rounded
    once to the element type."""
    acc = dst[:n].float()
    for p in range(P):
        acc = acc + src[p * stride:p * stride + n].float()
    dst[:n] = _round_once(acc * _f32_scalar(scale), dst.dtype)


def add_inplace_model(dst, src, n):
    """``dst[j] += src[j]`` for j < n: one fp32 add, rounded once."""
    dst[:n] = _round_once(dst[:n].float() + src[:n].float(), dst.dtype)


def scale_f32_model(dst, scale, n):
    """``dst[j] *= scale`` for j < n, fp32."""
    dst[:n] = dst[:n] * _f32_scalar(scale)


REDUCE_P = [0, 1, 7]
REDUCE_N = [1, 8, 1029]     # tail only; vectors only; vectors and a tail
REDUCE_SCALES = [1.0, 0.125]
REDUCE_OFFSET = 16          # elements in front of the destination
POINTWISE_N = [1, 7, 1029]


def reduce_values(n, dtype, gen):
    """Magnitudes in [0.5, 4) with random signs: every fp32 sum of two such
    bf16 values is exact.  The kernels add in fp32 and round once by
    construction, so exact sums are no longer required of the inputs
    (``rounding_case`` has the inexact ones); they are merely still
    tested."""
    mag = 0.5 + 3.5 * torch.rand(n, generator=gen)
    sign = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
    v = (mag * sign).to(dtype)
    a = v.float().abs()
    assert bool((a >= 0.5).all()) and bool((a <= 4.0).all())
    return v


def reduce_stride(n):
    return (n + 7) // 8 * 8 + 64


ROUNDING_N = 1029           # vectors and a tail
ROUNDING_P = [1, 7]
ROUNDING_NAN = (3, ROUNDING_N - 1)      # in a vector; in the tail


@functools.lru_cache(maxsize=None)
def rounding_case(P, scale=1.0):
    """bf16 inputs with plain ``randn`` values, whose fp32 sums do not fit
    bf16: the one rounding of the contract decides the stored bits, and a
    bf16 add per term or a second rounding would show.  ``P = None`` is
    ``add_inplace``, otherwise ``reduce_columns`` over P rows.  Two
    destination columns are NaN, one through ``dst`` and one through
    ``src``.  Returns (big, src, want, stride): the destination starts at
    ``big[REDUCE_OFFSET]``, and ``want`` is the model's result for ``big``.
    Computed once, shared and never modified."""
    n, off = ROUNDING_N, REDUCE_OFFSET
    stride = reduce_stride(n)
    g = _gen(n, -1 if P is None else P, int(scale * 8))
    big = torch.randn(off + n + off, generator=g).bfloat16()
    src = torch.randn((P or 1) * stride, generator=g).bfloat16()
    big[off + ROUNDING_NAN[0]] = float("nan")
    src[((P or 1) - 1) * stride + ROUNDING_NAN[1]] = float("nan")
    want = big.clone()
    if P is None:
        add_inplace_model(want[off:], src, n)
    else:
        reduce_columns_model(want[off:], src, P, stride, n, scale)
    return big, src, want, stride


# ---------------------------------------------------------------------------
# inputs the wrappers must refuse before anything is launched:
# (id, exception, needs a GPU, call(dev))
# ---------------------------------------------------------------------------
def _t(*shape, dev, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).to(dev)


def _tgt(*shape, dev, dtype=torch.int64):
    return torch.zeros(*shape, dtype=dtype).to(dev)


def _sgd_with(make):
    def call(dev):
        p, grad, buf = make(dev)
        p.requires_grad_(True)
        p.grad = grad
        opt = FusedSGD([p], lr=0.1, momentum=0.5)
        if buf is not None:
            opt._bufs[0] = buf
        opt.step()
    return call


VALIDATION = [
    ("conv2d-x-rank", ValueError, False, lambda d: ops.conv2d(
        _t(3, 8, 8, dev=d), _t(4, 3, 5, 5, dev=d))),
    ("conv2d-w-rank", ValueError, False, lambda d: ops.conv2d(
        _t(2, 3, 8, 8, dev=d), _t(4, 3, 25, dev=d))),
    ("conv2d-channels", ValueError, False, lambda d: ops.conv2d(
        _t(2, 3, 8, 8, dev=d), _t(4, 2, 5, 5, dev=d))),
    ("conv2d-bias-length", ValueError, False, lambda d: ops.conv2d(
        _t(2, 3, 8, 8, dev=d), _t(4, 3, 5, 5, dev=d), _t(5, dev=d))),
    ("conv2d-bias-rank", ValueError, False, lambda d: ops.conv2d(
        _t(2, 3, 8, 8, dev=d), _t(4, 3, 5, 5, dev=d), _t(4, 1, dev=d))),
    ("conv2d-filter-too-tall", ValueError, False, lambda d: ops.conv2d(
        _t(2, 3, 4, 8, dev=d), _t(4, 3, 5, 5, dev=d))),
    ("conv2d-filter-too-wide", ValueError, False, lambda d: ops.conv2d(
        _t(2, 3, 8, 4, dev=d), _t(4, 3, 5, 5, dev=d))),
    ("conv2d-empty-batch", ValueError, False, lambda d: ops.conv2d(
        _t(0, 3, 8, 8, dev=d), _t(4, 3, 5, 5, dev=d))),
    ("conv2d-w-dtype", TypeError, True, lambda d: ops.conv2d(
        _t(2, 3, 8, 8, dev=d), _t(4, 3, 5, 5, dev=d, dtype=torch.float64))),
    ("conv2d-b-dtype", TypeError, True, lambda d: ops.conv2d(
        _t(2, 3, 8, 8, dev=d), _t(4, 3, 5, 5, dev=d),
        _t(4, dev=d, dtype=torch.bfloat16))),
    ("conv2d-w-device", ValueError, True, lambda d: ops.conv2d(
        _t(2, 3, 8, 8, dev=d), _t(4, 3, 5, 5, dev="cpu"))),
    ("linear-x-rank", ValueError, False, lambda d: ops.linear(
        _t(2, 3, 6, dev=d), _t(4, 6, dev=d))),
    ("linear-w-rank", ValueError, False, lambda d: ops.linear(
        _t(2, 6, dev=d), _t(24, dev=d))),
    ("linear-k", ValueError, False, lambda d: ops.linear(
        _t(2, 6, dev=d), _t(4, 5, dev=d))),
    ("linear-w-transposed", ValueError, False, lambda d: ops.linear(
        _t(2, 6, dev=d), _t(6, 4, dev=d))),
    ("linear-bias-length", ValueError, False, lambda d: ops.linear(
        _t(2, 6, dev=d), _t(4, 6, dev=d), _t(6, dev=d))),
    ("linear-bias-rank", ValueError, False, lambda d: ops.linear(
        _t(2, 6, dev=d), _t(4, 6, dev=d), _t(1, 4, dev=d))),
    ("linear-empty-batch", ValueError, False, lambda d: ops.linear(
        _t(0, 6, dev=d), _t(4, 6, dev=d))),
    ("linear-w-dtype", TypeError, True, lambda d: ops.linear(
        _t(2, 6, dev=d), _t(4, 6, dev=d, dtype=torch.bfloat16))),
    ("linear-b-dtype", TypeError, True, lambda d: ops.linear(
        _t(2, 6, dev=d), _t(4, 6, dev=d), _t(4, dev=d, dtype=torch.float64))),
    ("linear-b-device", ValueError, True, lambda d: ops.linear(
        _t(2, 6, dev=d), _t(4, 6, dev=d), _t(4, dev="cpu"))),
    ("log_softmax-rank-1", ValueError, False, lambda d: ops.log_softmax(
        _t(10, dev=d))),
    ("log_softmax-rank-3", ValueError, False, lambda d: ops.log_softmax(
        _t(2, 5, 2, dev=d))),
    ("log_softmax-no-classes", ValueError, False, lambda d: ops.log_softmax(
        _t(4, 0, dev=d))),
    ("nll_loss-rank", ValueError, False, lambda d: ops.nll_loss(
        _t(4, 5, 2, dev=d), _tgt(4, dev=d))),
    ("nll_loss-target-length", ValueError, False, lambda d: ops.nll_loss(
        _t(4, 10, dev=d), _tgt(5, dev=d))),
    ("nll_loss-target-rank", ValueError, False, lambda d: ops.nll_loss(
        _t(4, 10, dev=d), _tgt(4, 1, dev=d))),
    ("nll_loss-target-int32", TypeError, False, lambda d: ops.nll_loss(
        _t(4, 10, dev=d), _tgt(4, dev=d, dtype=torch.int32))),
    ("nll_loss-target-float", TypeError, False, lambda d: ops.nll_loss(
        _t(4, 10, dev=d), _tgt(4, dev=d, dtype=torch.float32))),
    ("nll_loss-target-device", ValueError, True, lambda d: ops.nll_loss(
        _t(4, 10, dev=d), _tgt(4, dev="cpu"))),
    ("log_softmax_nll-rank", ValueError, False,
     lambda d: ops.log_softmax_nll(_t(40, dev=d), _tgt(4, dev=d))),
    ("log_softmax_nll-target-length", ValueError, False,
     lambda d: ops.log_softmax_nll(_t(4, 10, dev=d), _tgt(3, dev=d))),
    ("log_softmax_nll-target-int32", TypeError, False,
     lambda d: ops.log_softmax_nll(_t(4, 10, dev=d),
                                   _tgt(4, dev=d, dtype=torch.int32))),
    ("log_softmax_nll-target-uint8", TypeError, False,
     lambda d: ops.log_softmax_nll(_t(4, 10, dev=d),
                                   _tgt(4, dev=d, dtype=torch.uint8))),
    ("log_softmax_nll-target-device", ValueError, True,
     lambda d: ops.log_softmax_nll(_t(4, 10, dev=d), _tgt(4, dev="cpu"))),
    ("sgd-param-strided", ValueError, True, _sgd_with(
        lambda d: (_t(6, 4, dev=d).t(), _t(4, 6, dev=d), None))),
    ("sgd-grad-strided", ValueError, True, _sgd_with(
        lambda d: (_t(4, 6, dev=d), _t(6, 4, dev=d).t(), None))),
    ("sgd-buffer-strided", ValueError, True, _sgd_with(
        lambda d: (_t(4, 6, dev=d), _t(4, 6, dev=d), _t(6, 4, dev=d).t()))),
    ("sgd-param-dtype", TypeError, True, _sgd_with(
        lambda d: (_t(4, 6, dev=d, dtype=torch.float64),
                   _t(4, 6, dev=d, dtype=torch.float64), None))),
    ("sgd-buffer-dtype", TypeError, True, _sgd_with(
        lambda d: (_t(4, 6, dev=d), _t(4, 6, dev=d),
                   _t(4, 6, dev=d, dtype=torch.bfloat16)))),
]


def validation_cases(gpu):
    return [(i, e, c) for i, e, needs_gpu, c in VALIDATION
            if gpu or not needs_gpu]


def validation_match(name):
    """What the message must name: the op."""
    op = name.split("-")[0]
    return "FusedSGD" if op == "sgd" else op
