"""GPU tests of ops.cross_entropy (K21, csrc/cross_entropy.hip): the cases
and derived bounds of tests/xent_bounds.py against F.cross_entropy in
float64 (shared with tests/test_cross_entropy_cpu.py, so the kernels answer
to the bounds the CPU golden path meets), the refused inputs, stored zeros
for ignored rows, bitwise reproducibility, independence of the pointer's
alignment, the bf16 op as the fp32 op on the same values, and graph
replay of the direct entry points."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fp32_bounds as fb
    import xent_bounds as xb
    from dist_tuto_pth_amd import ops
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
RED = {"none": 0, "mean": 1, "sum": 2}


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    k = load_native("_kernels")
    assert k.cross_entropy_wave_max_n() == xb.WAVE_MAX_N


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class Direct:
    """The native entry points on preallocated buffers, no autograd."""

    def __init__(self, x, t, eps, ii, reduction, gloss):
        self.k = load_native("_kernels")
        B, N = x.shape
        f32 = dict(device=DEV, dtype=torch.float32)
        self.x, self.t, self.gloss = x, t, gloss
        self.row = torch.full((B,), float("nan"), **f32)
        self.lse = torch.full((B,), float("nan"), **f32)
        self.loss = torch.full((1,), float("nan"), **f32)
        self.count = torch.full((1,), float("nan"), **f32)
        self.gx = torch.full_like(x, float("nan"))
        self.args = (B, N, eps, ii, RED[reduction],
                     x.dtype == torch.bfloat16, 0)

    def run(self):
        s = torch.cuda.current_stream().cuda_stream
        self.k.cross_entropy_fwd(
            self.x.data_ptr(), self.t.data_ptr(), self.row.data_ptr(),
            self.lse.data_ptr(), self.loss.data_ptr(),
            self.count.data_ptr(), *self.args, s)
        self.k.cross_entropy_bwd(
            self.x.data_ptr(), self.t.data_ptr(), self.lse.data_ptr(),
            self.count.data_ptr(), self.gloss.data_ptr(),
            self.gx.data_ptr(), *self.args, s)
        return self

    def results(self):
        return [v.clone() for v in (self.row, self.lse, self.loss,
                                    self.count, self.gx)]


def _inputs(B, N, ignored="third", ii=-100, dtype=torch.float32):
    x, tgt, gvec = xb.xent_inputs((B, N), "randn")
    t = xb.xent_target(tgt, ii, ignored)
    return x.to(DEV).to(dtype), t.to(DEV), gvec.to(DEV)


# ---------------------------------------------------------------------------
# bounds against float64, refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("regime", xb.XENT_REGIMES)
@pytest.mark.parametrize("shape", xb.XENT_SHAPES, ids=str)
def test_cross_entropy_bounds(shape, regime):
    assert xb.xent_case(shape, regime, DEV) <= 1.0


@pytest.mark.parametrize("case", xb.xent_validation_cases(gpu=True),
                         ids=lambda c: c[0])
def test_cross_entropy_refuses(case):
    name, exc, call = case
    with pytest.raises(exc, match=r"ops\.cross_entropy"):
        call(DEV)


def test_launchers_refuse():
    k = load_native("_kernels")
    x, t, _ = _inputs(3, 10)
    d = Direct(x, t, 0.0, -100, "mean", torch.ones(1, device=DEV))
    s = torch.cuda.current_stream().cuda_stream
    p = [v.data_ptr() for v in (d.x, d.t, d.row, d.lse, d.loss, d.count)]
    for bad in ((0, 10, 0.0, -100, 1, False, 0),     # B = 0
                (3, 0, 0.0, -100, 1, False, 0),      # N = 0
                (3, 10, 0.0, -100, 3, False, 0),     # reduction
                (3, 10, 0.0, -100, 1, False, 5)):    # mapping
        with pytest.raises(ValueError, match="cross_entropy_fwd"):
            k.cross_entropy_fwd(*p, *bad, s)
    with pytest.raises(ValueError, match="cross_entropy_fwd"):
        k.cross_entropy_fwd(0, *p[1:], 3, 10, 0.0, -100, 1, False, 0, s)
    with pytest.raises(ValueError, match="cross_entropy_bwd"):
        k.cross_entropy_bwd(p[0], p[1], p[3], p[5], d.gloss.data_ptr(), 0,
                            3, 10, 0.0, -100, 1, False, 0, s)
    torch.cuda.synchronize()
    assert bool(torch.isnan(d.row).all())      # nothing was launched


# ---------------------------------------------------------------------------
# ignored rows: stored zeros
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [10, 1000, xb.WAVE_MAX_N + 1])
def test_ignored_rows_are_stored_zeros(N, dtype):
    """The upstream gradient is NaN: 0 * g would be NaN, a store is 0."""
    B = 7
    x, t, _ = _inputs(B, N, dtype=dtype)
    keep = (t != -100).cpu()
    for reduction in ("mean", "sum", "none"):
        xt = x.clone().requires_grad_(True)
        loss = ops.cross_entropy(xt, t, label_smoothing=0.125,
                                 reduction=reduction)
        fb._poison_free_blocks(DEV, B * N)
        loss.backward(torch.full_like(loss, float("nan")))
        gx = xt.grad.cpu()
        assert bool((_bits(gx[~keep]) == 0).all())
        assert bool(torch.isnan(gx[keep]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", xb.NAN_N)
def test_nan_logits_reach_the_loss(N, dtype):
    xb.nan_case(N, DEV, dtype)


# ---------------------------------------------------------------------------
# bitwise properties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(257, 10), (64, 1000), (5, 4097)],
                         ids=str)
def test_two_runs_are_bitwise_equal(shape, dtype):
    x, t, gvec = _inputs(*shape, dtype=dtype)
    for reduction, gl in (("mean", torch.full((1,), 3.0, device=DEV)),
                          ("none", gvec)):
        a = Direct(x, t, 0.125, -100, reduction, gl).run().results()
        fb._poison_free_blocks(DEV, x.numel())
        b = Direct(x, t, 0.125, -100, reduction, gl).run().results()
        torch.cuda.synchronize()
        for u, v in zip(a, b):
            assert torch.equal(_bits(u), _bits(v))
        assert bool(torch.isfinite(a[0]).all())
        assert bool(torch.isfinite(a[4].float()).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [8, 1000, 1024, xb.WAVE_MAX_N + 8, 4097])
def test_offset_view_gives_the_bits_of_its_aligned_clone(N, dtype):
    """A contiguous view one element into a buffer takes the element-wise
    path; the order of the reduction does not depend on it."""
    B = 5
    x, t, gvec = _inputs(B, N, dtype=dtype)
    buf = torch.zeros(B * N + 1, device=DEV, dtype=dtype)
    view = buf[1:].view(B, N)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    assert x.data_ptr() % 16 == 0
    gbuf = torch.full((B * N + 1,), float("nan"), device=DEV, dtype=dtype)
    for reduction, gl in (("mean", torch.full((1,), 3.0, device=DEV)),
                          ("none", gvec)):
        a = Direct(x, t, 0.125, -100, reduction, gl).run()
        b = Direct(view, t, 0.125, -100, reduction, gl)
        b.gx = gbuf[1:].view(B, N)
        b.run()
        for u, v in zip(a.results(), b.results()):
            assert torch.equal(_bits(u), _bits(v.contiguous()))
        # through autograd as well
        xa = x.clone().requires_grad_(True)
        xv = view.detach().requires_grad_(True)
        la = ops.cross_entropy(xa, t, label_smoothing=0.125,
                               reduction=reduction)
        lv = ops.cross_entropy(xv, t, label_smoothing=0.125,
                               reduction=reduction)
        assert _same_bits(la.detach(), lv.detach())
        la.backward(gl if reduction == "none" else gl[0])
        lv.backward(gl if reduction == "none" else gl[0])
        assert _same_bits(xa.grad, xv.grad)


@pytest.mark.parametrize("eps", [0.0, 0.125])
@pytest.mark.parametrize("N", [10, 1000] + xb.THRESHOLD_N)
def test_bf16_is_the_fp32_op_on_the_same_values(N, eps):
    """row and lse bit for bit; gx the fp32 gx rounded once (RNE)."""
    B = 5
    xh, t, gvec = _inputs(B, N, dtype=torch.bfloat16)
    xf = xh.float()
    for reduction, gl in (("mean", torch.full((1,), 3.0, device=DEV)),
                          ("sum", torch.full((1,), 3.0, device=DEV)),
                          ("none", gvec)):
        h = Direct(xh, t, eps, -100, reduction, gl).run().results()
        f = Direct(xf, t, eps, -100, reduction, gl).run().results()
        assert _same_bits(h[0], f[0])          # row
        assert _same_bits(h[1], f[1])          # lse
        if reduction != "none":
            assert _same_bits(h[2], f[2]) and _same_bits(h[3], f[3])
        assert h[4].dtype == torch.bfloat16
        assert _same_bits(h[4], f[4].to(torch.bfloat16))
        assert bool(torch.isfinite(f[4]).all())


def test_forced_mappings_agree_within_bounds():
    """The `mapping` override (used only to measure the threshold) runs
    the other kernel on the same rows: same loss within the row bound."""
    x, t, gvec = _inputs(5, 1000)
    rows = []
    for mapping in (1, 2):
        d = Direct(x, t, 0.0, -100, "none", gvec)
        d.args = d.args[:-1] + (mapping,)
        rows.append(d.run().results())
    ref = xb.xent_reference(x.cpu(), t.cpu(), gvec.cpu(), 0.0, -100, "none")
    for r in rows:
        fb.within("cross_entropy_none.mapping", r[0], ref["loss"],
                  ref["Bloss"])
        fb.within("cross_entropy_gx.mapping", r[4], ref["gx"], ref["Bgx"])


# ---------------------------------------------------------------------------
# graph replay
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graph_replay_matches_eager(dtype):
    B, N = 64, 1000
    x, t, _ = _inputs(B, N, ignored="none", dtype=dtype)
    x, t = x.clone(), t.clone()
    gl = torch.full((1,), 3.0, device=DEV)
    cap = Direct(x, t, 0.125, -100, "mean", gl)
    # warm-up on a side stream, then capture on one stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.run()
    for every, seed in ((3, 1), (2, 2)):
        g = torch.Generator().manual_seed(seed)
        x.copy_(torch.randn(B, N, generator=g).to(dtype))
        nt = torch.randint(0, N, (B,), generator=g)
        nt[::every] = -100
        t.copy_(nt)
        for v in (cap.row, cap.lse, cap.loss, cap.count, cap.gx):
            v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = cap.results()
        want = Direct(x, t, 0.125, -100, "mean", gl).run().results()
        for u, v in zip(got, want):
            assert torch.equal(_bits(u), _bits(v))
        assert float(got[3]) == B - len(range(0, B, every))
        assert bool(torch.isfinite(got[2]).all())


def test_zz_report_ratios():
    """Prints the largest error/bound ratio per quantity of this run."""
    xb.xent_report()
