"""Weight-gradient tiles (fp32-MFMA conv1/conv2 implicit GEMMs + the fc
tiles) driven through the raw partial + combine launches on hand-made
workspaces, against a float64 CPU reference."""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dist_tuto_pth_amd.models import Net
    from dist_tuto_pth_amd.ops import _stream
    from dist_tuto_pth_amd.ops.fused import net_fused_step
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
C1_SUBS = 8                 # conv1 sub-blocks (bands of 3 output rows)
T_ALL = 8 + C1_SUBS + 63 + 2  # conv2 | conv1 | fc1 | fc2 tiles
GW_ROW = 21840 + (C1_SUBS - 1) * 260  # partial row + conv1 extension
NAMES = ["conv1.w", "conv1.b", "conv2.w", "conv2.b",
         "fc1.w", "fc1.b", "fc2.w", "fc2.b"]
SHAPES = [(10, 1, 5, 5), (10,), (20, 10, 5, 5), (20,),
          (50, 320), (50,), (10, 50), (10,)]


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


def _inputs(B, integer, seed):
    g = torch.Generator().manual_seed(seed)
    dims = {"x": (B, 28, 28), "p1": (B, 10, 12, 12), "ga1": (B, 10, 24, 24),
            "ga2": (B, 20, 8, 8), "p2": (B, 320), "gh1": (B, 50),
            "d3": (B, 50), "glog": (B, 10)}
    out = {}
    for name, shp in dims.items():
        if integer:
            # seeded, position-dependent, asymmetric small integers
            out[name] = torch.randint(-3, 4, shp, generator=g).float()
        else:
            out[name] = torch.randn(shp, generator=g)
    return out


def _reference(t):
    """float64 gradients and S = sum |a*b| per element, all 8 tensors."""
    d = {k: v.double() for k, v in t.items()}
    xu = d["x"].unfold(1, 24, 1).unfold(2, 24, 1)        # [B,5,5,24,24]
    pu = d["p1"].unfold(2, 8, 1).unfold(3, 8, 1)         # [B,10,5,5,8,8]

    def grads(ga1, xu_, ga2, pu_, gh1, p2, glog, d3):
        return [
            torch.einsum("bkhw,brshw->krs", ga1, xu_).reshape(10, 1, 5, 5),
            ga1.sum((0, 2, 3)),
            torch.einsum("bkhw,bcrshw->kcrs", ga2, pu_),
            ga2.sum((0, 2, 3)),
            gh1.t() @ p2, gh1.sum(0), glog.t() @ d3, glog.sum(0)]

    ref = grads(d["ga1"], xu, d["ga2"], pu, d["gh1"], d["p2"], d["glog"],
                d["d3"])
    mag = grads(d["ga1"].abs(), xu.abs(), d["ga2"].abs(), pu.abs(),
                d["gh1"].abs(), d["p2"].abs(), d["glog"].abs(),
                d["d3"].abs())
    return ref, mag


def _run_gpu(t, B, nch, nch1, nch2):
    k = load_native("_kernels")
    w = {n: v.to(DEV).contiguous() for n, v in t.items()}
    # NaN-filled partial rows: any slot the tiles fail to write poisons
    # the combine's output
    part = torch.full((32, GW_ROW), float("nan"), device=DEV)
    grads = [torch.full(s, float("nan"), device=DEV) for s in SHAPES]
    bchunk = -(-B // nch)
    bchunk1 = -(-B // nch1)
    bchunk2 = -(-B // nch2)
    s = _stream()
    k.net_gw_partial_raw(
        w["x"].data_ptr(), w["p1"].data_ptr(), w["p2"].data_ptr(),
        w["d3"].data_ptr(), w["ga1"].data_ptr(), w["ga2"].data_ptr(),
        w["gh1"].data_ptr(), w["glog"].data_ptr(), part.data_ptr(), B,
        bchunk, bchunk1, bchunk2, 0, T_ALL, nch, nch1, nch2, s)
    k.net_gw_combine_raw(part.data_ptr(), [g.data_ptr() for g in grads],
                         nch, nch1, nch2, s)
    torch.cuda.synchronize()
    return [g.cpu() for g in grads], (bchunk, bchunk1, bchunk2)


@pytest.mark.parametrize("B,nch,nch1,nch2", [
    (7, 3, 3, 3),     # short last chunk: 3, 3, 1
    (5, 4, 4, 4),     # bchunk=2, row 3 starts past B (empty tail row)
    (12, 2, 3, 4),    # each family folds its own row count
    (40, 2, 2, 2),    # bchunk=20 > 16: the former large-chunk regime
    (1, 1, 1, 1),     # no remainder
])
def test_gw_integer_layout_exact(B, nch, nch1, nch2):
    """Small asymmetric integers: every partial sum is far below 2^24,
    so fp32 is exact in any order and all eight gradients must be
    BIT-equal to the float64 reference — a swapped (k,c,r,s), a
    transposed r/s or a shifted window changes the answer."""
    t = _inputs(B, True, 100 + B)
    ref, mag = _reference(t)
    assert max(float(m.max()) for m in mag) < 2 ** 22
    got, _ = _run_gpu(t, B, nch, nch1, nch2)
    for name, g, r in zip(NAMES, got, ref):
        print(name, "max |diff|", float((g.double() - r).abs().max()))
        assert torch.equal(g, r.float()), name


def test_gw_random_forward_bound():
    """Standard-normal inputs, B=24 in 4 chunks of 6: |gpu - ref| <=
    n*u*S per element, u = 2^-24, S = sum|a*b| (float64), n = additions
    in the longest chain the element can see:
      conv2: one wave folds 16 of a sample's 64 positions into its
             accumulator per sample (16*bchunk2 fmas), the 4 K-slices
             are summed in 2 steps, then nch2 partial rows;
      conv1: a sub-block owns `rows` output rows; its (sample,row) pairs
             go round-robin to 4 waves, 6 MFMA steps each, then 2
             cross-wave steps, then nch1*8 partial rows;
      fc:    bchunk terms per chunk, then nch rows."""
    B, nch = 24, 4
    t = _inputs(B, False, 7)
    ref, mag = _reference(t)
    got, (bchunk, bchunk1, bchunk2) = _run_gpu(t, B, nch, nch, nch)
    rows = 24 // C1_SUBS
    n_c2 = 16 * bchunk2 + 2 + nch
    n_c1 = 6 * math.ceil(bchunk1 * rows / 4) + 2 + nch * C1_SUBS
    n_fc = bchunk + nch
    ns = [n_c1, n_c1, n_c2, n_c2, n_fc, n_fc, n_fc, n_fc]
    u = 2.0 ** -24
    for name, g, r, m, n in zip(NAMES, got, ref, mag, ns):
        err = (g.double() - r).abs()
        bound = n * u * m
        print(name, "n", n, "max err", float(err.max()),
              "max err/bound", float((err / bound).max()))
        assert bool((err <= bound).all()), name


@pytest.mark.parametrize("B", [6, 33])
def test_fused_step_default_chunks_match_cpu(B):
    """End-to-end eval-mode step at the default chunk counts vs the CPU
    autograd reference (guards the wiring of the chunk defaults)."""
    torch.manual_seed(40 + B)
    net_c = Net().eval()
    net_g = Net().eval().to(DEV)
    net_g.load_state_dict({k: v.to(DEV)
                           for k, v in net_c.state_dict().items()})
    x = torch.randn(B, 1, 28, 28)
    tgt = torch.randint(0, 10, (B,))
    F.nll_loss(net_c(x), tgt).backward()
    net_fused_step(net_g, x.to(DEV), tgt.to(DEV))
    torch.cuda.synchronize()
    for (n, pc), pg in zip(net_c.named_parameters(), net_g.parameters()):
        d = (pg.grad.cpu() - pc.grad).abs().max()
        print(n, float(d))
        assert torch.allclose(pg.grad.cpu(), pc.grad, atol=5e-4), (n, d)
