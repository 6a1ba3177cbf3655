"""The operand staging of the tiled Net kernels (the prologues of the
tiled forward and data backward, the per-round idx1 prefetch and the
batched fc tiles of the partial weight-gradient kernel) on integer data.

Every value is a small integer and every sum stays below 2^24, so fp32
arithmetic is exact in any order and the kernels must equal a float64
reference bit for bit: a staged element that lands in the wrong slot, is
dropped or is read from the wrong address changes an integer.  No
tolerance anywhere.
"""

import functools

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


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _offset_by_one(t):
    """A copy of t whose first element sits 4 bytes past a 16-byte
    boundary: a view at element 1 of a larger buffer."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---- backward staging ----------------------------------------------------

def _route_pool(g, idx):
    """Max-pool backward by the kernels' index bytes: slot = low two bits,
    bit 2 = dead.  [B,C,H,W] -> [B,C,2H,2W]."""
    Bn, C, H, W = g.shape
    out = torch.zeros(Bn, C, 2 * H, 2 * W, dtype=torch.float64)
    v = torch.where((idx & 4) == 0, g, torch.zeros_like(g))
    am = (idx & 3).long()
    for slot in range(4):
        out[:, :, slot >> 1::2, slot & 1::2] = torch.where(
            am == slot, v, torch.zeros_like(v))
    return out


@functools.lru_cache(maxsize=None)
def _bwd_case(B):
    g = torch.Generator().manual_seed(5100 + B)
    ga2 = _ints(g, -3, 3, B, 1280)
    idx1 = torch.randint(0, 8, (B, 1440), generator=g, dtype=torch.uint8)
    w2 = _ints(g, -2, 2, 20, 10, 5, 5)
    ref = torch.nn.grad.conv2d_input((B, 10, 12, 12), w2.double(),
                                     ga2.double().view(B, 20, 8, 8))
    # |sum| <= 500 * 3 * 2, far below 2^24
    ref = _route_pool(ref, idx1.view(B, 10, 12, 12)).view(B, 5760)
    return ga2, idx1, w2, ref


def _run_bwd(B, w2_dev):
    k = load_native("_kernels")
    ga2, idx1, _, _ = _bwd_case(B)
    ws = fused._ws(B, DEV)
    ws["ga2"].copy_(ga2)
    ws["idx1"].copy_(idx1)
    ws["ga1"].fill_(float("nan"))
    tgt = torch.zeros(B, dtype=torch.int64, device=DEV)
    wf1 = torch.zeros(50, 320, device=DEV)
    wf2 = torch.zeros(10, 50, device=DEV)
    # head_done: the kernel reads w2, ga2 and idx1 only
    k.net_bwd_data_raw(w2_dev.data_ptr(), wf1.data_ptr(), wf2.data_ptr(),
                       tgt.data_ptr(),
                       ws["one"].data_ptr(), ws.ptrs, B, False,
                       ops._stream(), head_done=True)
    torch.cuda.synchronize()
    return ws["ga1"].cpu().clone()


@pytest.mark.parametrize("split", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_backward_staging_exact_integers(B, split, monkeypatch):
    """ga1 from ga2, idx1 and w2 alone, every sibling split: all 5760
    values per sample against conv_transpose2d + the pool1 routing."""
    monkeypatch.setenv("DTP_BWD_SPLIT", str(split))
    _, _, w2, ref = _bwd_case(B)
    got = _run_bwd(B, w2.to(DEV))
    assert float(ref.abs().sum()) > 0
    assert torch.equal(got.double(), ref)


@pytest.mark.parametrize("split", [1, 2])
def test_backward_staging_unaligned_w2(split, monkeypatch):
    """w2 4 bytes past a 16-byte boundary: the aligned run's bits."""
    monkeypatch.setenv("DTP_BWD_SPLIT", str(split))
    B = 3
    _, _, w2, ref = _bwd_case(B)
    aligned = _run_bwd(B, w2.to(DEV))
    got = _run_bwd(B, _offset_by_one(w2.to(DEV)))
    assert torch.equal(got, aligned)
    assert torch.equal(got.double(), ref)


# ---- forward staging -----------------------------------------------------

def _pool_first_max(a):
    """The kernels' 2x2 pool + ReLU: the first maximum in window order
    wins, bit 2 of the index byte is set when the maximum is not positive.
    [B,C,2H,2W] float64 -> (pooled, index bytes)."""
    Bn, C, H2, W2 = a.shape
    w = a.view(Bn, C, H2 // 2, 2, W2 // 2, 2).permute(0, 1, 2, 4, 3, 5)
    w = w.reshape(Bn, C, H2 // 2, W2 // 2, 4)
    m = w[..., 0].clone()
    am = torch.zeros_like(m, dtype=torch.int64)
    for s in range(1, 4):
        gt = w[..., s] > m
        m = torch.where(gt, w[..., s], m)
        am = torch.where(gt, torch.full_like(am, s), am)
    idx = torch.where(m > 0, am, am | 4).to(torch.uint8)
    return m.clamp_min(0.0), idx


@functools.lru_cache(maxsize=None)
def _fwd_case(B):
    g = torch.Generator().manual_seed(6200 + B)
    x = _ints(g, -2, 2, B, 1, 28, 28)
    prm = [_ints(g, -1, 1, 10, 1, 5, 5), _ints(g, -2, 2, 10),
           _ints(g, -1, 1, 20, 10, 5, 5), _ints(g, -2, 2, 20),
           _ints(g, -1, 1, 50, 320), _ints(g, -2, 2, 50),
           _ints(g, -1, 1, 10, 50), _ints(g, -2, 2, 10)]
    tgt = torch.randint(0, 10, (B,), generator=g)
    d = [p.double() for p in prm]
    conv = torch.nn.functional.conv2d
    p1, idx1 = _pool_first_max(conv(x.double(), d[0], d[1]))
    p2, idx2 = _pool_first_max(conv(p1, d[2], d[3]))
    h1 = (p2.view(B, 320) @ d[4].t() + d[5]).clamp_min(0.0)
    assert float(h1.abs().max()) < 2 ** 24      # about 4.1e6 at the most
    ref = {"p1": p1.view(B, 1440), "idx1": idx1.view(B, 1440),
           "p2": p2.view(B, 320), "idx2": idx2.view(B, 320), "h1": h1}
    return x, prm, tgt, ref


FWD_READ = ("p1", "idx1", "p2", "idx2", "h1")


def _run_fwd(B, prm_dev, split, poll):
    k = load_native("_kernels")
    x, _, tgt, _ = _fwd_case(B)
    ws = fused._ws(B, DEV)
    for n in ("p1", "p2", "h1"):
        ws[n].fill_(float("nan"))
    for n in ("idx1", "idx2"):
        ws[n].fill_(255)
    xd, td = x.to(DEV), tgt.to(DEV)
    k.net_fwd_raw(xd.data_ptr(), fused._ptrs(prm_dev), td.data_ptr(),
                  ws.ptrs, ops._seed_ptr(DEV), B, False, True, split, poll,
                  ops._stream())
    torch.cuda.synchronize()
    return {n: ws[n].cpu().clone() for n in FWD_READ}


def _check_fwd(got, ref):
    for n in FWD_READ:
        a = got[n] if got[n].dtype == torch.uint8 else got[n].double()
        assert torch.equal(a, ref[n]), n


@pytest.mark.parametrize("split,poll", [(1, 60000), (2, 60000), (2, 0)])
@pytest.mark.parametrize("B", [1, 3])
def test_forward_staging_exact_integers(B, split, poll):
    """p1, idx1, p2, idx2 and h1 of the tiled forward, unsplit, split and
    with the hand-off's fallback forced, against float64.  Integer data
    makes pooling ties frequent: the tie rule is part of the check."""
    _, prm, _, ref = _fwd_case(B)
    _check_fwd(_run_fwd(B, [p.to(DEV) for p in prm], split, poll), ref)


@pytest.mark.parametrize("split", [1, 2])
def test_forward_staging_unaligned_weights(split):
    """Every weight pointer 4 bytes past a 16-byte boundary."""
    B = 3
    _, prm, _, ref = _fwd_case(B)
    aligned = _run_fwd(B, [p.to(DEV) for p in prm], split, 60000)
    got = _run_fwd(B, [_offset_by_one(p.to(DEV)) for p in prm], split, 60000)
    for n in FWD_READ:
        assert torch.equal(got[n], aligned[n]), n
    _check_fwd(got, ref)


# ---- several samples per workgroup ---------------------------------------

def test_grid_stride_workgroups_reload_x_and_ga2(monkeypatch):
    """B = 4099 is the smallest batch above the 4096-workgroup grid cap:
    three workgroups of each tiled kernel run a second sample after one
    prologue.  The step with the head in the forward (the no-head
    backward) against the step with DTP_HEAD_IN_FWD=0 (the head variant
    of the same body): loss and all 8 gradients bit for bit."""
    B = 4099
    monkeypatch.setenv("DTP_FWD_TILED", "1")
    monkeypatch.setenv("DTP_BWD_SPLIT", "1")
    g = torch.Generator().manual_seed(4099)
    net = Net()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    net = net.to(DEV).eval()
    x = torch.randn(B, 1, 28, 28, generator=g).to(DEV)
    tgt = torch.randint(0, 10, (B,), generator=g).to(DEV)
    got = {}
    for head in ("1", "0"):
        monkeypatch.setenv("DTP_HEAD_IN_FWD", head)
        for p in net.parameters():
            p.grad = None
        loss = fused.net_fused_step(net, x, tgt).clone()
        torch.cuda.synchronize()
        got[head] = [loss.cpu()] + [p.grad.cpu().clone()
                                    for p in net.parameters()]
    assert len(got["1"]) == 9
    assert bool(torch.isfinite(got["1"][0]))
    for i, (a, b) in enumerate(zip(got["1"], got["0"])):
        assert float(a.abs().sum()) > 0, i
        assert torch.equal(a, b), (i, (a - b).abs().max().item())


# ---- fc tiles of the partial weight-gradient kernel ----------------------

# the partial rows are laid out like the flat gradient: conv1.w, conv1.b,
# conv2.w, conv2.b, fc1.w, fc1.b, fc2.w, fc2.b
OFF_WF1 = 250 + 10 + 5000 + 20
OFF_BF1 = OFF_WF1 + 16000
OFF_WF2 = OFF_BF1 + 50
OFF_BF2 = OFF_WF2 + 500


@pytest.mark.parametrize("B,nch,bchunk", [
    (5, 1, 5), (5, 5, 1),               # 5 and 1 samples per block
    (9, 1, 9), (9, 5, 2),               # 9 = a full batch of 8 + 1; 2, 1
    (100, 1, 100), (100, 5, 20),        # several batches and a tail of 4
    (100, 16, 7),                       # 7, a row of 2 and an empty row
    (100, 16, 8),                       # exactly 8, 4 and three empty rows
])
def test_fc_tiles_exact_integers(B, nch, bchunk):
    """The fc1 and fc2 segments of net_gw_partial_kernel on integer
    workspaces: every partial row against the float64 sums over that
    row's samples (an empty row is all zeros)."""
    k = load_native("_kernels")
    tiles = dict(k.gw_tiles)
    base_fc1 = tiles["conv2"] + tiles["conv1"]
    g = torch.Generator().manual_seed(7300 + 100 * B + nch)
    ws = fused._ws(B, DEV)
    src = {n: _ints(g, -3, 3, *ws[n].shape) for n in ("gh1", "p2", "glog",
                                                      "d3")}
    for n, t in src.items():
        ws[n].copy_(t)
    ws["part"].fill_(float("nan"))
    x = torch.zeros(B, 1, 28, 28, device=DEV)
    for base, nt in ((base_fc1, tiles["fc1"]),
                     (base_fc1 + tiles["fc1"], tiles["fc2"])):
        k.net_gw_partial_raw(
            x.data_ptr(), ws["p1"].data_ptr(), ws["p2"].data_ptr(),
            ws["d3"].data_ptr(), ws["ga1"].data_ptr(), ws["ga2"].data_ptr(),
            ws["gh1"].data_ptr(), ws["glog"].data_ptr(),
            ws["part"].data_ptr(), B, bchunk, bchunk, bchunk, base, nt, nch,
            nch, nch, ops._stream())
    torch.cuda.synchronize()
    part = ws["part"].cpu()
    d = {n: t.double() for n, t in src.items()}
    counts = set()
    for y in range(nch):
        b0, b1 = y * bchunk, max(y * bchunk, min(B, (y + 1) * bchunk))
        counts.add(b1 - b0)
        s = slice(b0, b1)
        row = part[y].double()
        assert torch.equal(row[OFF_WF1:OFF_BF1].view(50, 320),
                           d["gh1"][s].t() @ d["p2"][s]), y
        assert torch.equal(row[OFF_BF1:OFF_WF2], d["gh1"][s].sum(0)), y
        assert torch.equal(row[OFF_WF2:OFF_BF2].view(10, 50),
                           d["glog"][s].t() @ d["d3"][s]), y
        assert torch.equal(row[OFF_BF2:OFF_BF2 + 10], d["glog"][s].sum(0)), y
    print("samples per block:", sorted(counts))
