"""The combine dispatch (net_gw_combine_kernel, net_gw_combine_sgd_kernel)
driven through its raw launchers on a hand-made ``part`` workspace.

Every slot the kernel must not read holds NaN, every output is pre-filled
with NaN.  With small integers all sums and the SGD update are exact in
fp32 in any order, so the results must be bit-equal to float64; a
standard-normal workspace is held to the fp32 summation bound n*u*S."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dist_tuto_pth_amd.ops import _stream
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
NAN = float("nan")
GW_TOTAL = 21840
C1 = 260                      # conv1.w + conv1.b, the region with slots
SLOTS = 8                     # T_CONV1: main slot + 7 extension slots
GW_ROW = GW_TOTAL + (SLOTS - 1) * C1
ROWS = 32                     # GW_MAX_CH
CONV2 = (260, 5280)           # conv2.w + conv2.b
SIZES = [250, 10, 5000, 20, 16000, 50, 500, 10]
CASES = [(1, 1, 1), (2, 3, 4), (5, 3, 7), (16, 16, 24), (24, 24, 32),
         (32, 32, 32)]


@pytest.fixture(scope="module")
def k():
    # the HIP extension must actually load — no silent fallback
    k = load_native("_kernels")
    assert (k.GW_ROW, k.GW_MAX_CH) == (GW_ROW, ROWS)
    return k


def _live_mask(nch, nch1, nch2):
    """[ROWS, GW_ROW] bool: the slots the combine sums."""
    m = torch.zeros(ROWS, GW_ROW, dtype=torch.bool)
    m[:nch, CONV2[1]:GW_TOTAL] = True      # fc region
    m[:nch2, CONV2[0]:CONV2[1]] = True     # conv2 region
    m[:nch1, :C1] = True                   # conv1 main slot
    m[:nch1, GW_TOTAL:] = True             # conv1 extension slots
    return m


def _part(values, counts):
    """values where live, NaN everywhere else (float32, CPU)."""
    return torch.where(_live_mask(*counts), values,
                       torch.full_like(values, NAN))


def _fold(part64):
    """float64 [GW_TOTAL]: sum of the live slots of every element (the
    NaN slots must already be zeroed)."""
    out = part64[:, :GW_TOTAL].sum(0)
    out[:C1] += part64[:, GW_TOTAL:].reshape(ROWS, SLOTS - 1, C1).sum((0, 1))
    return out


def _row_counts(nch, nch1, nch2):
    n = torch.full((GW_TOTAL,), nch, dtype=torch.float64)
    n[CONV2[0]:CONV2[1]] = nch2
    n[:C1] = SLOTS * nch1
    return n


def _int_values(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (ROWS, GW_ROW), generator=g).float()


def _split(flat):
    return list(torch.split(flat, SIZES))


def _nan_outputs():
    return [torch.full((n,), NAN, device=DEV) for n in SIZES]


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _assert_bits(got, want64, what):
    for idx, (a, b) in enumerate(zip(got, _split(want64))):
        assert torch.equal(a.cpu().double(), b), f"{what}[{idx}]"


@pytest.mark.parametrize("counts", CASES)
def test_combine_integer_exact(k, counts):
    """All 8 gradients bit-equal to the float64 sum of the live slots;
    a read of any dead slot, or an element left unwritten, gives NaN."""
    part = _part(_int_values(11), counts)
    ref = _fold(torch.nan_to_num(part.double(), nan=0.0))
    grads = _nan_outputs()
    dpart = part.to(DEV)
    k.net_gw_combine_raw(dpart.data_ptr(), _ptrs(grads), *counts, _stream())
    torch.cuda.synchronize()
    _assert_bits(grads, ref, "grad")


@pytest.mark.parametrize("with_buf", [True, False])
@pytest.mark.parametrize("counts", CASES)
def test_combine_sgd_integer_exact(k, counts, with_buf):
    """Integer parameters and momentum, lr = 0.5, mu = 0.25: v = mu*buf + g
    and prm - lr*v are exact in fp32 (multiples of 1/8 far below 2^21),
    so grads, buffers and parameters are bit-equal to float64.  An empty
    buffer list means no momentum."""
    lr, mu = 0.5, 0.25
    part = _part(_int_values(12), counts)
    g64 = _fold(torch.nan_to_num(part.double(), nan=0.0))
    gen = torch.Generator().manual_seed(13)
    prm0 = torch.randint(-8, 9, (GW_TOTAL,), generator=gen).double()
    buf0 = torch.randint(-8, 9, (GW_TOTAL,), generator=gen).double()
    v64 = mu * buf0 + g64 if with_buf else g64
    grads = _nan_outputs()
    prms = [t.float().to(DEV) for t in _split(prm0)]
    bufs = [t.float().to(DEV) for t in _split(buf0)] if with_buf else []
    loss_part = torch.tensor([3.0, NAN], device=DEV)
    loss_out = torch.full((1,), NAN, device=DEV)
    dpart = part.to(DEV)
    k.net_gw_combine_sgd_raw(dpart.data_ptr(), _ptrs(grads),
                             _ptrs(prms), _ptrs(bufs), *counts, lr, mu,
                             loss_part.data_ptr(), loss_out.data_ptr(), 1,
                             _stream())
    torch.cuda.synchronize()
    _assert_bits(grads, g64, "grad")
    _assert_bits(prms, prm0 - lr * v64, "param")
    if with_buf:
        _assert_bits(bufs, v64, "buf")
    assert loss_out.item() == 3.0


@pytest.mark.parametrize("nblk", [1, 100, 256, 4096])
def test_combine_sgd_loss_exact(k, nblk):
    """loss_out is the exact sum of the first nblk_fwd integer loss
    partials; what lies past them is NaN and must not be read."""
    counts = (2, 3, 4)
    part = _part(_int_values(14), counts).to(DEV)
    gen = torch.Generator().manual_seed(15 + nblk)
    lp = torch.randint(-3, 4, (nblk,), generator=gen).float()
    loss_part = torch.full((4096 + 1024,), NAN)
    loss_part[:nblk] = lp
    loss_part = loss_part.to(DEV)
    loss_out = torch.full((1,), NAN, device=DEV)
    grads = _nan_outputs()
    prms = [torch.zeros(n, device=DEV) for n in SIZES]
    k.net_gw_combine_sgd_raw(part.data_ptr(), _ptrs(grads), _ptrs(prms), [],
                             *counts, 0.5, 0.25, loss_part.data_ptr(),
                             loss_out.data_ptr(), nblk, _stream())
    torch.cuda.synchronize()
    assert loss_out.item() == lp.double().sum().item()
    assert not any(torch.isnan(g).any().item() for g in grads)


def test_combine_random_bound(k):
    """Standard-normal partials at the B=128 plan: every element within
    n*u*S of float64, u = 2^-24, S = sum of |terms|, n = its row count
    (nch, nch2, or 8*nch1).  No element is excluded."""
    counts = (16, 16, 24)
    gen = torch.Generator().manual_seed(16)
    part = _part(torch.randn(ROWS, GW_ROW, generator=gen), counts)
    p64 = torch.nan_to_num(part.double(), nan=0.0)
    ref, mag = _fold(p64), _fold(p64.abs())
    bound = _row_counts(*counts) * 2.0 ** -24 * mag
    grads = _nan_outputs()
    dpart = part.to(DEV)
    k.net_gw_combine_raw(dpart.data_ptr(), _ptrs(grads), *counts, _stream())
    torch.cuda.synchronize()
    got = torch.cat([g.cpu().double() for g in grads])
    err = (got - ref).abs()
    worst = (err / bound).max().item()
    print(f"worst |gpu - ref| / (n*u*S) = {worst:.3f}")
    assert not torch.isnan(got).any()
    assert bool((err <= bound).all()), worst
