"""GPU tests of the fp32 kernels of csrc/kernels.hip beyond Net's shapes:
conv2d, linear, log_softmax, nll_loss, log_softmax_nll, FusedSGD's
sgd_step and the reduction helpers add_inplace, reduce_columns and
scale_f32.  The float64 references, the case lists and the derived
elementwise bounds are in tests/fp32_bounds.py (its docstring has the
rules); the case runners are shared with tests/test_fp32_kernels_cpu.py,
so the kernels answer to exactly the bounds the CPU golden path meets.
The reduction helpers are compared bit for bit with the contract model
that tests/test_xgmi_logic.py's FakeKernels runs."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fp32_bounds as fb
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------
# refused inputs: every one raises before anything is launched
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", fb.validation_cases(gpu=True),
                         ids=lambda c: c[0])
def test_wrappers_refuse(case):
    name, exc, call = case
    with pytest.raises(exc, match=fb.validation_match(name)):
        call(DEV)


def test_reduction_launchers_refuse():
    """A stride the vector paths would truncate, or a pointer their
    16-byte accesses would misalign, is refused by the launcher."""
    k = load_native("_kernels")
    s = _stream()
    for dtype, vec in ((torch.float32, 4), (torch.bfloat16, 8)):
        dt = fb.NCCL_DTYPE[dtype]
        esz = 4 if dtype == torch.float32 else 2
        dst = torch.ones(64, device=DEV, dtype=dtype)
        src = torch.ones(256, device=DEV, dtype=dtype)
        d, r = dst.data_ptr(), src.data_ptr()
        for stride in (vec + 1, 2 * vec - 1, vec // 2):
            with pytest.raises(ValueError, match="reduce_columns"):
                k.reduce_columns(d, r, 2, stride, 8, 1.0, dt, s)
        with pytest.raises(ValueError, match="reduce_columns"):
            k.reduce_columns(d + esz, r, 2, 64, 8, 1.0, dt, s)
        with pytest.raises(ValueError, match="reduce_columns"):
            k.reduce_columns(d, r + esz, 2, 64, 8, 1.0, dt, s)
        with pytest.raises(ValueError, match="reduce_columns"):
            k.reduce_columns(d + esz, 0, 0, 0, 8, 1.0, dt, s)
        with pytest.raises(ValueError, match="add_inplace"):
            k.add_inplace(d + esz, r, 8, dt, s)
        with pytest.raises(ValueError, match="add_inplace"):
            k.add_inplace(d, r + esz, 8, dt, s)
        torch.cuda.synchronize()
        assert bool((dst == 1).all()) and bool((src == 1).all())
    f = torch.ones(64, device=DEV)
    with pytest.raises(ValueError, match="scale_f32"):
        k.scale_f32(f.data_ptr() + 4, 2.0, 8, s)
    torch.cuda.synchronize()
    assert bool((f == 1).all())


# ---------------------------------------------------------------------------
# bounds against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", fb.CONV_SHAPES)
def test_conv2d_bounds(shape, bias):
    fb.conv_case(shape, bias, DEV)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", fb.LINEAR_SHAPES)
def test_linear_bounds(shape, bias, relu):
    fb.linear_case(shape, bias, relu, DEV)


def test_conv2d_noncontiguous_parameters():
    fb.noncontig_conv_case(DEV)


def test_linear_noncontiguous_weight():
    fb.noncontig_linear_case(DEV)


@pytest.mark.parametrize("regime", fb.REGIMES)
@pytest.mark.parametrize("shape", fb.SOFTMAX_SHAPES)
def test_log_softmax_and_losses_bounds(shape, regime):
    # one float64 reference per case, shared by the three ops
    fb.log_softmax_case(shape, regime, DEV)
    fb.nll_loss_case(shape, regime, DEV)
    fb.log_softmax_nll_case(shape, regime, DEV)


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("mu", fb.SGD_MOMENTA)
@pytest.mark.parametrize("which", list(fb.SGD_LISTS))
def test_fused_sgd_bounds(which, mu, zero_grad):
    fb.sgd_case(which, mu, zero_grad, DEV)


# ---------------------------------------------------------------------------
# reduction helpers: the real kernel against the contract model, bit for bit
# ---------------------------------------------------------------------------
def _bits_equal(a, b):
    if a.dtype == torch.bfloat16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    else:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


@pytest.mark.parametrize("P", fb.REDUCE_P)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reduce_columns_matches_contract(dtype, P):
    k = load_native("_kernels")
    off = fb.REDUCE_OFFSET
    esz = 4 if dtype == torch.float32 else 2
    for n in fb.REDUCE_N:
        stride = fb.reduce_stride(n)
        assert stride > n and stride % 8 == 0
        for scale in fb.REDUCE_SCALES:
            g = fb._gen(P, n, esz, int(scale * 8))
            # guard elements on both sides of the destination
            big = fb.reduce_values(off + n + off, dtype, g)
            src = fb.reduce_values(max(P, 1) * stride, dtype, g)
            want = big.clone()
            fb.reduce_columns_model(want[off:], src, P, stride, n, scale)
            assert _bits_equal(want[:off], big[:off])
            assert _bits_equal(want[off + n:], big[off + n:])
            assert P == 0 and scale == 1.0 or not _bits_equal(want, big)

            bd, sd = big.to(DEV), src.to(DEV)
            assert bd.data_ptr() % 16 == 0 and sd.data_ptr() % 16 == 0
            k.reduce_columns(bd.data_ptr() + off * esz,
                             sd.data_ptr() if P else 0, P,
                             stride if P else 0, n, scale,
                             fb.NCCL_DTYPE[dtype], _stream())
            assert _bits_equal(bd.cpu(), want), (n, scale)
            assert _bits_equal(sd.cpu(), src)
    if dtype == torch.bfloat16 and P in fb.ROUNDING_P:
        # inexact sums and NaN: the one rounding decides the stored bits
        for scale in fb.REDUCE_SCALES:
            big, src, want, stride = fb.rounding_case(P, scale)
            bd, sd = big.to(DEV), src.to(DEV)
            k.reduce_columns(bd.data_ptr() + off * esz, sd.data_ptr(), P,
                             stride, fb.ROUNDING_N, scale,
                             fb.NCCL_DTYPE[dtype], _stream())
            assert _bits_equal(bd.cpu(), want), scale
            assert _bits_equal(sd.cpu(), src)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_add_inplace_matches_contract(dtype):
    k = load_native("_kernels")
    for n in fb.POINTWISE_N:
        g = fb._gen(n, 3)
        # whole vectors past n: the guard behind the destination
        dst = fb.reduce_values(n + 16, dtype, g)
        src = fb.reduce_values(n + 16, dtype, g)
        want = dst.clone()
        fb.add_inplace_model(want, src, n)
        assert _bits_equal(want[n:], dst[n:])
        dd, sd = dst.to(DEV), src.to(DEV)
        k.add_inplace(dd.data_ptr(), sd.data_ptr(), n,
                      fb.NCCL_DTYPE[dtype], _stream())
        assert _bits_equal(dd.cpu(), want), n
        assert _bits_equal(sd.cpu(), src)
    if dtype == torch.bfloat16:
        # inexact sums and NaN: the one rounding decides the stored bits
        big, src, want, _ = fb.rounding_case(None)
        bd, sd = big.to(DEV), src.to(DEV)
        k.add_inplace(bd.data_ptr() + fb.REDUCE_OFFSET * 2, sd.data_ptr(),
                      fb.ROUNDING_N, fb.NCCL_DTYPE[dtype], _stream())
        assert _bits_equal(bd.cpu(), want)
        assert _bits_equal(sd.cpu(), src)


def test_scale_f32_matches_contract():
    k = load_native("_kernels")
    for n in fb.POINTWISE_N:
        for scale in (0.125, 1.0 / 3.0):
            dst = fb.reduce_values(n + 16, torch.float32, fb._gen(n, 5))
            want = dst.clone()
            fb.scale_f32_model(want, scale, n)
            assert _bits_equal(want[n:], dst[n:])
            dd = dst.to(DEV)
            k.scale_f32(dd.data_ptr(), scale, n, _stream())
            assert _bits_equal(dd.cpu(), want), (n, scale)


def test_zz_report_ratios():
    """Prints the largest error/bound ratio per op of this run."""
    fb.report()
    assert all(r <= 1.0 for r in fb.WORST.values())
