"""The cases of tests/fp32_bounds.py through the CPU branch of ops and
FusedSGD: the float64 references and the derived bounds the HIP kernels
answer to in tests/test_fp32_kernels_gpu.py are sound if the plain-torch
fp32 golden path meets them here.  Also every input the wrappers must
refuse, on CPU tensors, and the contract model of the reduction helpers
against hand-computed values."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_bounds as fb  # noqa: E402

DEV = "cpu"


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


@pytest.mark.parametrize("case", fb.validation_cases(gpu=False),
                         ids=lambda c: c[0])
def test_wrappers_refuse(case):
    name, exc, call = case
    with pytest.raises(exc, match=fb.validation_match(name)):
        call(DEV)


def test_reduction_contract_model():
    """The model by hand: fp32 accumulation in the order p = 0..P-1, one
    rounding, nothing outside [0, n) touched."""
    dst = torch.tensor([1.0, 2.0, 3.0, 9.0])
    src = torch.tensor([10.0, 20.0, 30.0, 0.0, 0.0, 100.0, 200.0, 300.0])
    fb.reduce_columns_model(dst, src, 2, 5, 3, 0.5)
    assert torch.equal(dst, torch.tensor([55.5, 111.0, 166.5, 9.0]))
    fb.reduce_columns_model(dst, src, 0, 0, 2, 2.0)
    assert torch.equal(dst, torch.tensor([111.0, 222.0, 166.5, 9.0]))
    # bf16: 256 + 1 + 1 is 258 in fp32 and rounds once to 258; two bf16
    # adds would stay at 256
    d = torch.tensor([256.0, 7.0]).bfloat16()
    s = torch.tensor([1.0, 0.0, 1.0, 0.0]).bfloat16()
    fb.reduce_columns_model(d, s, 2, 2, 1, 1.0)
    assert torch.equal(d.float(), torch.tensor([258.0, 7.0]))
    a = torch.tensor([1.0, 2.0, 3.0]).bfloat16()
    fb.add_inplace_model(a, torch.tensor([0.5, 0.5, 0.5]).bfloat16(), 2)
    assert torch.equal(a.float(), torch.tensor([1.5, 2.5, 3.0]))
    f = torch.tensor([1.0, 2.0, 3.0])
    fb.scale_f32_model(f, 0.25, 2)
    assert torch.equal(f, torch.tensor([0.25, 0.5, 3.0]))


def _bf16_bits_once(f):
    """fp32 -> bf16 bits in integer arithmetic: round to nearest even, any
    NaN to 0x7fc0 (what the kernels' store conversion does)."""
    u = f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    r = torch.where((u & 0x7FFFFFFF) > 0x7F800000,
                    torch.full_like(r, 0x7FC0), r)
    return (r & 0xFFFF).to(torch.int32)


@pytest.mark.parametrize("P", [None] + fb.ROUNDING_P)
def test_reduction_contract_rounds_once(P):
    """The expectation the GPU tests hold the bf16 kernels to at inexact
    sums: the model's bits are the fp32 sum in the order dst, p = 0..P-1,
    scaled, rounded once; the case has sums that need the rounding, and its
    NaN columns come out as 0x7fc0."""
    n, off = fb.ROUNDING_N, fb.REDUCE_OFFSET
    for scale in ([1.0] if P is None else fb.REDUCE_SCALES):
        big, src, want, stride = fb.rounding_case(P, scale)
        acc = big[off:off + n].float()
        for p in range(P or 1):
            acc = acc + src[p * stride:p * stride + n].float()
        acc = acc * torch.tensor(scale, dtype=torch.float32)
        got = want.view(torch.int16).to(torch.int32) & 0xFFFF
        assert torch.equal(got[off:off + n], _bf16_bits_once(acc))
        # guards untouched; NaN where it went in; rounding had work to do
        raw = big.view(torch.int16).to(torch.int32) & 0xFFFF
        assert torch.equal(got[:off], raw[:off])
        assert torch.equal(got[off + n:], raw[off + n:])
        for j in fb.ROUNDING_NAN:
            assert int(got[off + j]) == 0x7FC0
        inexact = torch.isfinite(acc) & (acc.bfloat16().float() != acc)
        print(f"P={P} scale={scale}: {int(inexact.sum())} of {n} inexact")
        assert int(inexact.sum()) > n // 4


def test_pad_chunks_realigns_a_misaligned_view():
    """The reduction launchers refuse a pointer off a 16-byte boundary, so
    the all-reduce algorithms route such a tensor through their aligned
    work buffer, as they do for one that needs padding."""
    from dist_tuto_pth_amd.algorithms.xgmi import _pad_chunks

    def buf(key, numel, dtype, device):
        return torch.empty(numel, dtype=dtype, device=device)

    base = torch.arange(65, dtype=torch.float32)
    assert base.data_ptr() % 16 == 0
    work, chunk, padded = _pad_chunks(base[:64], 4, buf)
    assert not padded and chunk == 16
    assert work.data_ptr() == base.data_ptr()
    view = base[1:]
    work, chunk, padded = _pad_chunks(view, 4, buf)
    assert padded and chunk == 16 and work.numel() == 64
    assert work.data_ptr() % 16 == 0 and torch.equal(work, view)


def test_zz_report_ratios():
    """Prints the largest error/bound ratio per op of this run."""
    fb.report()
    assert all(r <= 1.0 for r in fb.WORST.values())
