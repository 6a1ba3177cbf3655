"""GPU tests of FusedSGD's weight decay and Nesterov momentum (the
compile-time variants of sgd_step_kernel): two steps against
torch.optim.SGD on float64 copies, within the bounds derived in
tests/xent_bounds.py, shared with tests/test_sgd_decay_cpu.py."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import xent_bounds as xb
    from dist_tuto_pth_amd.optim import FusedSGD
    from dist_tuto_pth_amd.utils.native import load_native
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    # the HIP extension must actually load — no silent fallback
    load_native("_kernels")


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("which", list(xb.DECAY_LISTS))
def test_fused_sgd_decay_bounds(which, nesterov, zero_grad):
    xb.decay_case(which, nesterov, zero_grad, DEV)


@pytest.mark.parametrize("zero_grad", [False, True])
def test_weight_decay_without_momentum(zero_grad):
    """The weight-decay instance with null momentum buffers."""
    xb.decay_no_momentum_case(zero_grad, DEV)


def test_refused_settings():
    p = torch.zeros(4, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="FusedSGD"):
        FusedSGD([p], lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="FusedSGD"):
        FusedSGD([p], lr=0.1, momentum=0.5, weight_decay=-1e-4)
    # the native entry point refuses them too, before it launches
    k = load_native("_kernels")
    g = torch.ones(4, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(ValueError, match="sgd_step"):
        k.sgd_step([p.data_ptr()], [g.data_ptr()], [0], [4], 0.1, 0.0,
                   False, s, 0.0, True)
    with pytest.raises(ValueError, match="sgd_step"):
        k.sgd_step([p.data_ptr()], [g.data_ptr()], [0], [4], 0.1, 0.5,
                   False, s, -1.0, False)
    torch.cuda.synchronize()
    assert bool((p == 0).all())


def test_present_binding_and_defaults_agree():
    """The eight-argument sgd_step call and the explicit wd = 0, no
    Nesterov call give the same bits."""
    k = load_native("_kernels")
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(1029, generator=g)
    b0 = torch.randn(1029, generator=g)
    gr = torch.randn(1029, generator=g).to(DEV)
    s = torch.cuda.current_stream().cuda_stream
    outs = []
    for extra in ((), (0.0, False)):
        p, b = p0.to(DEV), b0.to(DEV)
        k.sgd_step([p.data_ptr()], [gr.data_ptr()], [b.data_ptr()], [1029],
                   0.1, 0.9, False, s, *extra)
        outs.append((p.cpu(), b.cpu()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], p0)
