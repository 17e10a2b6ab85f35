"""Darcy residual for any stencil set (pidm_darcy_residual_general_fwd / _bwd, csrc/k_stencil.hip) and ResidualsDarcy with
fd_acc 4 / 6 and bcs='periodic': against the specialised second-order kernel, against the genuine reference (golden
g27_darcy_general, tools/make_golden_stencils.py) and through one training step.  Tolerances are the existing figures of
tests/test_kernels_darcy.py (2e-6 forward, 5e-6 adjoint, max-norm relative: two summation orders of the same fp32 terms)."""
import os

import numpy as np
import pytest
import torch

from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd._lib import ptr, stream_ptr
from physicsinformeddiffusionmodels_amd.denoising_utils import DenoisingDiffusion
from physicsinformeddiffusionmodels_amd.grad_utils import StencilGradients, _ops_array
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
from physicsinformeddiffusionmodels_amd.unet_model import Unet3D
from tests.test_training_step import patched_rng

G = os.path.join(os.path.dirname(__file__), "golden")
CASES = ((4, "none", True), (6, "none", True), (4, "none", False), (2, "periodic", True), (4, "periodic", True))


def rel(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _lib(backend):
    L, dev = backend
    return L, (L if dev.type == "cpu" else None), dev


@pytest.mark.parametrize("P,B", [(16, 3), (64, 2), (10, 3), (21, 2)])
def test_general_entries_with_second_order_tables_equal_the_specialised_kernel(backend, P, B):
    L, lib, dev = _lib(backend)
    st = stream_ptr(dev)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(B, 2, P, P, generator=g)
    x0[:, 1] = torch.exp(0.5 * x0[:, 1])
    x0 = x0.to(dev)
    gr = torch.randn(B, P * P, 3, generator=g).to(dev)
    fs = O.darcy_source_field(P).reshape(-1).contiguous().to(dev)
    inv_h = float(P - 1)
    res_s, gx_s = torch.empty(B, P * P, 3, device=dev), torch.empty_like(x0)
    L.check(L.pidm_darcy_residual_fwd(ptr(x0), ptr(fs), inv_h, -inv_h, ptr(res_s), B, P, st))
    L.check(L.pidm_darcy_residual_bwd(ptr(x0), ptr(gr), inv_h, -inv_h, ptr(gx_s), B, P, st))
    sg = StencilGradients(d0=1.0 / inv_h, d1=-1.0 / inv_h, fd_acc=2, device=dev, lib=lib)
    ops, keep = _ops_array((sg.d_d0, sg.d_d1, sg.d_d00, sg.d_d11), dev)
    ws = torch.empty(L.pidm_darcy_general_ws(B, P), dtype=torch.uint8, device=dev)
    res_g, gx_g = torch.empty_like(res_s), torch.empty_like(x0)
    L.check(L.pidm_darcy_residual_general_fwd(ptr(x0), ptr(fs), ops, 0, 1.0, ptr(res_g), ptr(ws), B, P, st))
    L.check(L.pidm_darcy_residual_general_bwd(ptr(x0), ptr(gr), ops, 0, 1.0, ptr(gx_g), ptr(ws), B, P, st))
    print(f"P={P} B={B}: fwd {rel(res_g, res_s):.2e} adj {rel(gx_g, gx_s):.2e}")
    assert rel(res_g, res_s) < 2e-6
    assert rel(gx_g, gx_s) < 5e-6


@pytest.mark.parametrize("acc,bcs,rev", CASES)
def test_residuals_darcy_vs_reference_golden(backend, acc, bcs, rev):
    L, lib, dev = _lib(backend)
    g = np.load(os.path.join(G, "g27_darcy_general.npz"))
    tag = f"{acc}_{bcs}_{int(rev)}"
    R = ResidualsDarcy(model=None, fd_acc=acc, pixels_per_dim=16, pixels_at_boundary=True, reverse_d1=rev, device=dev, bcs=bcs, lib=lib)
    assert R.fd_acc == acc and R.periodic == (bcs == "periodic") and R.grads.stencil_gradients.fd_acc == acc
    xr = torch.from_numpy(g["x0"]).to(dev).requires_grad_(True)
    res = R.compute_residual(xr, pass_through=True)["residual"]
    (gx,) = torch.autograd.grad((torch.from_numpy(g["w"]).to(dev) * res).sum(), xr)
    ref, gref = torch.from_numpy(g["res_" + tag]), torch.from_numpy(g["gx_" + tag])
    print(f"{tag}: fwd {rel(res, ref):.2e} adj {rel(gx, gref):.2e}")
    assert rel(res, ref) < 2e-6
    assert rel(gx, gref) < 5e-6


def test_default_configuration_still_runs_the_specialised_kernel(backend):
    L, lib, dev = _lib(backend)
    P, B = 16, 3
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(B, 2, P, P, generator=g)
    x0[:, 1] = torch.exp(0.5 * x0[:, 1])
    x0 = x0.to(dev)
    R = ResidualsDarcy(model=None, fd_acc=2, pixels_per_dim=P, pixels_at_boundary=True, reverse_d1=True, device=dev, lib=lib)
    assert R.specialised and not R.periodic and hasattr(R, "grads")
    direct = torch.empty(B, P * P, 3, device=dev)
    L.check(L.pidm_darcy_residual_fwd(ptr(x0), ptr(R._f_s_flat.to(dev)), R.inv_h0, R.inv_h1, ptr(direct), B, P, stream_ptr(dev)))
    assert torch.equal(R.residual_of(x0), direct)


def test_cocogen_correction_is_second_order_only(backend):
    L, lib, dev = _lib(backend)
    for kw in (dict(fd_acc=4), dict(fd_acc=2, bcs="periodic")):
        R = ResidualsDarcy(model=None, pixels_per_dim=16, pixels_at_boundary=True, reverse_d1=True, device=dev, lib=lib, **kw)
        with pytest.raises(NotImplementedError):
            R.residual_correction(torch.zeros(1, 256, 2, device=dev))
        with pytest.raises(NotImplementedError):
            R.jacobian_max(torch.zeros(1, 2, 16, 16, device=dev))
    with pytest.raises(NotImplementedError):
        ResidualsDarcy(model=None, fd_acc=8, pixels_per_dim=16, pixels_at_boundary=True, reverse_d1=True)


@pytest.mark.parametrize("fd_acc,bcs", [(4, "none"), (2, "periodic")])
def test_training_step_through_the_general_residual(backend, fd_acc, bcs):
    """One step of the dim-8 UNet: the loss equals the loss algebra (reference src/denoising_utils.py:677-684) restated in float64
    from the step's own model_out and residual (1e-5 relative: DESIGN section 2's figure for the residual loss on identical
    inputs), every used parameter gets a finite gradient, and only fd_acc=2 / bcs='none' is offered the fused kernel."""
    L, lib, dev = _lib(backend)
    P, B = 16, 3
    m = Unet3D(dim=8, channels=2)
    m.load_state_dict(O.fill_state_dict(m.state_dict()))
    m = m.to(dev)
    m._pidm_lib = lib
    diff = DenoisingDiffusion(100, dev, lib=lib)
    mk = lambda a, b: ResidualsDarcy(model=m, fd_acc=a, pixels_per_dim=P, pixels_at_boundary=True, reverse_d1=True, device=dev,  # noqa: E731
                                     bcs=b, domain_length=1., lib=lib)
    res = mk(fd_acc, bcs)
    gen = torch.Generator().manual_seed(4)
    x0 = torch.randn(B, 2, P, P, generator=gen).to(dev)
    eps = torch.randn(B, 2, P, P, generator=gen).to(dev)
    t = torch.tensor([3, 50, 97]).to(dev)
    assert diff._darcy_fast_path_ok(mk(2, "none"), 0., 0., x0)
    assert not diff._darcy_fast_path_ok(res, 0., 0., x0)
    seen = {}
    inner = res.compute_residual

    def recording(*a, **k):
        out = inner(*a, **k)
        seen.update(out)
        return out
    res.compute_residual = recording
    with patched_rng(randint=lambda *a, **k: t.clone(), randn_like=lambda *a, **k: eps.clone()):
        loss, data_l, res_l, ineq_l, opt_l = diff.model_estimation_loss(x0, residual_func=res, c_data=1., c_residual=1e-3,
                                                                        c_ineq=0., lambda_opt=0.)
    out, r = seen["model_out"].detach().double().cpu(), seen["residual"].detach().double().cpu()
    if out.dim() == 3:
        out = out.reshape(B, P, P, 2).permute(0, 3, 1, 2)
    tc = t.cpu()
    p2w, var = diff.diff_dict["p2_loss_weight"].double().cpu()[tc], diff.diff_dict["posterior_variance_clipped"].double().cpu()[tc]
    data64 = (((x0.double().cpu() - out) ** 2).reshape(B, -1).mean(dim=1) * p2w).mean()
    want = 1. * data64 + (1e-3 * 0.5 * r ** 2 / var.view(B, 1, 1)).mean()
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item()), (loss.item(), want.item())
    assert abs(data_l - data64.item()) <= 1e-5 * abs(data64.item())
    assert abs(res_l - r.abs().mean().item()) <= 1e-5 * r.abs().mean().item()
    assert ineq_l == 0. and opt_l == 0.
    loss.backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) == 259 and all(torch.isfinite(gr).all() for gr in grads)
    assert sum(float(gr.abs().sum()) for gr in grads) > 0.
