"""Restatement of posterior guidance for the mechanics sampler, built only from oracle.pidm_oracle functions (mechanics_residual,
mechanics_model_out, bilinear_resize, unet_forward, p_sample_update, diffusion_tables), tests/mech_ref.residual_ref (per-element
stiffness) and torch autograd.  TEST INFRASTRUCTURE for tests/test_guided_mechanics.py: no project kernel is called.

Per sample, for an x0 estimate x [3,nel,nel] = (u_x, u_y, rho) with model_out = (u resized to nn = nel + 1, rho zero-padded):
L_obs = sum m (model_out - y)^2 with the padding row / column of channel 2 left out whatever m says there, L_pde = sum r^2,
L_vol = (mean(rho) - vf)^2, Phi = zeta_obs sqrt(L_obs) + zeta_pde sqrt(L_pde) + zeta_vol sqrt(L_vol); a term whose L is exactly 0 is
omitted.  One guided step from the nn x nn state x_t:  x_{t-1} = p_sample_update(model_out(x0_hat), x_t) - d Phi(x0_hat) / d x_t, where
x0_hat = unet(cat(resize(x_t), resize(conditioning), resize(bcs)) to nel x nel).

Every function works in the dtype it is given (`dtype=`): float64 is the reference and the same text in float32 is the yardstick for
what fp32 arithmetic costs (the rule of tests/test_kernels_mech_f64.py)."""
import torch

from oracle import pidm_oracle as O
from tests import mech_ref as MR
from tests.guided_ref import _default_float64, params64, tables64   # noqa: F401  (re-exported for the test module)


def quantities(x0, bcs, vf, kloc, elem_dofs):
    """(residual [B,ndof], model_out [B,3,nn,nn], shift [B]); kloc [8,8] (uniform mesh: the oracle's functions) or [E,8,8]"""
    kloc = torch.as_tensor(kloc)
    if kloc.dim() == 2:
        r, _, shift = O.mechanics_residual(x0, bcs, vf, kloc.to(x0.dtype), elem_dofs)
        return r, O.mechanics_model_out(x0), shift
    r, mo, _, shift = MR.residual_ref(x0, bcs, vf, kloc, elem_dofs)
    return r, mo, shift


def state_mask(m):
    """the mask without the padding row and column of channel 2"""
    w = m.clone()
    w[:, 2, -1, :] = 0
    w[:, 2, :, -1] = 0
    return w


def _sqrt_or_omit(L):
    on = L > 0
    return torch.sqrt(torch.where(on, L, torch.ones_like(L))) * on.to(L.dtype)


def potential(x0, bcs, vf, y, m, zetas, kloc, elem_dofs):
    """(Phi [B], sums [B,3], model_out) of x0 [B,3,nel,nel] in x0.dtype (differentiable)"""
    r, mo, shift = quantities(x0, bcs, vf, kloc, elem_dofs)
    l_obs = (state_mask(m) * (mo - y) ** 2).sum(dim=(1, 2, 3))
    l_pde = (r ** 2).sum(dim=1)
    l_vol = shift ** 2
    phi = zetas[0] * _sqrt_or_omit(l_obs) + zetas[1] * _sqrt_or_omit(l_pde) + zetas[2] * _sqrt_or_omit(l_vol)
    return phi, torch.stack([l_obs, l_pde, l_vol], dim=1), mo


def cotangent(x0, bcs, vf, y, m, zetas, kloc, elem_dofs, dtype=torch.float64):
    """v = dPhi/dx0 [B,3,nel,nel], model_out [B,3,nn,nn] and sums [B,3] in `dtype`"""
    x = x0.detach().to(dtype).clone().requires_grad_(True)
    phi, sums, mo = potential(x, bcs.to(dtype), vf.to(dtype), y.to(dtype), m.to(dtype), zetas, torch.as_tensor(kloc).to(dtype), elem_dofs)
    v = torch.autograd.grad(phi.sum(), x, allow_unused=True)[0] if phi.requires_grad else None
    if v is None:
        v = torch.zeros_like(x)
    return v.detach(), mo.detach(), sums.detach()


def guided_step(p, cfg, tables, x_t, cond, bcs, t, z, y, m, zetas, kloc, elem_dofs, surpress_noise=True, dtype=torch.float64):
    """One guided ancestral step from x_t [B,3,nn,nn]: returns (x_{t-1}, sums [B,3], g = dPhi/dx_t [B,3,nn,nn]) in `dtype`.
    p, tables: parameters / schedule tables already in `dtype`."""
    B, nel = x_t.shape[0], x_t.shape[-1] - 1
    x = x_t.detach().to(dtype).clone().requires_grad_(True)
    cond, bcs = cond.to(dtype), bcs.to(dtype)
    net_in = torch.cat((O.bilinear_resize(x, nel), O.bilinear_resize(cond, nel), O.bilinear_resize(bcs, nel)), dim=1)
    if dtype == torch.float64:
        with _default_float64():
            x0 = O.unet_forward(p, net_in, torch.full((B,), t, dtype=torch.long), cfg)
    else:
        x0 = O.unet_forward(p, net_in, torch.full((B,), t, dtype=torch.long), cfg)
    assert x0.dtype == dtype
    phi, sums, mo = potential(x0, bcs, cond[:, 0, 0, 0], y.to(dtype), m.to(dtype), zetas, torch.as_tensor(kloc).to(dtype), elem_dofs)
    g = torch.autograd.grad(phi.sum(), x, allow_unused=True)[0] if phi.requires_grad else None
    if g is None:
        g = torch.zeros_like(x)
    x_prev = O.p_sample_update(tables, mo.detach(), x.detach(), t, z.to(dtype), surpress_noise=surpress_noise) - g
    return x_prev.detach(), sums.detach(), g.detach()
