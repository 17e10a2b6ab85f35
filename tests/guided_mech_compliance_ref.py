"""Restatement of the compliance term of mechanics posterior guidance, on top of tests/guided_mech_ref.py: oracle.pidm_oracle
functions (mechanics_residual on a uniform mesh), tests/mech_ref.residual_ref (per-element stiffness) and torch autograd.  TEST
INFRASTRUCTURE for tests/test_guided_mechanics_compliance.py: no project kernel is called.

C = U . A(rho) U per sample, A the closed stiffness (identity rows on clamped dofs): the `compliance` output of both residual
restatements, signed.  Phi4 = Phi(tests/guided_mech_ref.potential) + zeta_comp C for compliance_form 'energy', and
Phi4 = Phi - zeta_comp C(sg(U), rho) for 'sensitivity' (sg = stop-gradient; U is linear in channels 0 and 1 of x0, so detaching those
channels is detaching U).  The reported fourth sum is C in both forms.  Every function works in the dtype it is given: float64 is
the reference and the same text in float32 is the yardstick."""
import torch

from oracle import pidm_oracle as O
from tests import guided_mech_ref as R
from tests import mech_ref as MR
from tests.guided_ref import _default_float64

FORMS = ("energy", "sensitivity")


def compliance(x0, bcs, vf, kloc, elem_dofs):
    """C [B] of x0 [B,3,nel,nel] in x0.dtype (differentiable); kloc [8,8] (uniform mesh: the oracle's function) or [E,8,8]"""
    kloc = torch.as_tensor(kloc)
    if kloc.dim() == 2:
        return O.mechanics_residual(x0, bcs, vf, kloc.to(x0.dtype), elem_dofs)[1]
    return MR.residual_ref(x0, bcs, vf, kloc, elem_dofs)[2]


def potential(x0, bcs, vf, y, m, zetas, form, kloc, elem_dofs):
    """(Phi4 [B], sums [B,4] = (L_obs, L_pde, L_vol, C), model_out); zetas = (obs, pde, vol, comp)"""
    assert form in FORMS, form
    phi, sums, mo = R.potential(x0, bcs, vf, y, m, zetas[:3], kloc, elem_dofs)
    c = compliance(x0, bcs, vf, kloc, elem_dofs)
    if form == "energy":
        phi = phi + zetas[3] * c
    else:
        x_sg = torch.cat((x0[:, :2].detach(), x0[:, 2:]), dim=1)
        phi = phi - zetas[3] * compliance(x_sg, bcs, vf, kloc, elem_dofs)
    return phi, torch.cat((sums, c[:, None]), dim=1), mo


def cotangent(x0, bcs, vf, y, m, zetas, form, kloc, elem_dofs, dtype=torch.float64):
    """v = dPhi4/dx0 [B,3,nel,nel], model_out [B,3,nn,nn] and sums [B,4] in `dtype`"""
    x = x0.detach().to(dtype).clone().requires_grad_(True)
    phi, sums, mo = potential(x, bcs.to(dtype), vf.to(dtype), y.to(dtype), m.to(dtype), zetas, form, torch.as_tensor(kloc).to(dtype),
                              elem_dofs)
    (v,) = torch.autograd.grad(phi.sum(), x)
    return v.detach(), mo.detach(), sums.detach()


def guided_step(p, cfg, tables, x_t, cond, bcs, t, z, y, m, zetas, form, kloc, elem_dofs, surpress_noise=True, dtype=torch.float64):
    """tests/guided_mech_ref.guided_step with the four-term potential: (x_{t-1}, sums [B,4], g = dPhi4/dx_t [B,3,nn,nn])"""
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
    phi, sums, mo = potential(x0, bcs, cond[:, 0, 0, 0], y.to(dtype), m.to(dtype), zetas, form, torch.as_tensor(kloc).to(dtype), elem_dofs)
    (g,) = torch.autograd.grad(phi.sum(), x)
    x_prev = O.p_sample_update(tables, mo.detach(), x.detach(), t, z.to(dtype), surpress_noise=surpress_noise) - g
    return x_prev.detach(), sums.detach(), g.detach()
