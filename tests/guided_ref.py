"""Float64 restatement of posterior guidance for the Darcy sampler, built only from oracle.pidm_oracle functions (unet_forward,
darcy_residual, p_sample_update, diffusion_tables) and torch autograd.  TEST INFRASTRUCTURE for tests/test_guided_sampling.py.

Per sample: L_obs = sum m (x - y)^2, L_pde = sum r(x)^2, Phi = zeta_obs sqrt(L_obs) + zeta_pde sqrt(L_pde); a term whose L is exactly
0 is omitted.  One guided step: x_{t-1} = p_sample_update(x0_hat(x_t), x_t) - d Phi(x0_hat(x_t)) / d x_t."""
import torch

from oracle import pidm_oracle as O


class _default_float64:
    """O.time_embedding builds its sinusoid table in the DEFAULT dtype: float64 for the duration of a restated UNet call"""

    def __enter__(self):
        self.prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *a):
        torch.set_default_dtype(self.prev)


def sums_of(xh, y, m):
    """(L_obs [B], L_pde [B]) of xh [B,2,P,P] (any float dtype; differentiable)"""
    r = O.darcy_residual(xh)
    return (m * (xh - y) ** 2).sum(dim=(1, 2, 3)), (r ** 2).sum(dim=(1, 2))


def _sqrt_or_omit(L):
    on = L > 0
    return torch.sqrt(torch.where(on, L, torch.ones_like(L))) * on.to(L.dtype)


def potential(xh, y, m, zeta_obs, zeta_pde):
    l_obs, l_pde = sums_of(xh, y, m)
    return zeta_obs * _sqrt_or_omit(l_obs) + zeta_pde * _sqrt_or_omit(l_pde), l_obs, l_pde


def cotangent(xh, y, m, zeta_obs, zeta_pde):
    """v = dPhi/dxh [B,2,P,P] and sums [B,2], float64"""
    x = xh.detach().double().clone().requires_grad_(True)
    phi, l_obs, l_pde = potential(x, y.double(), m.double(), zeta_obs, zeta_pde)
    if phi.requires_grad:
        (v,) = torch.autograd.grad(phi.sum(), x, allow_unused=True)
    else:
        v = None
    if v is None:
        v = torch.zeros_like(x)
    return v.detach(), torch.stack([l_obs, l_pde], dim=1).detach()


def params64(state_dict):
    return {k: (v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu()) for k, v in state_dict.items()}


def tables64(n_steps):
    return {k: v.double() for k, v in O.diffusion_tables(n_steps).items()}


def guided_step(p64, cfg, tables, x_t, t, z, y, m, zeta_obs, zeta_pde, surpress_noise=True):
    """One guided ancestral step from x_t [B,2,P,P]: returns (x_{t-1}, sums [B,2], g = dPhi/dx_t [B,2,P,P]), float64."""
    B = x_t.shape[0]
    x = x_t.detach().double().clone().requires_grad_(True)
    with _default_float64():
        x0 = O.unet_forward(p64, x, torch.full((B,), t, dtype=torch.long), cfg)
    assert x0.dtype == torch.float64
    phi, l_obs, l_pde = potential(x0, y.double(), m.double(), zeta_obs, zeta_pde)
    g = torch.autograd.grad(phi.sum(), x, allow_unused=True)[0] if phi.requires_grad else None
    if g is None:
        g = torch.zeros_like(x)
    x_prev = O.p_sample_update(tables, x0.detach(), x.detach(), t, z.double(), surpress_noise=surpress_noise) - g
    return x_prev.detach(), torch.stack([l_obs, l_pde], dim=1).detach(), g.detach()
