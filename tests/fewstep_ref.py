"""Float64 restatement of few-step (strided DDIM) sampling, built only from oracle.pidm_oracle functions, the restatements
tests/guided_ref.py and tests/guided_mech_ref.py, and torch autograd.  TEST INFRASTRUCTURE for tests/test_fewstep_sampling.py: no
project kernel and no method of DenoisingDiffusion is called - the coefficient algebra is restated here on its own.

A strided step from level t to level t_prev < t (t_prev = -1: the clean sample, abar_prev = 1) on the x0 estimate:
    x_prev = sqrt(p) x0 + sqrt(1 - p - sigma^2) eps + sigma z,   eps = (x_t - sqrt(a) x0) / sqrt(1 - a),   a = abar_t, p = abar_prev,
    sigma  = eta sqrt((1 - p) / (1 - a)) sqrt(1 - a / p)                                                    (Song et al., DDIM)
which `step_coefs` collects as x_prev = c1 x0 + c2 x_t + sigma z.  `abar` is what the engine's loops read: the fp32 schedule table
`alphas_prod`, widened to float64 (tests/guided_ref.tables64)."""
import torch

from oracle import pidm_oracle as O
from tests import guided_mech_ref as GM
from tests import guided_ref as GR
from tests.guided_ref import _default_float64


def step_coefs(abar, t, t_prev, eta):
    """(c1, c2, sigma) as float64 0-d tensors; abar: 1-D float64 tensor"""
    abar = torch.as_tensor(abar, dtype=torch.float64)
    a = abar[t]
    p = abar[t_prev] if t_prev >= 0 else torch.ones((), dtype=torch.float64)
    sigma = eta * torch.sqrt((1 - p) / (1 - a)) * torch.sqrt(torch.clamp(1 - a / p, min=0.0))
    eps_coef = torch.sqrt(torch.clamp(1 - p - sigma ** 2, min=0.0))
    # x_prev = sqrt(p) x0 + eps_coef (x_t - sqrt(a) x0) / sqrt(1 - a) + sigma z
    c2 = eps_coef / torch.sqrt(1 - a)
    c1 = torch.sqrt(p) - c2 * torch.sqrt(a)
    return c1, c2, sigma


def pairs(levels):
    """[(t, t_prev)] of a descending list of visited levels; the last one steps to -1"""
    return list(zip(levels, list(levels[1:]) + [-1]))


def update(abar, x0, x_t, t, t_prev, z, eta):
    c1, c2, sigma = step_coefs(abar, t, t_prev, eta)
    return c1 * x0.double() + c2 * x_t.double() + sigma * z.double()


# ---- Gaussian data: the exact posterior mean, the probability-flow end point, and the DDIM chain in float64 ---------------------
def gaussian_posterior_mean(x_t, abar_t, mu, s):
    """E[x0 | x_t] for x0 ~ N(mu, s^2), x_t = alpha x0 + sqrt(1 - alpha^2) eps, alpha = sqrt(abar_t)"""
    alpha = float(abar_t) ** 0.5
    return mu + (alpha * s * s / (alpha * alpha * s * s + 1.0 - alpha * alpha)) * (x_t - alpha * mu)


def gaussian_flow_endpoint(x_T, abar_T, mu, s):
    """where the probability-flow ODE takes x_T (at the level with abar_T) at t -> clean: the marginals N(alpha mu, alpha^2 s^2 +
    1 - alpha^2) are mapped onto each other by the affine map that keeps the standardised coordinate"""
    alpha = float(abar_T) ** 0.5
    return mu + s * (x_T.double() - alpha * mu) / (alpha * alpha * s * s + 1.0 - alpha * alpha) ** 0.5


def gaussian_chain(abar, levels, x_T, mu, s, eta=0.0, noises=None):
    """the strided chain from x_T over `levels` with the exact posterior mean as the model, float64"""
    abar = torch.as_tensor(abar, dtype=torch.float64)
    x = x_T.double()
    for k, (t, t_prev) in enumerate(pairs(levels)):
        x0 = gaussian_posterior_mean(x, abar[t], mu, s)
        z = torch.zeros_like(x) if noises is None else noises[k].double()
        x = update(abar, x0, x, t, t_prev, z, eta)
    return x


# ---- one strided step with the UNet: plain, guided Darcy, guided mechanics --------------------------------------------------------
def plain_step_strided(p64, cfg, abar, x_t, t, t_prev, z, eta):
    """(x_prev, x0_hat) of one unguided strided Darcy step from x_t [B,2,P,P], float64"""
    B = x_t.shape[0]
    with _default_float64():
        x0 = O.unet_forward(p64, x_t.detach().double(), torch.full((B,), t, dtype=torch.long), cfg)
    assert x0.dtype == torch.float64
    return update(abar, x0, x_t, t, t_prev, z, eta), x0


def guided_step_strided(p64, cfg, abar, x_t, t, t_prev, z, eta, y, m, zeta_obs, zeta_pde):
    """tests/guided_ref.guided_step with the strided coefficients: (x_prev, sums [B,2], g = dPhi/dx_t), float64.  The guidance term
    is subtracted as it is (no rescaling by the stride)."""
    B = x_t.shape[0]
    x = x_t.detach().double().clone().requires_grad_(True)
    with _default_float64():
        x0 = O.unet_forward(p64, x, torch.full((B,), t, dtype=torch.long), cfg)
    assert x0.dtype == torch.float64
    phi, l_obs, l_pde = GR.potential(x0, y.double(), m.double(), zeta_obs, zeta_pde)
    g = torch.autograd.grad(phi.sum(), x, allow_unused=True)[0] if phi.requires_grad else None
    if g is None:
        g = torch.zeros_like(x)
    x_prev = update(abar, x0.detach(), x.detach(), t, t_prev, z, eta) - g
    return x_prev.detach(), torch.stack([l_obs, l_pde], dim=1).detach(), g.detach()


def guided_mech_step_strided(p64, cfg, abar, x_t, cond, bcs, t, t_prev, z, eta, y, m, zetas, kloc, elem_dofs):
    """tests/guided_mech_ref.guided_step (which hard-codes the ancestral update) with the strided coefficients:
    (x_prev, sums [B,3], g = dPhi/dx_t [B,3,nn,nn]), float64"""
    dt = torch.float64
    B, nel = x_t.shape[0], x_t.shape[-1] - 1
    x = x_t.detach().to(dt).clone().requires_grad_(True)
    cond, bcs = cond.to(dt), bcs.to(dt)
    net_in = torch.cat((O.bilinear_resize(x, nel), O.bilinear_resize(cond, nel), O.bilinear_resize(bcs, nel)), dim=1)
    with _default_float64():
        x0 = O.unet_forward(p64, net_in, torch.full((B,), t, dtype=torch.long), cfg)
    assert x0.dtype == dt
    phi, sums, mo = GM.potential(x0, bcs, cond[:, 0, 0, 0], y.to(dt), m.to(dt), zetas, torch.as_tensor(kloc).to(dt), elem_dofs)
    g = torch.autograd.grad(phi.sum(), x, allow_unused=True)[0] if phi.requires_grad else None
    if g is None:
        g = torch.zeros_like(x)
    x_prev = update(abar, mo.detach(), x.detach(), t, t_prev, z, eta) - g
    return x_prev.detach(), sums.detach(), g.detach()
