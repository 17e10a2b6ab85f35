"""Float64 restatement of flux-conditioned posterior guidance for the Darcy sampler.  TEST INFRASTRUCTURE for
tests/test_guided_flux.py; extends tests/guided_ref.py (oracle.pidm_oracle functions + torch autograd) by the flux term.

The Darcy flux of x = (p, K) is q = (-K D0 p, -K D1 p) with D0 / D1 the first-derivative operators of the residual.  They are
built HERE as dense P x P float64 matrices from the textbook rule (weights solve the moment equations on the stencil's offsets:
central in the interior, one-sided within acc/2 of an edge, wrapped when periodic) - nothing is taken from the package.
L_flux = sum m_q (q - y_q)^2, Phi = zeta_obs sqrt(L_obs) + zeta_pde sqrt(L_pde) + zeta_flux sqrt(L_flux); a term whose L is
exactly 0 is omitted."""
import math

import numpy as np
import torch

from oracle import pidm_oracle as O
from tests import guided_ref as R


def _weights(offsets, deriv=1):
    """c_k with sum_k c_k o_k^m = m! [m == deriv], m = 0 .. n-1 (float64 solve of the moment equations)"""
    o = np.asarray(offsets, dtype=np.float64)
    A = np.vander(o, len(o), increasing=True).T
    rhs = np.zeros(len(o))
    rhs[deriv] = math.factorial(deriv)
    return np.linalg.solve(A, rhs)


def d1_matrix(P, h, acc=2, periodic=False):
    """Dense first-derivative operator of accuracy order acc on P points of spacing h (h may be negative): [P,P] float64"""
    half = acc // 2
    D = np.zeros((P, P))
    central = list(range(-half, half + 1))
    for i in range(P):
        if periodic or half <= i < P - half:
            offs = central
        elif i < half:
            offs = list(range(0, acc + 1))
        else:
            offs = [-k for k in range(0, acc + 1)]
        for o, w in zip(offs, _weights(offs)):
            D[i, (i + o) % P] += w / h
    return torch.from_numpy(D)


def spacings(P, pixels_at_boundary=True, reverse_d1=True):
    h0 = 1.0 / (P - 1) if pixels_at_boundary else 1.0 / P
    return h0, (-h0 if reverse_d1 else h0)


def flux(x, acc=2, periodic=False, pixels_at_boundary=True, reverse_d1=True):
    """q [B,2,P,P] of x [B,2,P,P] (float64, differentiable)"""
    P = x.shape[-1]
    h0, h1 = spacings(P, pixels_at_boundary, reverse_d1)
    D0, D1 = d1_matrix(P, h0, acc, periodic).to(x.dtype), d1_matrix(P, h1, acc, periodic).to(x.dtype)
    p, K = x[:, 0], x[:, 1]
    return torch.stack([-K * (D0 @ p), -K * (p @ D1.T)], dim=1)


def potential(xh, y, m, yq, mq, zeta_obs, zeta_pde, zeta_flux):
    l_obs, l_pde = R.sums_of(xh, y, m)
    l_flux = (mq * (flux(xh) - yq) ** 2).sum(dim=(1, 2, 3))
    phi = zeta_obs * R._sqrt_or_omit(l_obs) + zeta_pde * R._sqrt_or_omit(l_pde) + zeta_flux * R._sqrt_or_omit(l_flux)
    return phi, torch.stack([l_obs, l_pde, l_flux], dim=1)


def _grad(phi, x):
    g = torch.autograd.grad(phi.sum(), x, allow_unused=True)[0] if phi.requires_grad else None
    return torch.zeros_like(x) if g is None else g


def cotangent(xh, y, m, yq, mq, zeta_obs, zeta_pde, zeta_flux):
    """v = dPhi/dxh [B,2,P,P] and sums [B,3], float64"""
    x = xh.detach().double().clone().requires_grad_(True)
    phi, sums = potential(x, y.double(), m.double(), yq.double(), mq.double(), zeta_obs, zeta_pde, zeta_flux)
    return _grad(phi, x).detach(), sums.detach()


def part_maxima(xh, y, m, yq, mq):
    """per-sample max |dPhi/dx| of each term alone at unit weight: [B,3]"""
    out = []
    for z in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)):
        v, _ = cotangent(xh, y, m, yq, mq, *z)
        out.append(v.abs().amax(dim=(1, 2, 3)))
    return torch.stack(out, dim=1)


def guided_step(p64, cfg, tables, x_t, t, z, y, m, yq, mq, zeta_obs, zeta_pde, zeta_flux, surpress_noise=True):
    """One guided ancestral step from x_t [B,2,P,P]: (x_{t-1}, sums [B,3], g = dPhi/dx_t [B,2,P,P]), float64."""
    B = x_t.shape[0]
    x = x_t.detach().double().clone().requires_grad_(True)
    with R._default_float64():
        x0 = O.unet_forward(p64, x, torch.full((B,), t, dtype=torch.long), cfg)
    assert x0.dtype == torch.float64
    phi, sums = potential(x0, y.double(), m.double(), yq.double(), mq.double(), zeta_obs, zeta_pde, zeta_flux)
    g = _grad(phi, x)
    x_prev = O.p_sample_update(tables, x0.detach(), x.detach(), t, z.double(), surpress_noise=surpress_noise) - g
    return x_prev.detach(), sums.detach(), g.detach()
