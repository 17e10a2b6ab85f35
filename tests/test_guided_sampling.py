"""Posterior guidance of the Darcy sampler (csrc/k_guidance.hip, DenoisingDiffusion.p_sample_loop_guided) against the float64
restatement tests/guided_ref.py.  `backend` = host emulator or the gfx950 library (-m gpu)."""
import ctypes as C

import pytest
import torch

from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd._lib import PidmError
from physicsinformeddiffusionmodels_amd.denoising_utils import DenoisingDiffusion
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
from tests import guided_ref as R
from tests.test_training_step import patched_rng, setup

ZO, ZP = 1.0, 1e-3      # both terms of v then have the same order of magnitude (|J^T r| / |r| ~ 1 / h^2)


def make_res(backend, P, fd_acc=2, bcs='none'):
    L, dev = backend
    return ResidualsDarcy(model=None, fd_acc=fd_acc, pixels_per_dim=P, pixels_at_boundary=True, reverse_d1=True, device=dev, bcs=bcs,
                          lib=L if dev.type == "cpu" else None), dev


def fields(P, B, seed=0):
    """x0 estimate with K <- exp(0.5 randn) (as tests/test_darcy_general.py), observations of the same kind"""
    g = torch.Generator().manual_seed(100 * P + B + seed)
    x = torch.randn(B, 2, P, P, generator=g)
    x[:, 1] = torch.exp(0.5 * x[:, 1])
    y = torch.randn(B, 2, P, P, generator=g)
    y[:, 1] = torch.exp(0.5 * y[:, 1])
    return x, y, g


def mask_of(kind, B, P, g):
    m = torch.zeros(B, 2, P, P)
    if kind == "K":
        m[:, 1] = 1.0
    elif kind == "sparse":
        m = (torch.rand(B, 2, P, P, generator=g) < 0.1).float()
    else:
        assert kind == "none"
    return m


CASES = [("K", ZO, ZP), ("sparse", ZO, ZP), ("none", ZO, ZP), ("sparse", ZO, 0.0), ("sparse", 0.0, ZP)]
_ref_cache = {}


def reference(P, B, kind, zo, zp):
    key = (P, B, kind, zo, zp)
    if key not in _ref_cache:
        x, y, g = fields(P, B)
        m = mask_of(kind, B, P, g)
        v, s = R.cotangent(x, y, m, zo, zp)
        _ref_cache[key] = (x, y, m, v, s)
    return _ref_cache[key]


def check_cotangent(v, s, v_ref, s_ref, zo, zp):
    print("sums", s.tolist(), "ref", s_ref.tolist())
    rel_s = ((s.double() - s_ref).abs() / s_ref.abs().clamp_min(1e-300)).where(s_ref != 0, s.double().abs())
    print("sums rel err", rel_s.tolist())
    vmax = v_ref.abs().amax(dim=(1, 2, 3))
    err = (v.double() - v_ref).abs().amax(dim=(1, 2, 3))
    print("v err", err.tolist(), "v max", vmax.tolist())
    assert torch.isfinite(v).all() and torch.isfinite(s).all()
    assert (rel_s <= 1e-5).all()
    assert (err <= 1e-5 * vmax).all()
    if zo == 0.0 and zp == 0.0:
        assert (v == 0).all()


@pytest.mark.parametrize("kind,zo,zp", CASES)
@pytest.mark.parametrize("P,B", [(10, 3), (16, 3), (21, 2), (64, 2)])
def test_cotangent_kernel_vs_float64(backend, P, B, kind, zo, zp):
    res, dev = make_res(backend, P)
    x, y, m, v_ref, s_ref = reference(P, B, kind, zo, zp)
    v, s = res.guidance_cotangent(x.to(dev), y.to(dev), m.to(dev), zo, zp)
    if kind == "none":
        assert (s[:, 0] == 0).all()         # the observation term is exactly zero (and omitted: everything stays finite)
    check_cotangent(v.cpu(), s.cpu(), v_ref, s_ref, zo, zp)


def test_cotangent_beyond_the_lds_resident_size(backend):
    """P = 80 does not fit one workgroup's LDS (8 P^2 floats): ResidualsDarcy composes residual -> scale -> adjoint -> add on the
    second-order kernels instead; same restatement, same bounds."""
    P, B = 80, 1
    res, dev = make_res(backend, P)
    assert res.specialised
    x, y, m, v_ref, s_ref = reference(P, B, "sparse", ZO, ZP)
    v, s = res.guidance_cotangent(x.to(dev), y.to(dev), m.to(dev), ZO, ZP)
    check_cotangent(v.cpu(), s.cpu(), v_ref, s_ref, ZO, ZP)


def test_cotangent_kernel_is_deterministic_and_batch_independent(backend):
    P = 21
    res, dev = make_res(backend, P)
    x, y, g = fields(P, 3)
    m = mask_of("sparse", 3, P, g)
    x, y, m = x.to(dev), y.to(dev), m.to(dev)
    v1, s1 = res.guidance_cotangent(x, y, m, ZO, ZP)
    v2, s2 = res.guidance_cotangent(x, y, m, ZO, ZP)
    assert torch.equal(v1, v2) and torch.equal(s1, s2)
    for b in range(3):
        vb, sb = res.guidance_cotangent(x[b:b + 1], y[b:b + 1], m[b:b + 1], ZO, ZP)
        assert torch.equal(vb[0], v1[b]) and torch.equal(sb[0], s1[b]), b


@pytest.mark.parametrize("fd_acc,bcs", [(4, 'none'), (2, 'periodic')])
def test_general_path_vs_autograd_of_residual_of(backend, fd_acc, bcs):
    P, B = 16, 3
    res, dev = make_res(backend, P, fd_acc, bcs)
    assert not res.specialised
    x, y, g = fields(P, B, seed=1)
    m = mask_of("sparse", B, P, g)
    x, y, m = x.to(dev), y.to(dev), m.to(dev)
    xr = x.clone().requires_grad_(True)
    r = res.residual_of(xr)
    l_obs, l_pde = (m * (xr - y) ** 2).sum(dim=(1, 2, 3)), (r ** 2).sum(dim=(1, 2))
    phi = ZO * torch.sqrt(l_obs) + ZP * torch.sqrt(l_pde)
    (v_ref,) = torch.autograd.grad(phi.sum(), xr)
    v, s = res.guidance_cotangent(x, y, m, ZO, ZP)
    check_cotangent(v.cpu(), s.cpu(), v_ref.detach().cpu().double(), torch.stack([l_obs, l_pde], dim=1).detach().cpu().double(), ZO, ZP)
    v2, s2 = res.guidance_cotangent(x, y, m, ZO, ZP)
    assert torch.equal(v, v2) and torch.equal(s, s2)
    # an absent observation term: exactly the scaled adjoint, finite
    v0, s0 = res.guidance_cotangent(x, y, torch.zeros_like(m), ZO, ZP)
    assert (s0[:, 0] == 0).all() and torch.isfinite(v0).all()


@pytest.mark.parametrize("B,C_,HW", [(2, 2, 256), (3, 2, 21 * 21), (1, 3, 70)])
def test_guided_update_kernel(backend, B, C_, HW):
    L, dev = backend
    g = torch.Generator().manual_seed(HW)
    x0p, xt, z = (torch.randn(B, C_, HW, generator=g).to(dev) for _ in range(3))
    gr = torch.randn(B, HW, C_, generator=g).to(dev)
    c1, c2, sg = 0.3125, 0.71875, 0.09
    out = torch.full_like(xt, float('nan'))
    vp = lambda a: C.c_void_p(a.data_ptr())
    L.check(L.pidm_psample_update_guided(vp(x0p), vp(xt), vp(z), vp(gr), c1, c2, sg, vp(out), B, C_, HW, None), "update")
    ref = c1 * x0p + c2 * xt + sg * z - gr.permute(0, 2, 1)
    assert (out - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()


def _loop_setup(backend, n_steps=3):
    dim, P, B = 8, 16, 2
    m, _, res, dev = setup(backend, dim, P, 100)
    L = backend[0]
    diff = DenoisingDiffusion(n_steps, dev, lib=L if dev.type == "cpu" else None)
    g = torch.Generator().manual_seed(3)
    noises = [torch.randn(B, 2, P, P, generator=g) for _ in range(n_steps + 1)]
    obs = torch.randn(B, 2, P, P, generator=g)
    obs[:, 1] = torch.exp(0.5 * obs[:, 1])
    mask = (torch.rand(B, 2, P, P, generator=g) < 0.1).float()
    mask[:, 1] = 1.0                                    # K fully observed + a few pressure readings
    return m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps)


def _run(diff, dev, noises, fn):
    it = iter(noises)
    with patched_rng(randn=lambda *a, **k: next(it).clone().to(dev), randn_like=lambda *a, **k: next(it).clone().to(dev)):
        return fn()


def test_guided_loop_teacher_forced(backend):
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend)
    (x_seq, interm), aux = _run(diff, dev, noises, lambda: diff.p_sample_loop_guided((B, 2, P, P), res, obs.to(dev), mask.to(dev),
                                                                                     zeta_obs=ZO, zeta_pde=ZP))
    assert len(x_seq) == n_steps + 1 and len(interm) == n_steps + 1
    assert aux['guidance'].shape == (n_steps, B, 2) and aux['guidance'].device.type == dev.type
    assert aux['residual'].shape == (B,)
    cfg = O.UnetCfg(dim=dim, channels=2)
    p64 = R.params64(m.state_dict())
    tables = R.tables64(n_steps)
    assert torch.equal(x_seq[0], noises[0])
    for step, t in enumerate(reversed(range(n_steps))):
        # teacher forcing: the restatement advances the engine's own previous state
        x_ref, s_ref, g_ref = R.guided_step(p64, cfg, tables, x_seq[step], t, noises[1 + step], obs, mask, ZO, ZP)
        err = (x_seq[1 + step].double() - x_ref).abs().max().item()
        bound = 5e-5 * max(x_ref.abs().max().item(), 1.0) + 2e-4 * g_ref.abs().max().item()
        print(f"t={t}: err {err:.3e} bound {bound:.3e} |g| {g_ref.abs().max().item():.3e}")
        assert g_ref.abs().max().item() > 0
        assert err <= bound, f"step t={t}"
        s = aux['guidance'][step].cpu().double()
        print("sums", s.tolist(), "ref", s_ref.tolist())
        assert ((s - s_ref).abs() <= 1e-4 * s_ref.abs()).all(), f"step t={t}"
    r_ref = O.darcy_residual(x_seq[-1].double()).abs().mean(dim=(1, 2))
    assert ((aux['residual'].cpu().double() - r_ref).abs() <= 1e-4 * r_ref).all()


def test_guided_loop_without_guidance_equals_p_sample_loop(backend):
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend)
    plain, _ = _run(diff, dev, noises, lambda: diff.p_sample_loop(None, (B, 2, P, P), save_output=True, residual_func=res))
    (x_seq, _), aux = _run(diff, dev, noises, lambda: diff.p_sample_loop_guided((B, 2, P, P), res, obs.to(dev), mask.to(dev),
                                                                                zeta_obs=0.0, zeta_pde=0.0))
    err = (x_seq[-1] - plain[-1]).abs().max().item()
    assert err <= 5e-5 * max(plain[-1].abs().max().item(), 1.0)
    assert (aux['guidance'] > 0).all()                  # the sums are reported whatever the weights are


def test_guided_loop_replace_observed_and_broadcast(backend):
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend)
    obs1, mask1 = obs[:1], mask[:1]
    (x_seq, interm), aux = _run(diff, dev, noises, lambda: diff.p_sample_loop_guided(
        (B, 2, P, P), res, obs1.to(dev), mask1.to(dev), zeta_obs=ZO, zeta_pde=ZP, guide_below=1, replace_observed=True, keep_history=False))
    # steps t = 2, 1 are plain p_sample arithmetic (no sums), t = 0 is guided
    assert (aux['guidance'][:2] == 0).all() and (aux['guidance'][2] > 0).all()
    assert len(x_seq) == 1 and x_seq[0].device.type == dev.type
    x = x_seq[0].cpu()
    on = mask1.expand(B, -1, -1, -1) != 0
    assert torch.equal(x[on], obs1.expand(B, -1, -1, -1)[on])
    assert not torch.equal(x[~on], obs1.expand(B, -1, -1, -1)[~on])


def test_guidance_errors(backend):
    L, dev = backend
    m, diff, res, dev, noises, obs, mask, (dim, P, B, n_steps) = _loop_setup(backend)
    shape = (B, 2, P, P)

    class Mech:
        gov_eqs = 'mechanics'
        model = m
    with pytest.raises(PidmError, match="Darcy only"):
        diff.p_sample_loop_guided(shape, Mech(), obs, mask)
    with pytest.raises(PidmError, match="obs must be"):
        diff.p_sample_loop_guided(shape, res, obs[:, :, :8], mask)
    with pytest.raises(PidmError, match="mask must be"):
        diff.p_sample_loop_guided(shape, res, obs, mask[:, :1])
    with pytest.raises(PidmError, match="obs must be"):
        diff.p_sample_loop_guided((3, 2, P, P), res, obs, mask)
    res.model = type(m)(dim=8, channels=2, self_condition=True)
    with pytest.raises(PidmError, match="self-conditioning"):
        diff.p_sample_loop_guided(shape, res, obs, mask)
    # the C entries
    vp = lambda a: C.c_void_p(a.data_ptr())
    x = torch.zeros(1, 2, 4, 4, device=dev)
    big = torch.zeros(1, device=dev)       # never dereferenced: the size checks come first
    s = torch.zeros(1, 2, device=dev)
    f = torch.zeros(16, device=dev)
    for P_bad in (4, 72, 128):
        assert L.pidm_darcy_guidance_cotangent(vp(big), vp(big), vp(big), vp(big), 1.0, -1.0, 1.0, 1.0, vp(big), vp(s), 1, P_bad, None) != 0
        assert str(P_bad).encode() in L.pidm_last_error()
    assert L.pidm_darcy_guidance_cotangent(vp(x), vp(x), vp(x), vp(f), 1.0, -1.0, 1.0, 1.0, vp(x), vp(s), 0, 16, None) != 0
    assert b"B>0" in L.pidm_last_error()
    assert L.pidm_darcy_guidance_cotangent(vp(x), None, vp(x), vp(f), 1.0, -1.0, 1.0, 1.0, vp(x), vp(s), 1, 16, None) != 0
    assert b"null" in L.pidm_last_error()
    assert L.pidm_guidance_scale_general(vp(x), vp(x), vp(x), None, 1.0, 1.0, vp(x), vp(x), vp(s), 1, 4, None) != 0
    assert b"null" in L.pidm_last_error()
    assert L.pidm_guidance_scale_general(vp(x), vp(x), vp(x), vp(x), 1.0, 1.0, vp(x), vp(x), vp(s), -2, 4, None) != 0
    assert b"B>0" in L.pidm_last_error()
    assert L.pidm_guidance_add(None, vp(x), 4, None) != 0 and b"null" in L.pidm_last_error()
    assert L.pidm_psample_update_guided(vp(x), vp(x), vp(x), None, 1.0, 1.0, 1.0, vp(x), 1, 2, 16, None) != 0
    assert b"null" in L.pidm_last_error()
    assert L.pidm_psample_update_guided(vp(x), vp(x), vp(x), vp(x), 1.0, 1.0, 1.0, vp(x), 0, 2, 16, None) != 0
    assert b"B" in L.pidm_last_error()
    assert L.pidm_psample_update_guided(vp(x), vp(x), vp(x), vp(x), 1.0, 1.0, 1.0, vp(x), 1, 17, 16, None) != 0
    assert b"C=17" in L.pidm_last_error()
