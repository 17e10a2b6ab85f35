"""Flux observations in the guided Darcy sampler (csrc/k_guidance.hip: guidance_cotangent_flux_kernel, guidance_flux_general_kernel,
darcy_flux_kernel; ResidualsDarcy.flux_of / guidance_cotangent, DenoisingDiffusion.p_sample_loop_guided) against the float64
restatement tests/guided_flux_ref.py.  `backend` = host emulator or the gfx950 library (-m gpu).

Bounds are those of tests/test_guided_sampling.py for this kernel family (same fp32 stencil sums, same fp64 reductions):
sums 1e-5 relative, v 1e-5 of its per-sample maximum, flux_of 2e-6 max-norm relative."""
import ctypes as C

import pytest
import torch

from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd._lib import PidmError
from physicsinformeddiffusionmodels_amd.grad_utils import _ops_array
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
from tests import guided_flux_ref as F
from tests import guided_ref as R
from tests.test_guided_sampling import ZO, ZP, _loop_setup, _run, fields, make_res, mask_of

ZF_LOOP = 0.05      # |D^T (K e)| / |e| ~ K / h = 15 K at P = 16: the flux part of g is then of the order of the observation part


def flux_data(P, B, g, kind):
    """y_q ~ N(0,1); m_q: sparse (rand < 0.1), the four edges (rows 0 / P-1 of q0, columns 0 / P-1 of q1), or all zero"""
    yq = torch.randn(B, 2, P, P, generator=g)
    mq = torch.zeros(B, 2, P, P)
    if kind == "sparse":
        mq = (torch.rand(B, 2, P, P, generator=g) < 0.1).float()
    elif kind == "edges":
        mq[:, 0, 0, :] = mq[:, 0, -1, :] = 1.0
        mq[:, 1, :, 0] = mq[:, 1, :, -1] = 1.0
    else:
        assert kind == "zero"
    return yq, mq


_data_cache, _ref_cache = {}, {}


def data(P, B, kind):
    if (P, B, kind) not in _data_cache:
        x, y, g = fields(P, B)
        m = mask_of("sparse", B, P, g)
        yq, mq = flux_data(P, B, g, kind)
        zp = zf = None
        if kind != "zero":
            # zeta_pde / zeta_flux from the REFERENCE's own parts at unit weight: each balanced against the observation part (batch
            # mean of the ratio of the maxima, one significant digit).  |J^T r| / |r| ~ 1 / h^2 and |D^T K e| / |e| ~ 1 / h: a fixed
            # pair of weights cannot balance the three parts at every P
            pm = F.part_maxima(x, y, m, yq, mq)
            zp = float(f"{(ZO * pm[:, 0] / pm[:, 1]).mean().item():.0e}")
            zf = float(f"{(ZO * pm[:, 0] / pm[:, 2]).mean().item():.0e}")
        _data_cache[(P, B, kind)] = (x, y, m, yq, mq, zp, zf)
    return _data_cache[(P, B, kind)]


def reference(P, B, kind, zo, zp, zf):
    key = (P, B, kind, zo, zp, zf)
    if key not in _ref_cache:
        x, y, m, yq, mq, _, _ = data(P, B, kind)
        _ref_cache[key] = F.cotangent(x, y, m, yq, mq, zo, zp, zf)
    return _ref_cache[key]


def check(v, s, v_ref, s_ref):
    print("sums", s.tolist(), "ref", s_ref.tolist())
    rel_s = ((s.double() - s_ref).abs() / s_ref.abs().clamp_min(1e-300)).where(s_ref != 0, s.double().abs())
    print("sums rel err", rel_s.tolist())
    vmax = v_ref.abs().amax(dim=(1, 2, 3))
    err = (v.double() - v_ref).abs().amax(dim=(1, 2, 3))
    print("v err / v max", (err / vmax).tolist(), "v max", vmax.tolist())
    assert torch.isfinite(v).all() and torch.isfinite(s).all()
    assert (rel_s <= 1e-5).all()
    assert (err <= 1e-5 * vmax).all()


def call(res, dev, x, y, m, yq, mq, zo, zp, zf):
    v, s = res.guidance_cotangent(x.to(dev), y.to(dev), m.to(dev), zo, zp, flux_obs=yq.to(dev), flux_mask=mq.to(dev), zeta_flux=zf)
    assert tuple(s.shape) == (x.shape[0], 3)
    return v.cpu(), s.cpu()


# ---- 1. flux_of ------------------------------------------------------------------------------------------------------------------
FLUX_OF = [(2, 'none', 10, True, True), (2, 'none', 16, True, True), (2, 'none', 21, True, True), (2, 'none', 64, True, True),
           (4, 'none', 16, True, True), (6, 'none', 16, True, True), (2, 'periodic', 16, True, True), (4, 'periodic', 16, True, True),
           (2, 'none', 16, False, True), (4, 'periodic', 16, False, True), (2, 'none', 21, True, False)]


@pytest.mark.parametrize("acc,bcs,P,rev,pab", FLUX_OF)
def test_flux_of_vs_float64(backend, acc, bcs, P, rev, pab):
    L, dev = backend
    res = ResidualsDarcy(model=None, fd_acc=acc, pixels_per_dim=P, pixels_at_boundary=pab, reverse_d1=rev, device=dev, bcs=bcs,
                         lib=L if dev.type == "cpu" else None)
    x, _, _ = fields(P, 2, seed=2)
    q_ref = F.flux(x.double(), acc, bcs == 'periodic', pab, rev)
    xin = x.to(dev).requires_grad_(True)
    q = res.flux_of(xin)
    assert tuple(q.shape) == (2, 2, P, P) and q.device.type == dev.type and not q.requires_grad
    err = (q.cpu().double() - q_ref).abs().max().item() / q_ref.abs().max().item()
    print(f"flux_of acc={acc} {bcs} P={P} rev={rev} pab={pab}: rel err {err:.2e}")
    assert err <= 2e-6
    assert torch.equal(res.flux_of(x.to(dev)), q)
    with pytest.raises(ValueError, match="does not fit"):
        res.flux_of(torch.zeros(1, 2, P, P + 1, device=dev))


def test_src_reexport_resolves():
    import importlib
    mod = importlib.import_module("src.residuals_darcy")
    assert callable(mod.ResidualsDarcy.flux_of)


# ---- 2. the one-launch kernel ---------------------------------------------------------------------------------------------------
SIZES = [(10, 3), (16, 3), (21, 2), (64, 2)]


@pytest.mark.parametrize("P,B", SIZES)
def test_flux_term_alone(backend, P, B):
    res, dev = make_res(backend, P)
    x, y, m, yq, mq, _, _ = data(P, B, "sparse")
    v_ref, s_ref = reference(P, B, "sparse", 0.0, 0.0, 1.0)
    assert (s_ref[:, 2] > 0).all() and (s_ref[:, :2] > 0).all()      # (the sums of the unweighted terms are reported too)
    check(*call(res, dev, x, y, m, yq, mq, 0.0, 0.0, 1.0), v_ref, s_ref)


@pytest.mark.parametrize("kind", ["sparse", "edges"])
@pytest.mark.parametrize("P,B", SIZES)
def test_three_terms(backend, P, B, kind):
    res, dev = make_res(backend, P)
    x, y, m, yq, mq, zp, zf = data(P, B, kind)
    pm = F.part_maxima(x, y, m, yq, mq) * torch.tensor([ZO, zp, zf], dtype=torch.float64)
    print("zeta_pde", zp, "zeta_flux", zf, "part maxima", pm.tolist())
    assert (pm > 0).all() and (pm.amax(dim=1) <= 10 * pm.amin(dim=1)).all()
    v_ref, s_ref = reference(P, B, kind, ZO, zp, zf)
    assert (s_ref > 0).all()
    check(*call(res, dev, x, y, m, yq, mq, ZO, zp, zf), v_ref, s_ref)


@pytest.mark.parametrize("P,B", SIZES)
def test_vanished_and_unweighted_flux_term(backend, P, B):
    res, dev = make_res(backend, P)
    x, y, m, yq, mq, zp, zf = data(P, B, "sparse")
    v2, s2 = R.cotangent(x, y, m, ZO, zp)
    assert (s2 > 0).all()
    # mask all zero: the term is exactly absent
    v, s = call(res, dev, x, y, m, yq, torch.zeros_like(mq), ZO, zp, zf)
    assert (s[:, 2] == 0).all()
    check(v, s[:, :2], v2, s2)
    # weight zero with data present: the sum is still reported
    v, s = call(res, dev, x, y, m, yq, mq, ZO, zp, 0.0)
    s_ref = reference(P, B, "sparse", ZO, zp, zf)[1]
    assert (s_ref[:, 2] > 0).all()
    check(v, s, v2, s_ref)


# ---- 3. beyond the LDS-resident size: the composition on the second-order tables --------------------------------------------------
def test_composition_beyond_the_lds_resident_size(backend):
    P, B = 80, 1
    res, dev = make_res(backend, P)
    assert res.specialised
    x, y, m, yq, mq, zp, zf = data(P, B, "sparse")
    v_ref, s_ref = reference(P, B, "sparse", ZO, zp, zf)
    assert (s_ref > 0).all()
    check(*call(res, dev, x, y, m, yq, mq, ZO, zp, zf), v_ref, s_ref)
    v_ref, s_ref = reference(P, B, "sparse", 0.0, 0.0, 1.0)
    check(*call(res, dev, x, y, m, yq, mq, 0.0, 0.0, 1.0), v_ref, s_ref)


# ---- 4. general stencil sets -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fd_acc,bcs", [(4, 'none'), (6, 'none'), (2, 'periodic'), (4, 'periodic')])
def test_general_path_vs_autograd(backend, fd_acc, bcs):
    P, B = 16, 3
    res, dev = make_res(backend, P, fd_acc, bcs)
    assert not res.specialised
    x, y, g = fields(P, B, seed=1)
    m = mask_of("sparse", B, P, g)
    yq, mq = flux_data(P, B, g, "sparse")
    zf = ZF_LOOP
    x, y, m, yq, mq = (a.to(dev) for a in (x, y, m, yq, mq))
    sg = res.grads.stencil_gradients
    for zo, zp, zf_ in ((ZO, ZP, zf), (0.0, 0.0, 1.0)):
        xr = x.clone().requires_grad_(True)
        r = res.residual_of(xr)
        q = torch.stack([-xr[:, 1] * sg.d_d0(xr[:, 0]), -xr[:, 1] * sg.d_d1(xr[:, 0])], dim=1)
        ls = torch.stack([(m * (xr - y) ** 2).sum(dim=(1, 2, 3)), (r ** 2).sum(dim=(1, 2)), (mq * (q - yq) ** 2).sum(dim=(1, 2, 3))], dim=1)
        assert (ls > 0).all()
        phi = zo * torch.sqrt(ls[:, 0]) + zp * torch.sqrt(ls[:, 1]) + zf_ * torch.sqrt(ls[:, 2])
        (v_ref,) = torch.autograd.grad(phi.sum(), xr)
        v, s = res.guidance_cotangent(x, y, m, zo, zp, flux_obs=yq, flux_mask=mq, zeta_flux=zf_)
        check(v.cpu(), s.cpu(), v_ref.detach().cpu().double(), ls.detach().cpu().double())
        v2, s2 = res.guidance_cotangent(x, y, m, zo, zp, flux_obs=yq, flux_mask=mq, zeta_flux=zf_)
        assert torch.equal(v, v2) and torch.equal(s, s2)
    v0, s0 = res.guidance_cotangent(x, y, m, ZO, ZP, flux_obs=yq, flux_mask=torch.zeros_like(mq), zeta_flux=zf)
    vn, sn = res.guidance_cotangent(x, y, m, ZO, ZP)
    assert (s0[:, 2] == 0).all() and torch.equal(s0[:, :2], sn) and torch.isfinite(v0).all()
    assert (v0 - vn).abs().max().item() <= 1e-6 * vn.abs().max().item()


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------
def test_flux_kernel_is_deterministic_and_batch_independent(backend):
    P = 21
    res, dev = make_res(backend, P)
    x, y, m, yq, mq, zp, zf = (a.to(dev) if torch.is_tensor(a) else a for a in data(P, 3, "sparse"))
    kw = lambda sl: dict(flux_obs=yq[sl], flux_mask=mq[sl], zeta_flux=zf)
    v1, s1 = res.guidance_cotangent(x, y, m, ZO, zp, **kw(slice(None)))
    v2, s2 = res.guidance_cotangent(x, y, m, ZO, zp, **kw(slice(None)))
    assert torch.equal(v1, v2) and torch.equal(s1, s2)
    for b in range(3):
        sl = slice(b, b + 1)
        vb, sb = res.guidance_cotangent(x[sl], y[sl], m[sl], ZO, zp, **kw(sl))
        assert torch.equal(vb[0], v1[b]) and torch.equal(sb[0], s1[b]), b


# ---- 6. calls without flux data are what they were ---------------------------------------------------------------------------------
@pytest.mark.parametrize("P,fd_acc,bcs", [(21, 2, 'none'), (16, 4, 'none'), (80, 2, 'none')])
def test_without_flux_arguments_unchanged(backend, P, fd_acc, bcs):
    L, dev = backend
    res, dev = make_res(backend, P, fd_acc, bcs)
    B = 2
    x, y, g = fields(P, B)
    m = mask_of("sparse", B, P, g)
    x, y, m = x.to(dev), y.to(dev), m.to(dev)
    v0, s0 = res.guidance_cotangent(x, y, m, ZO, ZP)
    v1, s1 = res.guidance_cotangent(x, y, m, ZO, ZP, None, flux_obs=None, flux_mask=None, zeta_flux=0.3)
    assert tuple(s0.shape) == (B, 2) and tuple(s1.shape) == (B, 2)
    assert torch.equal(v0, v1) and torch.equal(s0, s1)
    if res.specialised and P <= 71:     # the bits of the C entry itself
        vp = lambda a: C.c_void_p(a.data_ptr())
        vc, sc = torch.empty_like(x), torch.empty(B, 2, device=dev)
        L.check(L.pidm_darcy_guidance_cotangent(vp(x), vp(y), vp(m), vp(res._f_s_flat), res.inv_h0, res.inv_h1, ZO, ZP, vp(vc), vp(sc), B,
                                                P, None), "cotangent")
        assert torch.equal(vc, v0) and torch.equal(sc, s0)


# ---- 7. the loop -----------------------------------------------------------------------------------------------------------------
def _flux_loop_setup(backend):
    m, diff, res, dev, noises, obs, mask, dims = _loop_setup(backend)
    mask = torch.zeros_like(mask)
    mask[:, 1] = 1.0                                    # K fully observed, no pressure readings: the flow readings carry p
    g = torch.Generator().manual_seed(11)
    B, P = obs.shape[0], obs.shape[-1]
    yq = res.flux_of(obs.to(dev)).cpu()                 # flux of the reference field (p, K) = obs
    mq = (torch.rand(B, 2, P, P, generator=g) < 0.1).float()
    return m, diff, res, dev, noises, obs, mask, yq, mq, dims


def test_flux_guided_loop_teacher_forced(backend):
    m, diff, res, dev, noises, obs, mask, yq, mq, (dim, P, B, n_steps) = _flux_loop_setup(backend)
    assert (mq.sum(dim=(1, 2, 3)) >= 20).all()
    (x_seq, interm), aux = _run(diff, dev, noises, lambda: diff.p_sample_loop_guided(
        (B, 2, P, P), res, obs.to(dev), mask.to(dev), zeta_obs=ZO, zeta_pde=ZP, flux_obs=yq.to(dev), flux_mask=mq[:1].to(dev),
        zeta_flux=ZF_LOOP))
    mq = mq[:1].expand(B, -1, -1, -1)                   # (the mask was given in broadcastable form)
    assert len(x_seq) == n_steps + 1 and aux['guidance'].shape == (n_steps, B, 3) and aux['guidance'].device.type == dev.type
    cfg = O.UnetCfg(dim=dim, channels=2)
    p64 = R.params64(m.state_dict())
    tables = R.tables64(n_steps)
    for step, t in enumerate(reversed(range(n_steps))):
        x_ref, s_ref, g_ref = F.guided_step(p64, cfg, tables, x_seq[step], t, noises[1 + step], obs, mask, yq, mq, ZO, ZP, ZF_LOOP)
        _, _, g_two = R.guided_step(p64, cfg, tables, x_seq[step], t, noises[1 + step], obs, mask, ZO, ZP)
        err = (x_seq[1 + step].double() - x_ref).abs().max().item()
        bound = 5e-5 * max(x_ref.abs().max().item(), 1.0) + 2e-4 * g_ref.abs().max().item()
        print(f"t={t}: err {err:.3e} bound {bound:.3e} |g| {g_ref.abs().max().item():.3e} |g - g_two_term| {(g_ref - g_two).abs().max().item():.3e}")
        assert (s_ref > 0).all() and (g_ref - g_two).abs().max().item() > 10 * bound      # the flux term is there, and it matters
        assert err <= bound, f"step t={t}"
        s = aux['guidance'][step].cpu().double()
        print("sums", s.tolist(), "ref", s_ref.tolist())
        assert ((s - s_ref).abs() <= 1e-4 * s_ref.abs()).all(), f"step t={t}"


def test_flux_guided_loop_guide_below_and_replace_observed(backend):
    m, diff, res, dev, noises, obs, mask, yq, mq, (dim, P, B, n_steps) = _flux_loop_setup(backend)
    (x_seq, _), aux = _run(diff, dev, noises, lambda: diff.p_sample_loop_guided(
        (B, 2, P, P), res, obs.to(dev), mask.to(dev), zeta_obs=ZO, zeta_pde=ZP, guide_below=1, replace_observed=True, keep_history=False,
        flux_obs=yq.to(dev), flux_mask=mq.to(dev), zeta_flux=ZF_LOOP))
    assert aux['guidance'].shape == (n_steps, B, 3)
    assert (aux['guidance'][:2] == 0).all() and (aux['guidance'][2] > 0).all()
    x = x_seq[0].cpu()
    assert torch.equal(x[:, 1], obs[:, 1]) and not torch.equal(x[:, 0], obs[:, 0])     # the state's observed entries; never the flux


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------
def test_flux_errors(backend):
    L, dev = backend
    m, diff, res, dev, noises, obs, mask, yq, mq, (dim, P, B, n_steps) = _flux_loop_setup(backend)
    shape = (B, 2, P, P)
    with pytest.raises(PidmError, match="flux_obs must be"):
        diff.p_sample_loop_guided(shape, res, obs, mask, flux_obs=yq[:, :, :8], flux_mask=mq)
    with pytest.raises(PidmError, match="flux_mask must be"):
        diff.p_sample_loop_guided(shape, res, obs, mask, flux_obs=yq, flux_mask=mq[:, :1])
    with pytest.raises(PidmError, match="flux_mask must be"):
        diff.p_sample_loop_guided(shape, res, obs, mask, flux_obs=yq)
    with pytest.raises(PidmError, match="flux_obs must be"):
        diff.p_sample_loop_guided(shape, res, obs, mask, flux_mask=mq)
    with pytest.raises(PidmError, match="flux_obs must be"):
        diff.p_sample_loop_guided((3, 2, P, P), res, obs[:1], mask[:1], flux_obs=yq, flux_mask=mq)
    x = obs.to(dev)
    with pytest.raises(PidmError, match="given together"):
        res.guidance_cotangent(x, x, x, ZO, ZP, flux_obs=x)
    with pytest.raises(PidmError, match="given together"):
        res.guidance_cotangent(x, x, x, ZO, ZP, flux_mask=x)
    with pytest.raises(PidmError, match="must match"):
        res.guidance_cotangent(x, x, x, ZO, ZP, flux_obs=x[:1], flux_mask=x)
    with pytest.raises(PidmError, match=r"\[B,3\]"):
        res.guidance_cotangent(x, x, x, ZO, ZP, sums_out=torch.zeros(B, 2, device=dev), flux_obs=x, flux_mask=x)
    with pytest.raises(AssertionError):
        res.flux_of(x[:, :1])
    # the C entries: size checks come before any dereference
    vp = lambda a: C.c_void_p(a.data_ptr())
    big = torch.zeros(1, device=dev)
    x = torch.zeros(1, 2, 16, 16, device=dev)
    s = torch.zeros(1, 3, device=dev)
    f = torch.zeros(256, device=dev)
    for P_bad in (4, 72):
        assert L.pidm_darcy_guidance_cotangent_flux(vp(big), vp(big), vp(big), vp(big), vp(big), vp(big), 1.0, -1.0, 1.0, 1.0, 1.0,
                                                    vp(big), vp(s), 1, P_bad, None) != 0
        assert f"P={P_bad}".encode() in L.pidm_last_error()
    assert L.pidm_darcy_guidance_cotangent_flux(vp(x), vp(x), vp(x), vp(x), vp(x), vp(f), 1.0, -1.0, 1.0, 1.0, 1.0, vp(x), vp(s), 0, 16,
                                                None) != 0
    assert b"B>0" in L.pidm_last_error()
    assert L.pidm_darcy_guidance_cotangent_flux(vp(x), vp(x), vp(x), None, vp(x), vp(f), 1.0, -1.0, 1.0, 1.0, 1.0, vp(x), vp(s), 1, 16,
                                                None) != 0
    assert b"null" in L.pidm_last_error()
    sg = res.grads.stencil_gradients
    ops, keep = _ops_array((sg.d_d0, sg.d_d1), dev)
    for P_bad in (1, 65536):
        assert L.pidm_guidance_flux_general(vp(big), vp(big), vp(big), vp(big), vp(big), 1.0, None, vp(s), vp(big), vp(big), vp(big), 1, P_bad,
                                            None) != 0
        assert f"P={P_bad}".encode() in L.pidm_last_error()
        assert L.pidm_darcy_flux(vp(big), ops, 0, vp(big), vp(big), 1, P_bad, None) != 0
        assert f"P={P_bad}".encode() in L.pidm_last_error()
    assert L.pidm_guidance_flux_general(vp(x), vp(x), vp(x), vp(x), vp(x), 1.0, None, vp(s), vp(x), vp(x), vp(x), -1, 16, None) != 0
    assert b"B>0" in L.pidm_last_error()
    assert L.pidm_guidance_flux_general(vp(x), vp(x), None, vp(x), vp(x), 1.0, None, vp(s), vp(x), vp(x), vp(x), 1, 16, None) != 0
    assert b"null" in L.pidm_last_error()
    assert L.pidm_darcy_flux(vp(x), ops, 0, vp(x), vp(x), 0, 16, None) != 0
    assert b"B>0" in L.pidm_last_error()
    assert L.pidm_darcy_flux(vp(x), ops, 0, None, vp(x), 1, 16, None) != 0
    assert b"null" in L.pidm_last_error()
    assert L.pidm_darcy_flux(vp(x), None, 0, vp(x), vp(x), 1, 16, None) != 0
    assert b"null" in L.pidm_last_error()
    assert L.pidm_darcy_flux_ws(0, 16) == 0 and L.pidm_darcy_flux_ws(2, 16) == 2 * 2 * 256 * 4
