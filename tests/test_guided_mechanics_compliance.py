"""The compliance term of mechanics posterior guidance (mech_guidance_kernel<energy / sensitivity> of csrc/k_guidance_mech.hip,
pidm_mech_guidance_cotangent_compliance, ResidualsMechanics.guidance_cotangent(zeta_comp=, compliance_form=),
DenoisingDiffusion.p_sample_loop_guided_mechanics(zeta_comp=, compliance_form=)) against the restatement
tests/guided_mech_compliance_ref.py.  `backend` = host emulator or the gfx950 library (-m gpu).

The tolerance rule is the one of tests/test_guided_mechanics.py (inputs, masks and helpers come from there too):
err(q) = max|q - q64| / max|q64| and a kernel passes when err(kernel) <= 4 err(ref32) + 4 * 2^-23, ref32 being the restatement in
float32; two fp32 results compared with each other get twice that bound; the GPU-only cases, which have no float32 restatement, get
1e-5 relative against the composition of the existing kernels; loop steps get 5e-5 max(|x_ref|, 1) + 2e-4 max|g_ref| and their sums
1e-4 relative.  Every test prints its figures before it asserts.

The weights of a cotangent case come from the float64 restatement, never from the kernel: zeta_k = 1 / max|v_k| with v_k the
cotangent of term k alone at zeta = 1 (k = obs, pde, vol, compliance in the case's form), so each active term peaks at 1 and
max|v| <= 4; the test prints the peaks and asserts that each active one is at least a tenth of max|v|."""
import pytest
import torch
import torch.nn.functional as F

from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd._lib import PidmError, ptr, stream_ptr
from physicsinformeddiffusionmodels_amd.residuals_mechanics_K import _MechResidualFn
from tests import guided_mech_compliance_ref as RC
from tests import guided_mech_ref as R
from tests import test_guided_mechanics as G

ULP = G.ULP
FORMS = RC.FORMS
# (nel, B, warped mesh)
MESHES = [(3, 3, False), (5, 3, False), (16, 3, False), (5, 3, True)]
CASES = [(n, b, w, f, z) for n, b, w in MESHES for f in FORMS for z in ("all", "comp")] + [(64, 2, False, f, "all") for f in FORMS]
CASE_IDS = [f"nel{n}-B{b}-{'warped' if w else 'uniform'}-{f}-{z}" for n, b, w, f, z in CASES]
SUM_NAMES = ("L_obs", "L_pde", "L_vol", "C")

_REF = {}


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("guided_mech_compliance_meshes")


def check_sums(case, s, s32, s64):
    for j, name in enumerate(SUM_NAMES):
        if (s64[:, j] == 0).all():
            assert (s[:, j] == 0).all(), (case, name)
        else:
            G.check(case, name, s[:, j], s32[:, j], s64[:, j])


def reference(res, nel, B, warped, form, weights, clamp_two_columns=False):
    """inputs, the four zetas and the float64 / float32 restatement of a cotangent case, computed once"""
    key = (nel, B, warped, form, weights, clamp_two_columns)
    if key not in _REF:
        kloc, ed = G.tables(res)
        x, bcs, vf, y, g = G.make_inputs(nel, B, 3000 + nel)
        if clamp_two_columns:
            bcs[:, 0:2, :, 1] = 1.0                     # with column 0: all eight dofs of the elements of column 0 are clamped
        m = G.mask_of("sparse", B, nel + 1, g)
        peaks = []
        for j in range(4):
            zj = [1.0 if i == j else 0.0 for i in range(4)]
            peaks.append(RC.cotangent(x, bcs, vf, y, m, zj, form, kloc, ed)[0].abs().max().item())
        on = {"all": (1, 1, 1, 1), "comp": (0, 0, 0, 1)}[weights]
        zetas = [float(o) / p if p > 0 else float(o) for o, p in zip(on, peaks)]
        ref = {dt: RC.cotangent(x, bcs, vf, y, m, zetas, form, kloc, ed, dtype=dt) for dt in (torch.float64, torch.float32)}
        vmax = ref[torch.float64][0].abs().max().item()
        active = [z * p for z, p in zip(zetas, peaks)]
        print(f"GUIDED_MECH_C nel={nel} {form} {weights}: term peaks at zeta=1 {peaks}, zetas {zetas}, scaled peaks {active}, max|v| {vmax}")
        assert peaks[3] > 0
        for a, z, p in zip(active, zetas, peaks):
            if z != 0 and p > 0:
                assert a >= 0.1 * vmax, (active, vmax)
        _REF[key] = (x, bcs, vf, y, m, zetas, ref)
    return _REF[key]


def call(res, dev, x, bcs, vf, y, m, zetas, form, **kw):
    return res.guidance_cotangent(x.to(dev), bcs.to(dev), vf.to(dev), y.to(dev), m.to(dev), *zetas[:3], zeta_comp=zetas[3],
                                  compliance_form=form, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# the one-launch cotangent with the compliance term
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nel,B,warped,form,weights", CASES, ids=CASE_IDS)
def test_compliance_cotangent_vs_float64(backend, mesh_dir, nel, B, warped, form, weights):
    L, dev = backend
    res = G.get_res(backend, mesh_dir, nel, warped)
    x, bcs, vf, y, m, zetas, ref = reference(res, nel, B, warped, form, weights)
    (v64, mo64, s64), (v32, mo32, s32) = ref[torch.float64], ref[torch.float32]
    case = f"nel={nel} {'warped' if warped else 'uniform'} {form} {weights}"
    s = torch.full((B, 4), float('nan'), device=dev)
    v, mo, s_ret = call(res, dev, x, bcs, vf, y, m, zetas, form, sums_out=s)
    assert s_ret is s and v.shape == x.shape and mo.shape == y.shape
    assert torch.isfinite(v).all() and torch.isfinite(s).all() and torch.isfinite(mo).all()
    G.check(case, "model_out", mo, mo32, mo64)
    check_sums(case, s.cpu(), s32, s64)
    assert (s64[:, 1] > 0).all() and (s64[:, 2] > 0).all() and (s64[:, 3] != 0).all()
    G.check(case, "v", v, v32, v64)
    if form == "sensitivity" and weights == "comp":
        assert (v[:, :2] == 0).all() and (v64[:, :2] == 0).all()    # the displacement channels gain nothing


@pytest.mark.parametrize("nel,B,warped", [(16, 3, False), (5, 3, True)])
@pytest.mark.parametrize("form", FORMS)
def test_zero_compliance_weight_is_the_existing_call(backend, mesh_dir, form, nel, B, warped):
    L, dev = backend
    res = G.get_res(backend, mesh_dir, nel, warped)
    x, bcs, vf, y, m, zetas, ref = reference(res, nel, B, warped, form, "all")
    (_, _, s64), (_, _, s32) = ref[torch.float64], ref[torch.float32]
    v0, mo0, s0 = res.guidance_cotangent(x.to(dev), bcs.to(dev), vf.to(dev), y.to(dev), m.to(dev), *zetas[:3])
    v, mo, s = call(res, dev, x, bcs, vf, y, m, zetas[:3] + [0.0], form)
    assert s0.shape == (B, 3) and s.shape == (B, 4)
    print(f"GUIDED_MECH_C zero weight nel={nel} {form}: max|v - v0| {(v - v0).abs().max().item():.3e}, C {s[:, 3].tolist()}")
    assert torch.equal(v, v0) and torch.equal(mo, mo0) and torch.equal(s[:, :3], s0)
    assert (s[:, 3] != 0).all()
    G.check(f"zero weight nel={nel} {form}", "C", s[:, 3].cpu(), s32[:, 3], s64[:, 3])


@pytest.mark.parametrize("form", FORMS)
def test_fully_clamped_element(backend, mesh_dir, form):
    """Columns 0 and 1 of nodes clamped in x and y: the elements of column 0 have no free dof.  'sensitivity': their compliance
    contribution to v_rho is exactly zero.  'energy': the clamped dofs' 2 zeta U_i reaches v through the resize adjoint."""
    L, dev = backend
    nel, B = 5, 3
    res = G.get_res(backend, mesh_dir, nel)
    x, bcs, vf, y, m, zetas, ref = reference(res, nel, B, False, form, "comp", clamp_two_columns=True)
    assert (bcs[:, 0:2, :, :2] != 0).all()
    (v64, mo64, s64), (v32, mo32, s32) = ref[torch.float64], ref[torch.float32]
    case = f"clamped element {form}"
    v, mo, s = call(res, dev, x, bcs, vf, y, m, zetas, form)
    G.check(case, "v", v, v32, v64)
    check_sums(case, s.cpu(), s32, s64)
    print(f"GUIDED_MECH_C {case}: restatement v_rho column 0 {v64[:, 2, :, 0].abs().max().item():.3e}, elsewhere "
          f"{v64[:, 2, :, 1:].abs().min().item():.3e}; v_u column 0 {v64[:, :2, :, 0].abs().min().item():.3e}")
    if form == "sensitivity":
        assert (v64[:, 2, :, 0] == 0).all() and (v.cpu()[:, 2, :, 0] == 0).all()
        assert (v64[:, 2, :, 1:] != 0).all() and (v.cpu()[:, 2, :, 1:] != 0).all()
    else:
        # with every dof of these elements clamped, d C / d rho_e = 0 there as well, and what the displacement pixels of column 0
        # receive is the identity rows' 2 zeta U_i (plus the K^T of free neighbours)
        assert (v64[:, 2, :, 0] == 0).all() and (v64[:, :2, :, 0] != 0).all()


def composition4(res, x, bcs, vf, y, m, zetas, form):
    """Phi4 from the outputs of the existing residual kernel pair (the third one is C), gradient by torch autograd on the device"""
    xr = x.clone().requires_grad_(True)
    r, mo, comp, shift = _MechResidualFn.apply(xr, bcs, vf, res.stiffs, res.lib)
    l_obs = (R.state_mask(m) * (mo - y) ** 2).sum(dim=(1, 2, 3))
    l_pde = (r ** 2).sum(dim=1)
    l_vol = shift ** 2
    phi3 = sum(z * R._sqrt_or_omit(l) for z, l in zip(zetas[:3], (l_obs, l_pde, l_vol)))
    sums = torch.stack([l_obs, l_pde, l_vol, comp], dim=1).detach()
    if form == "energy":
        (v,) = torch.autograd.grad((phi3 + zetas[3] * comp).sum(), xr)
        return v.detach(), mo.detach(), sums
    (v3,) = torch.autograd.grad(phi3.sum(), xr, retain_graph=True)
    (dc,) = torch.autograd.grad(comp.sum(), xr)
    v = v3.detach().clone()
    v[:, 2] -= zetas[3] * dc[:, 2]
    return v, mo.detach(), sums


@pytest.mark.parametrize("nel,B,warped", [(5, 3, True), (16, 3, False)])
@pytest.mark.parametrize("form", FORMS)
def test_compliance_cotangent_vs_composition_of_existing_kernels(backend, mesh_dir, form, nel, B, warped):
    L, dev = backend
    res = G.get_res(backend, mesh_dir, nel, warped)
    x, bcs, vf, y, m, zetas, ref = reference(res, nel, B, warped, form, "all")
    (v64, mo64, s64), (v32, mo32, s32) = ref[torch.float64], ref[torch.float32]
    case = f"composition nel={nel} {form}"
    xd, bd, vd, yd, md = (a.to(dev) for a in (x, bcs, vf, y, m))
    vc, moc, sc = composition4(res, xd, bd, vd, yd, md, zetas, form)
    v, mo, s = call(res, dev, x, bcs, vf, y, m, zetas, form)
    G.check(case, "v (composition)", vc, v32, v64)
    check_sums(case + " (composition)", sc.cpu(), s32, s64)
    G.check(case, "v (one launch)", v, v32, v64)
    check_sums(case + " (one launch)", s.cpu(), s32, s64)
    e = G.err(v, vc)
    bound = 2 * (4 * G.err(v32, v64) + 4 * ULP)
    print(f"GUIDED_MECH_C {case}: one launch vs composition {e:.3e} bound {bound:.3e}")
    assert e <= bound
    assert torch.equal(mo, moc)


@pytest.mark.parametrize("form", FORMS)
def test_compliance_cotangent_is_deterministic_and_batch_independent(backend, mesh_dir, form):
    nel, B = 16, 3
    L, dev = backend
    res = G.get_res(backend, mesh_dir, nel)
    x, bcs, vf, y, m, zetas, _ = reference(res, nel, B, False, form, "all")
    v1, mo1, s1 = call(res, dev, x, bcs, vf, y, m, zetas, form)
    v2, mo2, s2 = call(res, dev, x, bcs, vf, y, m, zetas, form)
    assert torch.equal(v1, v2) and torch.equal(s1, s2) and torch.equal(mo1, mo2)
    for b in range(B):
        sl = slice(b, b + 1)
        vb, mob, sb = call(res, dev, x[sl], bcs[sl], vf[sl], y[sl], m[sl], zetas, form)
        print(f"GUIDED_MECH_C batch independence {form} b={b}: max|dv| {(vb[0] - v1[b]).abs().max().item():.3e}")
        assert torch.equal(vb[0], v1[b]) and torch.equal(sb[0], s1[b]) and torch.equal(mob[0], mo1[b]), b


# ------------------------------------------------------------------------------------------------------------------------------
# guards
# ------------------------------------------------------------------------------------------------------------------------------
def test_native_guards_of_the_compliance_entry(backend, mesh_dir):
    L, dev = backend
    nel = 3
    res = G.get_res(backend, mesh_dir, nel)
    st = res.stiffs
    x, bcs, vf, y, g = G.make_inputs(nel, 1, 5)
    m = G.mask_of("sparse", 1, nel + 1, g)
    x, bcs, vf, y, m = (a.to(dev) for a in (x, bcs, vf, y, m))
    v, mo, s = torch.empty_like(x), torch.empty_like(y), torch.empty(1, 4, device=dev)
    mesh = [ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), ptr(st.dof_elems32), nel]

    def cot(bufs=None, mesh_=None, outs=None, B=1, form=0):
        bufs = bufs or [ptr(x), ptr(bcs), ptr(vf), ptr(y), ptr(m)]
        return L.pidm_mech_guidance_cotangent_compliance(*bufs, 1.0, 1.0, 1.0, 1.0, form, *(mesh_ or mesh),
                                                         *(outs or [ptr(v), ptr(mo), ptr(s)]), B, None)

    before = G.launches(L)
    for k in range(5):
        bufs = [ptr(x), ptr(bcs), ptr(vf), ptr(y), ptr(m)]
        bufs[k] = None
        assert cot(bufs=bufs) != 0 and b"null buffer" in L.pidm_last_error(), k
    for k in range(3):
        outs = [ptr(v), ptr(mo), ptr(s)]
        outs[k] = None
        assert cot(outs=outs) != 0 and b"null buffer" in L.pidm_last_error(), k
    assert cot(B=0) != 0 and b"B must be positive" in L.pidm_last_error()
    assert cot(B=-3) != 0 and b"B must be positive" in L.pidm_last_error()
    assert cot(mesh_=[None] + mesh[1:]) != 0 and b"null mesh table" in L.pidm_last_error()
    assert cot(mesh_=mesh[:2] + [None] + mesh[3:]) != 0 and b"null mesh table" in L.pidm_last_error()
    assert cot(mesh_=mesh[:3] + [None, nel]) != 0 and b"null mesh table" in L.pidm_last_error()
    assert cot(mesh_=mesh[:1] + [8] + mesh[2:]) != 0 and b"kloc_stride" in L.pidm_last_error()
    assert cot(mesh_=mesh[:4] + [80]) != 0 and b"LDS" in L.pidm_last_error()       # (the size check comes before any access)
    assert cot(mesh_=mesh[:4] + [0]) != 0 and b"nel" in L.pidm_last_error()
    for bad in (2, -1):
        assert cot(form=bad) != 0 and b"comp_form" in L.pidm_last_error(), bad
    print(f"GUIDED_MECH_C guards: launches before {before}, after the refusals {G.launches(L)}")
    assert G.launches(L) == before                                  # nothing was launched
    assert cot() == 0
    assert G.launches(L) == before + 1
    assert cot(form=1) == 0
    assert G.launches(L) == before + 2


def test_python_level_errors_of_the_compliance_arguments(backend, mesh_dir):
    L, dev = backend
    nel, B = 5, 2
    res = G.get_res(backend, mesh_dir, nel)
    x, bcs, vf, y, g = G.make_inputs(nel, B, 9)
    m = G.mask_of("sparse", B, nel + 1, g)
    x, bcs, vf, y, m = (a.to(dev) for a in (x, bcs, vf, y, m))
    with pytest.raises(PidmError, match="compliance_form"):
        res.guidance_cotangent(x, bcs, vf, y, m, 1.0, 1.0, zeta_comp=1.0, compliance_form="adjoint")
    with pytest.raises(PidmError, match=r"sums_out.*\[B,4\]"):
        res.guidance_cotangent(x, bcs, vf, y, m, 1.0, 1.0, zeta_comp=1.0, sums_out=torch.empty(B, 3, device=dev))
    with pytest.raises(PidmError, match=r"sums_out.*\[B,3\]"):
        res.guidance_cotangent(x, bcs, vf, y, m, 1.0, 1.0, sums_out=torch.empty(B, 4, device=dev))
    v, mo, s = res.guidance_cotangent(x, bcs, vf, y, m, 1.0, 1.0, zeta_comp=0.5, compliance_form="sensitivity")
    assert s.shape == (B, 4)


# ------------------------------------------------------------------------------------------------------------------------------
# the sampler loop
# ------------------------------------------------------------------------------------------------------------------------------
ZETAS4 = (1.0, 1.0, 1.0, 1.0)


def _guided(diff, dev, noises, cond, bcs, shape, res, obs, mask, zeta_comp, form):
    return G._run(dev, noises, lambda: diff.p_sample_loop_guided_mechanics(
        (cond.to(dev), bcs.to(dev)), shape, res, obs.to(dev), mask.to(dev), *ZETAS4[:3], zeta_comp=zeta_comp, compliance_form=form))


@pytest.mark.parametrize("form", FORMS)
def test_guided_loop_with_compliance_teacher_forced(backend, mesh_dir, form):
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, n_steps) = G._loop_setup(backend, mesh_dir)
    nn = nel + 1
    shape = (B, 3, nn, nn)
    (x_seq, interm), aux = _guided(diff, dev, noises, cond, bcs, shape, res, obs, mask, ZETAS4[3], form)
    assert len(x_seq) == n_steps + 1 and len(interm) == n_steps + 1
    assert aux['guidance'].shape == (n_steps, B, 4) and aux['guidance'].device.type == dev.type
    cfg = O.UnetCfg(dim=dim, channels=10, out_dim=3, sigmoid_last_channel=True)
    p64 = R.params64(m.state_dict())
    tables64 = R.tables64(n_steps)
    kloc, ed = G.tables(res)
    assert torch.equal(x_seq[0], noises[0])
    for step, t in enumerate(reversed(range(n_steps))):
        # teacher forcing: the restatement advances the engine's own previous state
        x_ref, s_ref, g_ref = RC.guided_step(p64, cfg, tables64, x_seq[step], cond, bcs, t, noises[1 + step], obs, mask, ZETAS4, form,
                                             kloc, ed)
        err_ = (x_seq[1 + step].double() - x_ref).abs().max().item()
        bound = 5e-5 * max(x_ref.abs().max().item(), 1.0) + 2e-4 * g_ref.abs().max().item()
        print(f"{form} t={t}: err {err_:.3e} bound {bound:.3e} |g| {g_ref.abs().max().item():.3e} |x| {x_ref.abs().max().item():.3e}")
        s = aux['guidance'][step].cpu().double()
        print("sums", s.tolist(), "ref", s_ref.tolist())
        assert g_ref.abs().max().item() > 0
        assert err_ <= bound, f"step t={t}"
        assert ((s - s_ref).abs() <= 1e-4 * s_ref.abs()).all(), f"step t={t}"
    # zeta_comp = 0.0 walks the states of zeta_comp = None and reports the same first three sums
    (x_none, _), aux_none = G._run(dev, noises, lambda: diff.p_sample_loop_guided_mechanics(
        (cond.to(dev), bcs.to(dev)), shape, res, obs.to(dev), mask.to(dev), *ZETAS4[:3]))
    (x_zero, _), aux_zero = _guided(diff, dev, noises, cond, bcs, shape, res, obs, mask, 0.0, form)
    assert aux_none['guidance'].shape == (n_steps, B, 3) and aux_zero['guidance'].shape == (n_steps, B, 4)
    for a, b in zip(x_zero, x_none):
        assert torch.equal(a, b)
    assert torch.equal(aux_zero['guidance'][..., :3], aux_none['guidance'])
    assert (aux_zero['guidance'][..., 3] != 0).all()
    assert not torch.equal(x_seq[-1], x_none[-1])                   # ... and a weight of 1.0 does not


def test_guided_loop_rejects_an_unknown_compliance_form(backend, mesh_dir):
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, n_steps) = G._loop_setup(backend, mesh_dir)
    with pytest.raises(PidmError, match="compliance_form"):
        diff.p_sample_loop_guided_mechanics((cond.to(dev), bcs.to(dev)), (B, 3, nel + 1, nel + 1), res, obs, mask, zeta_comp=1.0,
                                            compliance_form="adjoint")


# ------------------------------------------------------------------------------------------------------------------------------
# GPU only: the benchmark's mesh
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_compliance_cotangent_nel64_b32_vs_composition_gpu(mesh_dir, form):
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    backend = (get_lib(), torch.device("cuda:0"))
    dev = backend[1]
    nel, B = 64, 32
    res = G.get_res(backend, mesh_dir, nel)
    x, bcs, vf, y, g = G.make_inputs(nel, B, 64032)
    m = G.mask_of("sparse", B, nel + 1, g)
    _, _, _, _, _, zetas, _ = reference(res, nel, 2, False, form, "all")          # the weights of the nel = 64 case above
    xd, bd, vd, yd, md = (a.to(dev) for a in (x, bcs, vf, y, m))
    vc, moc, sc = composition4(res, xd, bd, vd, yd, md, zetas, form)
    v, mo, s = call(res, dev, x, bcs, vf, y, m, zetas, form)
    assert torch.isfinite(v).all() and (s[:, :3] > 0).all() and (s[:, 3] != 0).all()
    G.check_rel(f"{form} v", v, vc)
    for j, name in enumerate(SUM_NAMES):
        G.check_rel(f"{form} {name}", s[:, j], sc[:, j])
    assert torch.equal(mo, moc)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_two_guided_steps_with_compliance_dim32_nel64_gpu(mesh_dir, form):
    """Two guided steps at the benchmark's mesh against the same steps assembled on the device as in
    tests/test_guided_mechanics.py::test_two_guided_steps_dim32_nel64_gpu, with the four-term composition."""
    from physicsinformeddiffusionmodels_amd._engine import input_gradient_pass
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    backend = (get_lib(), torch.device("cuda:0"))
    n_steps = 2
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, _) = G._loop_setup(backend, mesh_dir, n_steps=n_steps, dim=32, nel=64)
    nn = nel + 1
    L = backend[0]
    (x_seq, _), aux = _guided(diff, dev, noises, cond, bcs, (B, 3, nn, nn), res, obs, mask, ZETAS4[3], form)
    assert aux['guidance'].shape == (n_steps, B, 4)
    cd, bd, od, md = (a.to(dev) for a in (cond, bcs, obs, mask))
    vf = cd[:, 0, 0, 0].contiguous()
    ht = diff._host_tables
    rs = lambda a: F.interpolate(a, size=(nel, nel), mode="bilinear", align_corners=False)
    for step, t in enumerate(reversed(range(n_steps))):
        xt = x_seq[step].to(dev)
        xr = xt.clone().requires_grad_(True)
        net_in = torch.cat((rs(xr), rs(cd), rs(bd)), dim=1)
        with torch.no_grad():
            x0p, pull = input_gradient_pass(m, net_in.detach(), torch.full((B,), t, device=dev, dtype=torch.long))
            x0p = x0p.clone()
        v, mo, sums = composition4(res, x0p, bd, vf, od, md, ZETAS4, form)
        with torch.no_grad():
            g_in = pull(v).reshape(B, nel, nel, 10).permute(0, 3, 1, 2)
        (g,) = torch.autograd.grad((net_in * g_in).sum(), xr)
        c1, c2 = float(ht['posterior_mean_coef1'][t]), float(ht['posterior_mean_coef2'][t])
        sigma = 0.0 if t == 0 else float(ht['betas'][t].sqrt())
        plain = torch.empty_like(xt)
        z = noises[1 + step].to(dev)
        L.check(L.pidm_psample_update(ptr(mo.contiguous()), ptr(xt), ptr(z), c1, c2, sigma, ptr(plain), xt.numel(), stream_ptr(dev)),
                "pidm_psample_update")
        x_ref = plain - g
        e = (x_seq[1 + step].to(dev) - x_ref).abs().max().item()
        bound = 1e-5 * x_ref.abs().max().item()
        print(f"GUIDED_MECH_C gpu {form} t={t}: err {e:.3e} bound {bound:.3e} |g| {g.abs().max().item():.3e}")
        assert g.abs().max().item() > 0
        assert e <= bound
        for j in range(4):
            G.check_rel(f"{form} t={t} sums[{j}]", aux['guidance'][step][:, j], sums[:, j])
