"""Posterior guidance of the mechanics sampler (csrc/k_guidance_mech.hip, ResidualsMechanics.guidance_cotangent,
DenoisingDiffusion.p_sample_loop_guided_mechanics) against the restatement tests/guided_mech_ref.py.  `backend` = host emulator or
the gfx950 library (-m gpu).

Tolerance rule of the kernel tests (tests/test_kernels_mech_f64.py): err(q) = max|q - q64| / max|q64| and a kernel passes when
err(kernel) <= 4 err(ref32) + 4 * 2^-23, ref32 being the restatement evaluated in float32 by torch on the CPU inside the test.  Where
two fp32 results are compared with each other (one launch against the composition of the existing forward / adjoint kernels) each
carries that bound against float64, so their distance is held to twice it.  Where no float32 restatement exists (the GPU-only
cases) the bound is 1e-5 relative, as check_cotangent of tests/test_guided_sampling.py.  Every test prints its figures before it
asserts.

The weights of a cotangent case are derived from the float64 restatement, never from the kernel: zeta_k = 1 / max|v_k| with v_k the
cotangent of term k alone at zeta = 1, so each active term peaks at 1 and max|v| <= 3; the test prints the peaks and asserts that
each is at least a tenth of max|v|.

The loop tests keep the bounds of the Darcy loop test: per step err <= 5e-5 max(|x_ref|, 1) + 2e-4 max|g_ref|, sums to 1e-4
relative."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pidm_oracle as O
from physicsinformeddiffusionmodels_amd._engine import get_engine
from physicsinformeddiffusionmodels_amd._lib import PidmError, ptr, stream_ptr
from physicsinformeddiffusionmodels_amd.denoising_utils import DenoisingDiffusion
from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
from physicsinformeddiffusionmodels_amd.residuals_mechanics_K import ResidualsMechanics, _MechResidualFn
from physicsinformeddiffusionmodels_amd.unet_model import Unet3D
from tests import guided_mech_ref as R
from tests import mech_ref as MR
from tests.test_training_step import patched_rng

ULP = 2.0 ** -23
# (nel, B, warped mesh)
MESHES = [(3, 3, False), (5, 3, False), (16, 3, False), (5, 3, True)]
MASKS = ["rho", "sparse", "none", "disp"]
WEIGHTS = ["all", "obs", "pde", "vol", "zero"]
CASES = ([(n, b, w, k, "all") for n, b, w in MESHES for k in MASKS] +
         [(n, b, w, "sparse", z) for n, b, w in MESHES for z in WEIGHTS[1:]] + [(64, 2, False, "sparse", "all")])
CASE_IDS = [f"nel{n}-B{b}-{'warped' if w else 'uniform'}-{k}-{z}" for n, b, w, k, z in CASES]

_RES, _REF = {}, {}


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("guided_mech_meshes")


def get_res(backend, mesh_dir, nel, warped=False, model=None):
    L, dev = backend
    key = (nel, warped, dev.type)
    if model is not None or key not in _RES:
        folder = MR.warped_mesh(mesh_dir / f"warped{nel}", nel, seed=100 + nel) if warped else "/nonexistent/"
        res = ResidualsMechanics(model=model, pixels_per_dim=nel, pixels_at_boundary=True, no_BC_folder=folder, device=dev,
                                 lib=L if dev.type == "cpu" else None)
        assert res.stiffs.kloc_stride == (64 if warped else 0)
        if model is not None:
            return res
        _RES[key] = res
    return _RES[key]


def tables(res):
    """(kloc, elem_dofs) of the restatement: the fp32 values the kernels read; [8,8] on a uniform mesh (the oracle's functions)"""
    k = res.stiffs.tot_local_stiffness.cpu()
    return (k[0] if res.stiffs.kloc_stride == 0 else k), res.stiffs.elem_dofs32.cpu().numpy()


def make_inputs(nel, B, seed):
    """x0 estimate (u ~ N(0,1), rho ~ U(0,1)); column 0 clamped (mask values 1.0 and -2.0), one more node clamped in x only;
    loads 0.1 N(0,1) on two columns of nodes (one of them the clamped column: a Dirichlet dof carries no load); observations of
    the same kind as the estimate"""
    g = torch.Generator().manual_seed(seed)
    nn = nel + 1
    x = torch.randn(B, 3, nel, nel, generator=g)
    x[:, 2] = torch.rand(B, nel, nel, generator=g)
    bcs = torch.zeros(B, 4, nn, nn)
    bcs[:, 0, :, 0] = 1.0
    bcs[:, 1, :, 0] = -2.0
    bcs[:, 0, nn // 2, nn - 1] = 1.0
    load = 0.1 * torch.randn(B, 2, nn, nn, generator=g)
    bcs[:, 2:4, :, 0] = load[:, :, :, 0]
    bcs[:, 2:4, :, nn - 1] = load[:, :, :, nn - 1]
    vf = 0.1 + 0.1 * torch.rand(B, generator=g)
    y = torch.randn(B, 3, nn, nn, generator=g)
    y[:, 2] = torch.rand(B, nn, nn, generator=g)
    return x, bcs, vf, y, g


def mask_of(kind, B, nn, g):
    m = torch.zeros(B, 3, nn, nn)
    if kind == "rho":
        m[:, 2] = 1.0                       # the padding row / column included: the kernel has to ignore it
    elif kind == "disp":
        m[:, :2] = 1.0
    elif kind == "sparse":
        m = (torch.rand(B, 3, nn, nn, generator=g) < 0.1).float()
    else:
        assert kind == "none"
    return m


def err(q, q64):
    q = np.asarray(q.detach().cpu(), dtype=np.float64)
    q64 = np.asarray(q64.detach().cpu(), dtype=np.float64)
    assert q.shape == q64.shape, (q.shape, q64.shape)
    return float(np.abs(q - q64).max() / max(np.abs(q64).max(), 1e-300))


def check(case, name, got, ref32, ref64):
    ek, er = err(got, ref64), err(ref32, ref64)
    print(f"GUIDED_MECH {case} {name}: err(kernel) {ek:.3e} err(ref32) {er:.3e}")
    assert ek <= 4 * er + 4 * ULP, (case, name, ek, er)


def check_sums(case, s, s32, s64):
    for j, name in enumerate(("L_obs", "L_pde", "L_vol")):
        if (s64[:, j] == 0).all():
            assert (s[:, j] == 0).all(), (case, name)
        else:
            check(case, name, s[:, j], s32[:, j], s64[:, j])


def reference(res, nel, B, warped, kind, weights):
    """inputs, zetas and the float64 / float32 restatement of a cotangent case, computed once"""
    key = (nel, B, warped, kind, weights)
    if key not in _REF:
        kloc, ed = tables(res)
        x, bcs, vf, y, g = make_inputs(nel, B, 3000 + nel)
        m = mask_of(kind, B, nel + 1, g)
        peaks = []
        for j in range(3):
            zj = [1.0 if i == j else 0.0 for i in range(3)]
            peaks.append(R.cotangent(x, bcs, vf, y, m, zj, kloc, ed)[0].abs().max().item())
        on = {"all": (1, 1, 1), "obs": (1, 0, 0), "pde": (0, 1, 0), "vol": (0, 0, 1), "zero": (0, 0, 0)}[weights]
        zetas = [float(o) / p if p > 0 else float(o) for o, p in zip(on, peaks)]
        ref = {dt: R.cotangent(x, bcs, vf, y, m, zetas, kloc, ed, dtype=dt) for dt in (torch.float64, torch.float32)}
        vmax = ref[torch.float64][0].abs().max().item()
        active = [z * p for z, p in zip(zetas, peaks)]
        print(f"GUIDED_MECH nel={nel} {kind} {weights}: term peaks at zeta=1 {peaks}, zetas {zetas}, scaled peaks {active}, max|v| {vmax}")
        for a, z, p in zip(active, zetas, peaks):
            if z != 0 and p > 0:
                assert a >= 0.1 * vmax, (active, vmax)
        _REF[key] = (x, bcs, vf, y, m, zetas, ref)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------------------
# the one-launch cotangent kernel
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nel,B,warped,kind,weights", CASES, ids=CASE_IDS)
def test_cotangent_kernel_vs_float64(backend, mesh_dir, nel, B, warped, kind, weights):
    L, dev = backend
    res = get_res(backend, mesh_dir, nel, warped)
    x, bcs, vf, y, m, zetas, ref = reference(res, nel, B, warped, kind, weights)
    (v64, mo64, s64), (v32, mo32, s32) = ref[torch.float64], ref[torch.float32]
    case = f"nel={nel} {'warped' if warped else 'uniform'} {kind} {weights}"
    s = torch.full((B, 3), float('nan'), device=dev)
    v, mo, s_ret = res.guidance_cotangent(x.to(dev), bcs.to(dev), vf.to(dev), y.to(dev), m.to(dev), *zetas, sums_out=s)
    assert s_ret is s and v.shape == x.shape and mo.shape == y.shape
    assert torch.isfinite(v).all() and torch.isfinite(s).all() and torch.isfinite(mo).all()
    check(case, "model_out", mo, mo32, mo64)
    check_sums(case, s.cpu(), s32, s64)
    assert (s64[:, 1] > 0).all() and (s64[:, 2] > 0).all()           # the sums are written whatever the weights are
    if kind == "none":
        assert (s[:, 0] == 0).all()
    if weights == "zero":
        assert (v == 0).all()
    else:
        check(case, "v", v, v32, v64)


def test_padding_of_channel_2_is_ignored(backend, mesh_dir):
    nel, B = 5, 3
    L, dev = backend
    res = get_res(backend, mesh_dir, nel)
    x, bcs, vf, y, m, zetas, _ = reference(res, nel, B, False, "rho", "all")
    args = lambda y_, m_: (x.to(dev), bcs.to(dev), vf.to(dev), y_.to(dev), m_.to(dev), *zetas)
    v, mo, s = res.guidance_cotangent(*args(y, m))
    y2, m2 = y.clone(), m.clone()
    y2[:, 2, nel, :] += 3.0
    y2[:, 2, :, nel] -= 7.0
    m2[:, 2, nel, :] = 0.0
    m2[:, 2, :, nel] = 5.0
    v2, mo2, s2 = res.guidance_cotangent(*args(y2, m2))
    assert torch.equal(v, v2) and torch.equal(s, s2) and torch.equal(mo, mo2)
    assert (mo[:, 2, nel, :] == 0).all() and (mo[:, 2, :, nel] == 0).all()


def test_exact_zeros_are_omitted(backend, mesh_dir):
    nel, B = 5, 3
    L, dev = backend
    res = get_res(backend, mesh_dir, nel)
    x, bcs, vf, y, g = make_inputs(nel, B, 77)
    m = torch.zeros(B, 3, nel + 1, nel + 1)
    v, _, s = res.guidance_cotangent(x.to(dev), bcs.to(dev), vf.to(dev), y.to(dev), m.to(dev), 1.0, 1.0, 1.0)
    assert (s[:, 0] == 0).all() and torch.isfinite(v).all() and (s[:, 1:] > 0).all()
    # a constant density 0.375 (exact in fp32, and so is its mean) with vf = 0.375: the volume term is exactly zero
    x[:, 2] = 0.375
    vf = torch.full((B,), 0.375)
    m = mask_of("sparse", B, nel + 1, g)
    v, _, s = res.guidance_cotangent(x.to(dev), bcs.to(dev), vf.to(dev), y.to(dev), m.to(dev), 1.0, 1.0, 1.0)
    assert (s[:, 2] == 0).all() and torch.isfinite(v).all() and torch.isfinite(s).all() and (s[:, :2] > 0).all()
    # ... and with the other two weights off and nothing observed v is exactly zero
    v, _, s = res.guidance_cotangent(x.to(dev), bcs.to(dev), vf.to(dev), y.to(dev), torch.zeros_like(m).to(dev), 1.0, 0.0, 1.0)
    assert (v == 0).all() and (s[:, 1] > 0).all()


def test_cotangent_kernel_is_deterministic_and_batch_independent(backend, mesh_dir):
    nel, B = 16, 3
    L, dev = backend
    res = get_res(backend, mesh_dir, nel)
    x, bcs, vf, y, m, zetas, _ = reference(res, nel, B, False, "sparse", "all")
    x, bcs, vf, y, m = (a.to(dev) for a in (x, bcs, vf, y, m))
    v1, mo1, s1 = res.guidance_cotangent(x, bcs, vf, y, m, *zetas)
    v2, mo2, s2 = res.guidance_cotangent(x, bcs, vf, y, m, *zetas)
    assert torch.equal(v1, v2) and torch.equal(s1, s2) and torch.equal(mo1, mo2)
    for b in range(B):
        sl = slice(b, b + 1)
        vb, mob, sb = res.guidance_cotangent(x[sl], bcs[sl], vf[sl], y[sl], m[sl], *zetas)
        assert torch.equal(vb[0], v1[b]) and torch.equal(sb[0], s1[b]) and torch.equal(mob[0], mo1[b]), b


def composition(res, x, bcs, vf, y, m, zetas):
    """Phi from the outputs of the existing residual kernel pair, its gradient by torch autograd on the inputs' device"""
    xr = x.clone().requires_grad_(True)
    r, mo, _, shift = _MechResidualFn.apply(xr, bcs, vf, res.stiffs, res.lib)
    l_obs = (R.state_mask(m) * (mo - y) ** 2).sum(dim=(1, 2, 3))
    l_pde = (r ** 2).sum(dim=1)
    l_vol = shift ** 2
    phi = sum(z * R._sqrt_or_omit(l) for z, l in zip(zetas, (l_obs, l_pde, l_vol)))
    (v,) = torch.autograd.grad(phi.sum(), xr)
    return v.detach(), mo.detach(), torch.stack([l_obs, l_pde, l_vol], dim=1).detach()


@pytest.mark.parametrize("nel,B,warped", [(5, 3, True), (16, 3, False)])
def test_cotangent_kernel_vs_composition_of_existing_kernels(backend, mesh_dir, nel, B, warped):
    L, dev = backend
    res = get_res(backend, mesh_dir, nel, warped)
    x, bcs, vf, y, m, zetas, ref = reference(res, nel, B, warped, "sparse", "all")
    (v64, mo64, s64), (v32, mo32, s32) = ref[torch.float64], ref[torch.float32]
    case = f"composition nel={nel}"
    xd, bd, vd, yd, md = (a.to(dev) for a in (x, bcs, vf, y, m))
    vc, moc, sc = composition(res, xd, bd, vd, yd, md, zetas)
    v, mo, s = res.guidance_cotangent(xd, bd, vd, yd, md, *zetas)
    check(case, "v (composition)", vc, v32, v64)
    check_sums(case + " (composition)", sc.cpu(), s32, s64)
    check(case, "v (one launch)", v, v32, v64)
    check_sums(case + " (one launch)", s.cpu(), s32, s64)
    # one launch against the composition, both fp32: each is within the rule of float64, so twice the rule between them
    e = err(v, vc)
    bound = 2 * (4 * err(v32, v64) + 4 * ULP)
    print(f"GUIDED_MECH {case}: one launch vs composition {e:.3e} bound {bound:.3e}")
    assert e <= bound
    assert torch.equal(mo, moc)                                     # same arithmetic as mech_kernel<false>


# ------------------------------------------------------------------------------------------------------------------------------
# the guided update through the resize adjoint
# ------------------------------------------------------------------------------------------------------------------------------
def update_ref(x0, xt, z, g, c1, c2, sg, C_, Hi, dt):
    x0, xt, z, g = (a.to(dt) for a in (x0, xt, z, g))
    B = x0.shape[0]
    g_img = g[..., :C_].reshape(B, Hi, Hi, C_).permute(0, 3, 1, 2)
    xv = torch.zeros_like(x0).requires_grad_(True)
    (rtg,) = torch.autograd.grad((F.interpolate(xv, size=(Hi, Hi), mode="bilinear", align_corners=False) * g_img).sum(), xv)
    return c1 * x0 + c2 * xt + sg * z - rtg


@pytest.mark.parametrize("C_,Cg", [(3, 10), (2, 2)])
@pytest.mark.parametrize("Ho,Hi", [(4, 3), (6, 5), (17, 16), (65, 64), (5, 8)])
def test_guided_resized_update_kernel(backend, Ho, Hi, C_, Cg):
    L, dev = backend
    B = 2
    g_ = torch.Generator().manual_seed(100 * Ho + Hi + C_)
    x0, xt, z = (torch.randn(B, C_, Ho, Ho, generator=g_) for _ in range(3))
    gr = torch.randn(B, Hi * Hi, Cg, generator=g_)
    c1, c2, sg = 0.3125, 0.71875, 0.09
    ref64, ref32 = (update_ref(x0, xt, z, gr, c1, c2, sg, C_, Hi, dt) for dt in (torch.float64, torch.float32))
    outs = []
    for rep in range(2):
        out = torch.full((B, C_, Ho, Ho), float('nan'), device=dev)
        a = [t.to(dev) for t in (x0, xt, z, gr)]
        L.check(L.pidm_psample_update_guided_resized(*(ptr(t) for t in a), c1, c2, sg, ptr(out), B, C_, Cg, Hi, Ho, stream_ptr(dev)),
                "pidm_psample_update_guided_resized")
        outs.append(out.cpu())
    assert torch.isfinite(outs[0]).all()
    check(f"update Ho={Ho} Hi={Hi} C={C_} Cg={Cg}", "x_prev", outs[0], ref32, ref64)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------------------------
# guards
# ------------------------------------------------------------------------------------------------------------------------------
def test_native_guards(backend, mesh_dir):
    L, dev = backend
    nel = 3
    res = get_res(backend, mesh_dir, nel)
    st = res.stiffs
    x, bcs, vf, y, g = make_inputs(nel, 1, 5)
    m = mask_of("sparse", 1, nel + 1, g)
    x, bcs, vf, y, m = (a.to(dev) for a in (x, bcs, vf, y, m))
    v, mo, s = torch.empty_like(x), torch.empty_like(y), torch.empty(1, 3, device=dev)
    mesh = [ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), ptr(st.dof_elems32), nel]

    def cot(bufs=None, mesh_=None, outs=None, B=1):
        bufs = bufs or [ptr(x), ptr(bcs), ptr(vf), ptr(y), ptr(m)]
        return L.pidm_mech_guidance_cotangent(*bufs, 1.0, 1.0, 1.0, *(mesh_ or mesh), *(outs or [ptr(v), ptr(mo), ptr(s)]), B, None)

    before = launches(L)
    assert cot(bufs=[ptr(x), ptr(bcs), ptr(vf), None, ptr(m)]) != 0 and b"null buffer" in L.pidm_last_error()
    assert cot(outs=[ptr(v), ptr(mo), None]) != 0 and b"null buffer" in L.pidm_last_error()
    assert cot(B=0) != 0 and b"B must be positive" in L.pidm_last_error()
    assert cot(mesh_=[None] + mesh[1:]) != 0 and b"null mesh table" in L.pidm_last_error()
    assert cot(mesh_=mesh[:3] + [None, nel]) != 0 and b"null mesh table" in L.pidm_last_error()
    assert cot(mesh_=mesh[:1] + [8] + mesh[2:]) != 0 and b"kloc_stride" in L.pidm_last_error()
    assert cot(mesh_=mesh[:4] + [80]) != 0 and b"LDS" in L.pidm_last_error()       # (the size check comes before any access)
    assert cot(mesh_=mesh[:4] + [0]) != 0 and b"nel" in L.pidm_last_error()
    a = torch.zeros(1, 2, 4, 4, device=dev)
    gg = torch.zeros(1, 9, 2, device=dev)
    upd = lambda g_=gg, B=1, C_=2, Cg=2, Hi=3, Ho=4, o=a: L.pidm_psample_update_guided_resized(
        ptr(a), ptr(a), ptr(a), ptr(g_) if g_ is not None else None, 1.0, 1.0, 1.0, ptr(o) if o is not None else None, B, C_, Cg, Hi,
        Ho, None)
    assert upd(g_=None) != 0 and b"null buffer" in L.pidm_last_error()
    assert upd(o=None) != 0 and b"null buffer" in L.pidm_last_error()
    assert upd(B=0) != 0 and b"B=0" in L.pidm_last_error()
    assert upd(B=65536) != 0 and b"B=65536" in L.pidm_last_error()
    assert upd(C_=3, Cg=2) != 0 and b"C=3" in L.pidm_last_error()
    assert upd(C_=0) != 0 and b"C=0" in L.pidm_last_error()
    assert upd(C_=2, Cg=17) != 0 and b"Cg=17" in L.pidm_last_error()
    assert upd(Hi=0) != 0 and b"Hi=0" in L.pidm_last_error()
    assert upd(Ho=0) != 0 and b"Ho=0" in L.pidm_last_error()
    assert launches(L) == before                                    # nothing was launched
    assert cot() == 0 and upd() == 0
    assert launches(L) == before + 2


def launches(L):
    a = (C.c_longlong * 4)()
    L.check(L.pidm_debug_launch_counts(a))
    return a[0]


def test_python_level_errors(backend, mesh_dir):
    L, dev = backend
    nel, B = 5, 2
    res = get_res(backend, mesh_dir, nel)
    x, bcs, vf, y, g = make_inputs(nel, B, 9)
    m = mask_of("sparse", B, nel + 1, g)
    x, bcs, vf, y, m = (a.to(dev) for a in (x, bcs, vf, y, m))
    with pytest.raises(PidmError, match="x0_pred must be"):
        res.guidance_cotangent(x[:, :2], bcs, vf, y, m, 1.0, 1.0)
    with pytest.raises(PidmError, match="x0_pred must be"):
        res.guidance_cotangent(y, bcs, vf, y, m, 1.0, 1.0)
    with pytest.raises(PidmError, match="bcs must be"):
        res.guidance_cotangent(x, bcs[:, :3], vf, y, m, 1.0, 1.0)
    with pytest.raises(PidmError, match="vf must be"):
        res.guidance_cotangent(x, bcs, vf[:1], y, m, 1.0, 1.0)
    with pytest.raises(PidmError, match="obs must be"):
        res.guidance_cotangent(x, bcs, vf, y[:, :, :nel], m, 1.0, 1.0)
    with pytest.raises(PidmError, match="mask must be"):
        res.guidance_cotangent(x, bcs, vf, y, m[:1], 1.0, 1.0)
    with pytest.raises(PidmError, match="floating-point"):
        res.guidance_cotangent(x, bcs, vf, y, m.bool(), 1.0, 1.0)
    with pytest.raises(PidmError, match="sums_out"):
        res.guidance_cotangent(x, bcs, vf, y, m, 1.0, 1.0, sums_out=torch.empty(B, 2, device=dev))
    with pytest.raises(PidmError, match="sums_out"):
        res.guidance_cotangent(x, bcs, vf, y, m, 1.0, 1.0, sums_out=torch.empty(B, 3, device=dev, dtype=torch.float64))
    if dev.type == "cpu":
        with pytest.raises(PidmError, match="no CPU fallback"):
            ResidualsMechanics(model=None, pixels_per_dim=nel, pixels_at_boundary=True, no_BC_folder="/nonexistent/",
                               device=dev).guidance_cotangent(x, bcs, vf, y, m, 1.0, 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# the sampler loop
# ------------------------------------------------------------------------------------------------------------------------------
ZETAS = (1.0, 1.0, 1.0)


def _loop_setup(backend, mesh_dir, n_steps=3, dim=8, nel=16, B=2):
    L, dev = backend
    lib = L if dev.type == "cpu" else None
    m = Unet3D(dim=dim, channels=10, out_dim=3, sigmoid_last_channel=True)
    m.load_state_dict(O.fill_state_dict(m.state_dict()))
    m = m.to(dev)
    m._pidm_lib = lib
    diff = DenoisingDiffusion(n_steps, dev, lib=lib)
    res = get_res(backend, mesh_dir, nel, model=m)
    nn = nel + 1
    g = torch.Generator().manual_seed(11)
    noises = [torch.randn(B, 3, nn, nn, generator=g) for _ in range(n_steps + 1)]
    _, bcs, vf, obs, _ = make_inputs(nel, B, 21)
    cond = torch.randn(B, 3, nn, nn, generator=g)
    cond[:, 0] = vf[:, None, None]
    mask = (torch.rand(B, 3, nn, nn, generator=g) < 0.1).float()
    mask[:, 2, : nn // 2] = 1.0                         # half of the design prescribed + a few displacement readings
    return m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, n_steps)


def _run(dev, noises, fn):
    it = iter(noises)
    with patched_rng(randn=lambda *a, **k: next(it).clone().to(dev), randn_like=lambda *a, **k: next(it).clone().to(dev)):
        return fn()


def test_guided_loop_teacher_forced(backend, mesh_dir):
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, n_steps) = _loop_setup(backend, mesh_dir)
    nn = nel + 1
    (x_seq, interm), aux = _run(dev, noises, lambda: diff.p_sample_loop_guided_mechanics(
        (cond.to(dev), bcs.to(dev)), (B, 3, nn, nn), res, obs.to(dev), mask.to(dev), *ZETAS))
    assert len(x_seq) == n_steps + 1 and len(interm) == n_steps + 1
    assert aux['guidance'].shape == (n_steps, B, 3) and aux['guidance'].device.type == dev.type
    assert aux['residual'].shape == (B,)
    cfg = O.UnetCfg(dim=dim, channels=10, out_dim=3, sigmoid_last_channel=True)
    p64 = R.params64(m.state_dict())
    tables64 = R.tables64(n_steps)
    kloc, ed = tables(res)
    assert torch.equal(x_seq[0], noises[0])
    for step, t in enumerate(reversed(range(n_steps))):
        # teacher forcing: the restatement advances the engine's own previous state
        x_ref, s_ref, g_ref = R.guided_step(p64, cfg, tables64, x_seq[step], cond, bcs, t, noises[1 + step], obs, mask, ZETAS, kloc, ed)
        err_ = (x_seq[1 + step].double() - x_ref).abs().max().item()
        bound = 5e-5 * max(x_ref.abs().max().item(), 1.0) + 2e-4 * g_ref.abs().max().item()
        print(f"t={t}: err {err_:.3e} bound {bound:.3e} |g| {g_ref.abs().max().item():.3e} |x| {x_ref.abs().max().item():.3e}")
        s = aux['guidance'][step].cpu().double()
        print("sums", s.tolist(), "ref", s_ref.tolist())
        assert g_ref.abs().max().item() > 0
        assert err_ <= bound, f"step t={t}"
        assert ((s - s_ref).abs() <= 1e-4 * s_ref.abs()).all(), f"step t={t}"
    x = x_seq[-1].double()
    r_ref = final_residual_ref(x, bcs, kloc, ed)
    print("final mean |r|", aux['residual'].tolist(), "ref", r_ref.tolist())
    assert ((aux['residual'].cpu().double() - r_ref).abs() <= 1e-4 * r_ref).all()


def final_residual_ref(x, bcs, kloc, ed):
    """per-sample mean |K_closed(rho) u - f| of a nodal state x [B,3,nn,nn] (u at the nodes, rho = x[:,2,:-1,:-1]), float64 by
    mech_ref.dense_K"""
    B = x.shape[0]
    E = (x.shape[-1] - 1) ** 2
    kloc_e = np.asarray(kloc, dtype=np.float64)
    if kloc_e.ndim == 2:
        kloc_e = np.broadcast_to(kloc_e, (E, 8, 8))
    out = []
    for b in range(B):
        K, f = MR.dense_K(x[b, 2, :-1, :-1].reshape(-1).numpy(), bcs[b].numpy(), kloc_e, ed)
        u = x[b, :2].permute(1, 2, 0).reshape(-1).numpy()
        out.append(np.abs(K @ u - f).mean())
    return torch.tensor(out, dtype=torch.float64)


def test_guided_loop_without_guidance_equals_p_sample_loop(backend, mesh_dir):
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, n_steps) = _loop_setup(backend, mesh_dir)
    nn = nel + 1
    ci = (cond.to(dev), bcs.to(dev), None)
    plain, _ = _run(dev, noises, lambda: diff.p_sample_loop(ci, (B, 3, nn, nn), save_output=True, residual_func=res))
    (x_seq, _), aux = _run(dev, noises, lambda: diff.p_sample_loop_guided_mechanics(ci, (B, 3, nn, nn), res, obs.to(dev), mask.to(dev),
                                                                                    0.0, 0.0, 0.0))
    err_ = (x_seq[-1] - plain[-1]).abs().max().item()
    print(f"unguided vs p_sample_loop: {err_:.3e}")
    assert err_ <= 5e-5 * max(plain[-1].abs().max().item(), 1.0)
    assert (aux['guidance'] > 0).all()                  # the sums are reported whatever the weights are


def test_guided_loop_replace_observed_and_broadcast(backend, mesh_dir):
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, n_steps) = _loop_setup(backend, mesh_dir)
    nn = nel + 1
    obs1, mask1 = obs[:1].clone(), mask[:1].clone()
    mask1[:, 2, :, nel] = 1.0                           # "observed" padding: must be left alone
    obs1[:, 2, :, nel] = 9.0
    (x_seq, interm), aux = _run(dev, noises, lambda: diff.p_sample_loop_guided_mechanics(
        (cond.to(dev), bcs.to(dev)), (B, 3, nn, nn), res, obs1.to(dev), mask1.to(dev), *ZETAS, guide_below=1, replace_observed=True,
        keep_history=False))
    # steps t = 2, 1 are plain p_sample arithmetic (no sums), t = 0 is guided
    assert (aux['guidance'][:2] == 0).all() and (aux['guidance'][2] > 0).all()
    assert len(x_seq) == 1 and len(interm) == 1 and x_seq[0].device.type == dev.type
    x = x_seq[0].cpu()
    on = mask1.expand(B, -1, -1, -1) != 0
    pad = torch.zeros_like(on)
    pad[:, 2, nel, :] = True
    pad[:, 2, :, nel] = True
    ob = obs1.expand(B, -1, -1, -1)
    assert torch.equal(x[on & ~pad], ob[on & ~pad])
    assert not torch.equal(x[~on], ob[~on])
    assert (x[:, 2, :, nel] != 9.0).all()
    # the padding is what the same loop leaves there without the replacement
    (x_seq2, _), _ = _run(dev, noises, lambda: diff.p_sample_loop_guided_mechanics(
        (cond.to(dev), bcs.to(dev)), (B, 3, nn, nn), res, obs1.to(dev), mask1.to(dev), *ZETAS, guide_below=1, keep_history=False))
    assert torch.equal(x[pad], x_seq2[0].cpu()[pad]) and torch.equal(x[~on], x_seq2[0].cpu()[~on])


def test_guided_loop_errors(backend, mesh_dir):
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, n_steps) = _loop_setup(backend, mesh_dir)
    nn = nel + 1
    shape, ci = (B, 3, nn, nn), (cond.to(dev), bcs.to(dev))
    loop = diff.p_sample_loop_guided_mechanics
    darcy = ResidualsDarcy(model=m, fd_acc=2, pixels_per_dim=nel, pixels_at_boundary=True, reverse_d1=True, device=dev, bcs='none',
                           lib=backend[0] if dev.type == "cpu" else None)
    with pytest.raises(PidmError, match="mechanics only"):
        loop(ci, shape, darcy, obs, mask)
    with pytest.raises(PidmError, match="mechanics only"):
        loop(ci, shape, None, obs, mask)
    with pytest.raises(PidmError, match="Darcy only"):                  # the Darcy loop keeps refusing a mechanics residual
        diff.p_sample_loop_guided((B, 2, nel, nel), res, obs, mask)
    with pytest.raises(PidmError, match="shape must be"):
        loop(ci, (B, 3, nel, nel), res, obs, mask)
    with pytest.raises(PidmError, match="obs must be"):
        loop(ci, shape, res, obs[:, :2], mask)
    with pytest.raises(PidmError, match="mask must be"):
        loop(ci, shape, res, obs, mask[:, :, :nel])
    with pytest.raises(PidmError, match="obs must be"):
        loop(ci, shape, res, torch.cat((obs, obs[:1])), mask)       # neither B nor 1 samples
    with pytest.raises(PidmError, match="conditioning must be"):
        loop((cond[:1], bcs), shape, res, obs, mask)
    with pytest.raises(PidmError, match="bcs must be"):
        loop((cond, bcs[:, :3]), shape, res, obs, mask)
    with pytest.raises(PidmError, match="conditioning_input must be"):
        loop(cond, shape, res, obs, mask)
    res.use_ddim_x0 = True
    with pytest.raises(PidmError, match="use_ddim_x0"):
        loop(ci, shape, res, obs, mask)
    res.use_ddim_x0 = False
    res.model = Unet3D(dim=8, channels=10, out_dim=3, sigmoid_last_channel=True, self_condition=True)
    with pytest.raises(PidmError, match="self-conditioning"):
        loop(ci, shape, res, obs, mask)


def test_guided_loop_leaves_no_trace(backend, mesh_dir):
    """After a guided loop every p.grad, the flat gradient buffer and a pending training tape of the model are unchanged."""
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, n_steps) = _loop_setup(backend, mesh_dir, n_steps=2)
    nn = nel + 1
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, nel * nel, 10, generator=g).to(dev)
    t = torch.randint(0, n_steps, (B,), generator=g).to(dev)
    w = torch.randn(B, 3, nel, nel, generator=g).to(dev)

    def train_step(between=None):
        for p in m.parameters():
            p.grad = None
        xr = x.clone().requires_grad_(True)
        out = m(xr, t)
        if between is not None:
            between()
        (out * w).sum().backward()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, xr.grad.clone()

    def guided():
        return _run(dev, noises, lambda: diff.p_sample_loop_guided_mechanics(
            (cond.to(dev), bcs.to(dev)), (B, 3, nn, nn), res, obs.to(dev), mask.to(dev), *ZETAS, keep_history=False))

    A, gxA = train_step()
    assert len(A) > 100
    eng = get_engine(m, nel, m._pidm_lib)
    flat_A = eng.flat_grad.clone()
    (xs, _), aux = guided()
    assert torch.isfinite(xs[0]).all() and (aux['guidance'] > 0).all()
    assert torch.equal(eng.flat_grad, flat_A)
    for k, p in m.named_parameters():
        if k in A:
            assert torch.equal(p.grad, A[k]), k
        else:
            assert p.grad is None, k
    # the same training step with a whole guided loop BETWEEN its forward and its backward (pending tape)
    A2, gxA2 = train_step(lambda: guided())
    assert A2.keys() == A.keys() and torch.equal(gxA2, gxA)
    for k in A:
        assert torch.equal(A2[k], A[k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# GPU only: the benchmark's mesh
# ------------------------------------------------------------------------------------------------------------------------------
def check_rel(name, got, ref, tol=1e-5):
    e = err(got, ref)
    print(f"GUIDED_MECH gpu {name}: {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (name, e)


@pytest.mark.gpu
def test_cotangent_nel64_b32_vs_composition_gpu(mesh_dir):
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    backend = (get_lib(), torch.device("cuda:0"))
    dev = backend[1]
    nel, B = 64, 32
    res = get_res(backend, mesh_dir, nel)
    x, bcs, vf, y, g = make_inputs(nel, B, 64032)
    m = mask_of("sparse", B, nel + 1, g)
    _, _, _, _, _, zetas, _ = reference(res, nel, 2, False, "sparse", "all")      # the weights of the nel = 64 case above
    xd, bd, vd, yd, md = (a.to(dev) for a in (x, bcs, vf, y, m))
    vc, moc, sc = composition(res, xd, bd, vd, yd, md, zetas)
    v, mo, s = res.guidance_cotangent(xd, bd, vd, yd, md, *zetas)
    assert torch.isfinite(v).all() and (s > 0).all()
    check_rel("v", v, vc)
    for j, name in enumerate(("L_obs", "L_pde", "L_vol")):
        check_rel(name, s[:, j], sc[:, j])
    assert torch.equal(mo, moc)


@pytest.mark.gpu
def test_two_guided_steps_dim32_nel64_gpu(mesh_dir):
    """Two guided steps at the benchmark's mesh against the same steps assembled on the device from input_gradient_pass, the
    composition of the existing residual kernels, autograd of F.interpolate for the resize adjoint and pidm_psample_update: the UNet
    passes are identical, only the new kernels differ."""
    from physicsinformeddiffusionmodels_amd._engine import input_gradient_pass
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    backend = (get_lib(), torch.device("cuda:0"))
    n_steps = 2
    m, diff, res, dev, noises, cond, bcs, obs, mask, (dim, nel, B, _) = _loop_setup(backend, mesh_dir, n_steps=n_steps, dim=32, nel=64)
    nn = nel + 1
    L = backend[0]
    (x_seq, _), aux = _run(dev, noises, lambda: diff.p_sample_loop_guided_mechanics(
        (cond.to(dev), bcs.to(dev)), (B, 3, nn, nn), res, obs.to(dev), mask.to(dev), *ZETAS))
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
        v, mo, sums = composition(res, x0p, bd, vf, od, md, ZETAS)
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
        print(f"GUIDED_MECH gpu t={t}: err {e:.3e} bound {bound:.3e} |g| {g.abs().max().item():.3e}")
        assert g.abs().max().item() > 0
        assert e <= bound
        for j in range(3):
            check_rel(f"t={t} sums[{j}]", aux['guidance'][step][:, j], sums[:, j])
