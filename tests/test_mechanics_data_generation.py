"""Mechanics training-data generation (csrc/k_mech_gen.hip, physicsinformeddiffusionmodels_amd/mechanics_data_generation.py)
against the dense float64 restatement of tests/simp_ref.py.

The bound on x_new is not fixed in advance: the restatement runs once exactly and once with its solved u multiplied by
1 + 10 pcg_rtol N(0,1) (how far a solve that is only converged to pcg_rtol may move the result); 10 x the largest difference of
the two is the bound.  u and the compliance are held to 100 pcg_rtol, relative.  Every comparison prints bound and observed
error before it asserts (DESIGN.md section 4b records them)."""
import os

import numpy as np
import pytest
import torch

from physicsinformeddiffusionmodels_amd import mechanics_data_generation as M
from physicsinformeddiffusionmodels_amd._lib import PidmError, ptr, stream_ptr
from tests import simp_ref as R

RTOL = 1e-10
_meshes = {}


def mesh(nel):
    if nel not in _meshes:
        _meshes[nel] = R.Mesh(nel)
    return _meshes[nel]


def _emu_or_gpu(backend):
    L, dev = backend
    return (L if dev.type == "cpu" else None), dev


def problems(nel, scenarios, seed0=100):
    """bcs [B,4,nn,nn] float32, vf [B] float32: one problem per requested support scenario."""
    ps = [M.sample_problem(seed0 + i, nel, scenario=s) for i, s in enumerate(scenarios)]
    return np.stack([p[0] for p in ps]), np.array([p[1] for p in ps], dtype=np.float32)


def start(kind, B, E, vf):
    if kind == "uniform":
        return np.repeat(vf.astype(np.float64)[:, None], E, axis=1)
    return np.random.RandomState(7).uniform(0.05, 1.0, size=(B, E))


def run_step(lib, dev, nel, x, u, bcs, vf, active=None, **kw):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt, device=dev)   # noqa: E731
    out = M.simp_step(t(x, torch.float64), t(u, torch.float64), t(bcs, torch.float32), t(vf, torch.float32), nel,
                      active=None if active is None else t(active, torch.int32), lib=lib, **kw)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items() if k != "ws"}


def dense_pair(nel, x, bcs, vf, rng):
    """The restatement's exact step and its perturbed twin for every sample of a batch."""
    ms = mesh(nel)
    exact = [R.simp_step(ms, x[b], bcs[b], float(vf[b])) for b in range(len(x))]
    pert = [R.simp_step(ms, x[b], bcs[b], float(vf[b]), perturb=(rng, 10 * RTOL)) for b in range(len(x))]
    return exact, pert


def check_step(tag, got, exact, pert):
    for b, (e, p) in enumerate(zip(exact, pert)):
        bound_x = 10 * np.abs(e["x"] - p["x"]).max()
        err_x = np.abs(got["x"][b] - e["x"]).max()
        err_u = np.abs(got["u"][b] - e["u"]).max() / np.abs(e["u"]).max()
        err_c = abs(got["compliance"][b] - e["compliance"]) / abs(e["compliance"])
        err_ch = abs(got["change"][b] - e["change"])
        print(f"{tag} sample {b}: x_new bound {bound_x:.2e} err {err_x:.2e}; u bound {100 * RTOL:.1e} err {err_u:.2e}; "
              f"c err {err_c:.2e}; change err {err_ch:.2e}; pcg {got['pcg_iters'][b]} relres {got['relres'][b]:.2e}")
        assert bound_x > 0
        assert err_x <= bound_x
        assert err_u <= 100 * RTOL
        assert err_c <= 100 * RTOL
        assert err_ch <= bound_x
        assert got["relres"][b] <= RTOL and got["pcg_iters"][b] > 0


# ---- 1: one step vs dense float64 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["uniform", "random"])
# (the kernel keeps 4, 17 or 25 dofs per lane in registers: nel = 8 / 12 take the first form, nel = 33 the second; the third
#  runs in test_full_size_five_steps)
@pytest.mark.parametrize("nel,scenarios", [(8, (0, 4, 6)), (12, (3, 7)), (33, (5,))])
def test_one_step_vs_dense(backend, nel, scenarios, kind):
    lib, dev = _emu_or_gpu(backend)
    B, E = len(scenarios), nel * nel
    bcs, vf = problems(nel, scenarios)
    x = start(kind, B, E, vf)
    got = run_step(lib, dev, nel, x, np.zeros((B, 2 * (nel + 1) ** 2)), bcs, vf, pcg_rtol=RTOL)
    exact, pert = dense_pair(nel, x, bcs, vf, np.random.RandomState(3))
    check_step(f"nel={nel} {kind}", got, exact, pert)


# ---- 2: ten-step chain ----------------------------------------------------------------------------------------------------------

def test_ten_step_chain(backend):
    lib, dev = _emu_or_gpu(backend)
    nel, scenarios = 8, (0, 4, 6)
    B, E, ms = len(scenarios), nel * nel, mesh(nel)
    bcs, vf = problems(nel, scenarios)
    rng = np.random.RandomState(11)
    xe = start("uniform", B, E, vf)
    xp, xk, uk = xe.copy(), xe.copy(), np.zeros((B, ms.neq))
    c_ref, c_ker = [], []
    for step in range(10):
        exact = [R.simp_step(ms, xe[b], bcs[b], float(vf[b])) for b in range(B)]
        pert = [R.simp_step(ms, xp[b], bcs[b], float(vf[b]), perturb=(rng, 10 * RTOL)) for b in range(B)]
        got = run_step(lib, dev, nel, xk, uk, bcs, vf, pcg_rtol=RTOL)
        xe, xp = np.stack([e["x"] for e in exact]), np.stack([p["x"] for p in pert])
        xk, uk = got["x"], got["u"]
        for b in range(B):
            assert abs(xe[b].mean() - vf[b]) <= 1e-6          # the restatement holds the volume constraint ...
            assert abs(xk[b].mean() - vf[b]) <= 1e-6          # ... and so does the kernel
            bound = 10 * np.abs(xe[b] - xp[b]).max()
            err = np.abs(xk[b] - xe[b]).max()
            print(f"chain step {step + 1} sample {b}: x bound {bound:.2e} err {err:.2e}, c {got['compliance'][b]:.6f} "
                  f"(dense {exact[b]['compliance']:.6f}), mean x {xk[b].mean():.8f}, pcg {got['pcg_iters'][b]}")
            assert bound > 0 and err <= bound
        c_ref.append([e["compliance"] for e in exact])
        c_ker.append(got["compliance"].copy())
    assert (np.array(c_ref[9]) < np.array(c_ref[0])).all()
    assert (c_ker[9] < c_ker[0]).all()


# ---- 3: warm start, activity, batch invariance ----------------------------------------------------------------------------------

def test_warm_start_activity_batch_invariance(backend):
    lib, dev = _emu_or_gpu(backend)
    nel, scenarios = 8, (1, 5, 2)
    B, E = len(scenarios), nel * nel
    bcs, vf = problems(nel, scenarios, seed0=300)
    x = start("random", B, E, vf)
    u0 = np.zeros((B, 2 * (nel + 1) ** 2))
    a = run_step(lib, dev, nel, x, u0, bcs, vf)
    assert (a["pcg_iters"] > 0).all() and (a["relres"] <= 1e-8).all()
    # the converged u with the same x: no iteration, u unchanged
    w = run_step(lib, dev, nel, x, a["u"], bcs, vf)
    print("warm start: relres", a["relres"], "->", w["relres"], "iterations", a["pcg_iters"], "->", w["pcg_iters"])
    assert (w["pcg_iters"] == 0).all()
    assert np.array_equal(w["u"], a["u"]) and np.array_equal(w["x"], a["x"])
    # an inactive sample comes back bit-identical, the others as before
    marker = np.random.RandomState(1).standard_normal(u0.shape)
    act = np.array([1, 0, 1], dtype=np.int32)
    m = run_step(lib, dev, nel, x, marker * (1 - act[:, None]), bcs, vf, active=act)
    assert np.array_equal(m["x"][1], x[1]) and np.array_equal(m["u"][1], marker[1])
    for b in (0, 2):
        assert np.array_equal(m["x"][b], a["x"][b]) and np.array_equal(m["u"][b], a["u"][b])
    # a batch of 3 = three batches of 1; two runs are identical
    for b in range(B):
        s = run_step(lib, dev, nel, x[b:b + 1], u0[b:b + 1], bcs[b:b + 1], vf[b:b + 1])
        for k in ("x", "u", "compliance", "change", "pcg_iters", "relres"):
            assert np.array_equal(s[k][0], a[k][b]), k
    a2 = run_step(lib, dev, nel, x, u0, bcs, vf)
    for k in ("x", "u", "compliance", "change", "pcg_iters", "relres"):
        assert np.array_equal(a2[k], a[k]), k


# ---- 4: fields ------------------------------------------------------------------------------------------------------------------

def test_fields_vs_dense(backend):
    lib, dev = _emu_or_gpu(backend)
    nel, B = 8, 2
    ms = mesh(nel)
    bcs, _ = problems(nel, (0, 7), seed0=500)
    rng = np.random.RandomState(5)
    rho = rng.uniform(0.05, 1.0, size=(B, nel * nel)).astype(np.float32)
    u = np.stack([ms.solve(rho[b].astype(np.float64), bcs[b]) for b in range(B)]).astype(np.float32)
    got = M.mech_fields(torch.from_numpy(u).to(dev), torch.from_numpy(rho).to(dev), nel, lib=lib).cpu().numpy()
    assert got.shape == (B, 2, nel + 1, nel + 1) and got.dtype == np.float32
    for b in range(B):
        ref, cnt = R.fields(ms, u[b].astype(np.float64), rho[b].astype(np.float64))
        assert cnt[0, 0] == 1 and cnt[0, 3] == 2 and cnt[3, 3] == 4 and set(np.unique(cnt)) == {1, 2, 4}
        for ch, name in enumerate(("strain energy density", "von Mises")):
            scale = np.abs(ref[ch]).max()
            for n in (1, 2, 4):        # corner, edge and interior averages each within the tolerance
                err = np.abs(got[b, ch] - ref[ch])[cnt == n].max() / scale
                print(f"fields sample {b} {name}, nodes with {n} element(s): err {err:.2e} (bound 2e-6)")
                assert err <= 2e-6
        assert ref.min() >= 0 and scale > 0


# ---- 5: round trip --------------------------------------------------------------------------------------------------------------

def test_dataset_round_trip(backend, tmp_path):
    from physicsinformeddiffusionmodels_amd.data_utils import Dataset_Paths
    lib, dev = _emu_or_gpu(backend)
    L = backend[0]
    nel, nn, seeds = 16, 17, [21, 22, 23, 24]
    out = tmp_path / "a"
    assert M.generate_mechanics_dataset(4, out, nel=nel, max_iter=15, seeds=seeds, device=dev, lib=lib) == seeds
    assert sorted(os.listdir(out)) == ["0.npy", "1.npy", "2.npy", "3.npy"]
    ds = Dataset_Paths(out)
    assert len(ds) == 4
    ms = mesh(nel)
    st = M._mesh(nel, dev)
    for i, s in enumerate(seeds):
        raw = np.load(out / f"{i}.npy")
        assert raw.shape == (nn, nn, 10) and raw.dtype == np.float32
        d = ds[i].numpy()
        assert d.shape == (10, nn, nn) and np.array_equal(d, raw.transpose(2, 0, 1))
        bcs, vf = M.sample_problem(s, nel)
        assert (d[0] == d[0, 0, 0]).all() and 0.3 <= d[0, 0, 0] <= 0.5 and d[0, 0, 0] == np.float32(vf)
        Ef = d[5]
        assert (Ef[nel, :] == 0).all() and (Ef[:, nel] == 0).all()
        assert set(np.unique(Ef[:nel, :nel])) <= {np.float32(1e-3), np.float32(1.0)} and (Ef[:nel, :nel] == 1).any()
        assert np.array_equal(d[6:10], bcs)
        assert np.isfinite(d).all() and d[1].max() > 0 and d[2].min() >= 0 and d[2].max() > 0
        # the stored displacements solve the stored field under the training operator: mean |r| <= 1e-5, the reference's own
        # acceptance figure for data (src/residuals_mechanics_K.py:305)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        res = torch.empty(1, st.neq, dtype=torch.float32, device=dev)
        comp = torch.empty(1, dtype=torch.float32, device=dev)
        E_t, u_t, bc_t = t(Ef[:nel, :nel]).reshape(1, -1), t(d[3:5]).unsqueeze(0), t(bcs).unsqueeze(0)
        L.check(L.pidm_mech_apply(ptr(E_t), ptr(u_t), ptr(bc_t), ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), ptr(st.dof_elems32), nel, ptr(res), ptr(comp), 1,
                                  stream_ptr(dev)))
        mean_r = float(res.abs().mean())
        # the dense restatement with fp32-rounded displacements sits at ~1e-7
        Evec = Ef[:nel, :nel].reshape(-1).astype(np.float64)
        ud = ms.solve(Evec, bcs).astype(np.float32).astype(np.float64)
        f, mask = ms.load_and_mask(bcs)
        mean_dense = np.abs(np.where(mask, ud, ms.dense_K(Evec) @ ud) - f).mean()
        print(f"round trip sample {i} (seed {s}): mean |r| {mean_r:.2e}, dense restatement with fp32 u {mean_dense:.2e}")
        assert mean_dense <= 1e-6
        assert mean_r <= 1e-5
    # same seeds, same bytes; other seeds, other files
    # (two short runs that share one seed: the shared sample does not depend on its batch mates)
    out2, out3 = tmp_path / "b", tmp_path / "c"
    M.generate_mechanics_dataset(2, out2, nel=nel, max_iter=2, seeds=[21, 31], device=dev, lib=lib)
    M.generate_mechanics_dataset(2, out3, nel=nel, max_iter=2, seeds=[21, 32], device=dev, lib=lib)
    assert (out2 / "0.npy").read_bytes() == (out3 / "0.npy").read_bytes()
    assert (out2 / "1.npy").read_bytes() != (out3 / "1.npy").read_bytes()
    assert (out2 / "0.npy").read_bytes() != (out / "0.npy").read_bytes()      # 2 iterations are not 15


# ---- 6: error paths ---------------------------------------------------------------------------------------------------------------

def test_errors(backend, tmp_path):
    lib, dev = _emu_or_gpu(backend)
    L = backend[0]
    nel = 8
    with pytest.raises(PidmError, match=r"did not converge.*#0 \(seed 1\).*#1 \(seed 2\)"):
        M.generate_mechanics_batch([1, 2], nel, device=dev, lib=lib, pcg_max_iter=3)
    with pytest.raises(PidmError, match="not unique"):
        M.generate_mechanics_dataset(3, str(tmp_path), seeds=[4, 5, 4], nel=nel, device=dev, lib=lib)
    bcs, vf = problems(nel, (0,))
    x = start("uniform", 1, nel * nel, vf)
    u = np.zeros((1, 2 * (nel + 1) ** 2))
    for kw, msg in ((dict(rmin=1.0), "rmin"), (dict(rmin=0.5), "rmin"), (dict(n_bisect=0), "n_bisect"), (dict(penal=0.5), "penal"),
                    (dict(e_min=0.0), "e_min"), (dict(e_min=1.0), "e_min")):
        with pytest.raises(PidmError, match=msg):
            run_step(lib, dev, nel, x, u, bcs, vf, **kw)
    # the native entry point itself: a mesh that does not fit LDS, null buffers, B <= 0
    st = M._mesh(nel, dev)
    d = torch.zeros(16, dtype=torch.float64, device=dev)
    f = torch.zeros(16, dtype=torch.float32, device=dev)
    i32 = torch.zeros(16, dtype=torch.int32, device=dev)
    mesh_args = (ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), ptr(st.dof_elems32))
    par = (3.0, 1e-3, 1.5, 0.2, 60, 100, 1e-8)
    d2 = torch.zeros(16, dtype=torch.float64, device=dev)
    outs = (ptr(d2), ptr(d2), ptr(d2), ptr(d2), ptr(i32), ptr(d2), ptr(d2))
    for bad_nel in (128, 80, 1):
        assert L.pidm_simp_step(ptr(d), ptr(d), ptr(f), ptr(f), None, *mesh_args, bad_nel, *par, *outs, 1, stream_ptr(dev)) != 0
        assert b"LDS" in L.pidm_last_error()
    assert L.pidm_simp_step(None, ptr(d), ptr(f), ptr(f), None, *mesh_args, nel, *par, *outs, 1, stream_ptr(dev)) != 0
    assert b"null" in L.pidm_last_error()
    assert L.pidm_simp_step(ptr(d), ptr(d), ptr(f), ptr(f), None, *mesh_args, nel, *par, *outs, 0, stream_ptr(dev)) != 0
    assert b"B=" in L.pidm_last_error()
    assert L.pidm_mech_fields(ptr(f), ptr(f), ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), 128, 0.3, ptr(f), 1, stream_ptr(dev)) != 0
    assert b"LDS" in L.pidm_last_error()
    assert L.pidm_mech_fields(None, ptr(f), ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), nel, 0.3, ptr(f), 1, stream_ptr(dev)) != 0
    assert L.pidm_simp_ws_bytes(64, 4) >= 4 * 2 * 8450 * 8


def test_product_library_rejects_cpu_tensors():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(PidmError):
        M.generate_mechanics_batch([1], 8, device="cpu")
    bcs, vf = problems(8, (0,))
    with pytest.raises(PidmError):
        M.simp_optimize(torch.from_numpy(bcs), vf, 8)
    with pytest.raises(PidmError):
        M.mech_fields(torch.zeros(1, 162), torch.ones(1, 64), 8)


def test_sample_problem_rules():
    """Every drawn problem is statically determinate or better: the dense K_FF at nel = 8 is non-singular for 200 seeds, and
    the load rules hold (unit point loads on free boundary nodes, nel/4 away from the supports, angles multiples of 30 degrees)."""
    nel = 8
    ms = mesh(nel)
    K = ms.dense_K(np.ones(ms.E))
    seen = set()
    for seed in range(200):
        for n_loads in ((1, 2) if seed < 40 else (1,)):
            bcs, vf = M.sample_problem(seed, nel, n_loads=n_loads)
            assert bcs.shape == (4, nel + 1, nel + 1) and bcs.dtype == np.float32 and 0.3 <= vf <= 0.5
            f, mask = ms.load_and_mask(bcs)
            ev = np.linalg.eigvalsh(K[np.ix_(~mask, ~mask)])
            # (a singular K_FF would show |ev[0]| ~ 1e-13 ev[-1] in fp64)
            assert ev[0] > 1e-10 * ev[-1] and np.isfinite(ev[-1] / ev[0])
            pinned = (bcs[0] != 0) | (bcs[1] != 0)
            loaded = np.argwhere((bcs[2] != 0) | (bcs[3] != 0))
            assert len(loaded) == n_loads
            pr = np.argwhere(pinned)
            for r, c in loaded:
                assert r in (0, nel) or c in (0, nel)
                assert not pinned[r, c]
                assert np.sqrt(((pr - [r, c]) ** 2).sum(1)).min() >= nel / 4
                fx, fy = float(bcs[2, r, c]), float(bcs[3, r, c])
                assert abs(np.hypot(fx, fy) - 1) < 1e-6
                ang = np.rad2deg(np.arctan2(fy, fx)) / 30.0
                assert abs(ang - round(ang)) < 1e-4
        b1, v1 = M.sample_problem(seed, nel)
        b2, v2 = M.sample_problem(seed, nel)
        assert np.array_equal(b1, b2) and v1 == v2
        seen.add((bcs[0].tobytes(), bcs[1].tobytes()))
    assert len(seen) >= 6            # at least six support scenarios occur
    for s in range(M.N_SCENARIOS):   # and every listed scenario removes the rigid-body modes
        bcs, _ = M.sample_problem(0, nel, scenario=s)
        _, mask = ms.load_and_mask(bcs)
        assert np.linalg.eigvalsh(K[np.ix_(~mask, ~mask)])[0] > 1e-6


def test_reference_module_path_reexports():
    import src.mechanics_data_generation as S
    for name in ("sample_problem", "simp_step", "simp_optimize", "mech_fields", "generate_mechanics_batch",
                 "generate_mechanics_dataset", "main"):
        assert getattr(S, name) is getattr(M, name)


# ---- 7: the full-size LDS layout (GPU only) -----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nel", [64, 72])
def test_full_size_five_steps(nel):
    dev = torch.device("cuda:0")
    from physicsinformeddiffusionmodels_amd._lib import get_lib
    L = get_lib()
    B, rtol = 4, 1e-8
    bcs, vf = problems(nel, (0, 4, 6, 3), seed0=700)
    E, ndof = nel * nel, 2 * (nel + 1) ** 2
    x, u = start("uniform", B, E, vf), np.zeros((B, ndof))
    comps = []
    for step in range(5):
        got = run_step(None, dev, nel, x, u, bcs, vf, pcg_rtol=rtol)
        x, u = got["x"], got["u"]
        print(f"nel={nel} step {step + 1}: c {got['compliance']}, pcg {got['pcg_iters']}, relres {got['relres']}, mean x {x.mean(1)}")
        assert (got["relres"] <= rtol).all() and (got["pcg_iters"] > 0).all()
        assert (np.abs(x.mean(1) - vf) <= 1e-6).all()
        assert ((x >= 0) & (x <= 1)).all()
        comps.append(got["compliance"].copy())
    comps = np.array(comps)
    assert (np.diff(comps, axis=0) < 0).all()
    # a final binarised solve satisfies the training operator
    st = M._mesh(nel, dev)
    bc_t = torch.from_numpy(bcs).to(dev)
    Ef = torch.where(torch.from_numpy(x).to(dev) > 0.5, 1.0, 1e-3).float().contiguous()
    ud = M._fe_solve(L, st, nel, Ef, bc_t, 1e-10, 20000, [f"#{i}" for i in range(B)], "final solve")
    u_img = ud.view(B, nel + 1, nel + 1, 2).permute(0, 3, 1, 2).contiguous()
    res = torch.empty(B, ndof, dtype=torch.float32, device=dev)
    comp = torch.empty(B, dtype=torch.float32, device=dev)
    L.check(L.pidm_mech_apply(ptr(Ef), ptr(u_img), ptr(bc_t), ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), ptr(st.dof_elems32),
                              nel, ptr(res), ptr(comp), B, stream_ptr(dev)))
    mean_r = res.abs().mean(dim=1).cpu().numpy()
    print(f"nel={nel} final binarised solve: mean |r|", mean_r)
    assert (mean_r <= 1e-5).all()
