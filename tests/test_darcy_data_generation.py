"""Darcy training-data generation at the default order 2 (csrc/k_darcy_gen_cgls.h with the operators of csrc/k_darcy_gen_acc.hip,
physicsinformeddiffusionmodels_amd/darcy_data_generation.py) against a dense float64 least-squares oracle, the reference
generator's golden samples (g25) and the engine's own training residual."""
import functools
import os

import numpy as np
import pytest
import torch

from physicsinformeddiffusionmodels_amd import darcy_data_generation as D
from physicsinformeddiffusionmodels_amd._lib import PidmError
from tests import darcy_gen_ref as R
from tests.darcy_gen_ref import CASES, TOL, emu_or_gpu as _emu_or_gpu


def _d(P, h, order):
    M = np.zeros((P, P))
    if order == 1:
        M[0, :3], M[-1, -3:] = [-1.5, 2, -.5], [.5, -2, 1.5]
        for i in range(1, P - 1):
            M[i, i - 1:i + 2] = [-.5, 0, .5]
    else:
        M[0, :4], M[-1, -4:] = [2, -5, 4, -1], [-1, 4, -5, 2]
        for i in range(1, P - 1):
            M[i, i - 1:i + 2] = [1, -2, 1]
    return M / h ** order


_dense_case = functools.partial(R.dense_case, lambda P, h, order, acc: _d(P, h, order), "none")   # (this file's second-order rows)


@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("pab,rev", CASES)
def test_solve_matches_dense_lstsq(backend, P, pab, rev):
    _dense_case(*_emu_or_gpu(backend), P, pab, rev, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("pab,rev", CASES)
def test_solve_matches_dense_lstsq_p32(pab, rev):
    _dense_case(None, torch.device("cuda:0"), 32, pab, rev, 2)


def test_kle_synthesis_matches_numpy(backend):
    lib, dev = _emu_or_gpu(backend)
    P = 16
    basis = D.kle_basis(P, 0.1, 64, True)
    seeds = [5, 6, 7]
    K, p, res, iters = D.generate_darcy_batch(seeds, P, basis=basis, device=dev, lib=lib)
    for i, s in enumerate(seeds):
        ref = np.exp(basis.T @ D.z_of_seed(s, 64))
        np.testing.assert_allclose(K[i].cpu().numpy(), ref, rtol=1e-12, atol=0)
    assert (iters.cpu().numpy() > 0).all()


def test_seed_draw_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "g25_darcy_data.npz"))
    for P in (16, 64):
        for s in range(2):
            seed = int(g[f"P{P}_s{s}_seed"])
            assert np.array_equal(D.z_of_seed(seed, 64), g[f"P{P}_s{s}_z"])
            _, z = D.KLE_expansion(np.ones(64), np.zeros((4, 64)), 64, 4, seed=seed)
            assert np.array_equal(z, g[f"P{P}_s{s}_z"])


@pytest.mark.parametrize("P", [16, pytest.param(64, marks=pytest.mark.slow)])
def test_golden_field_in_kle_span(golden_dir, P):
    """log K of the reference lies in the span of kle_basis; inside every cluster of equal eigenvalues (x <-> y symmetric grid:
    LAPACK may return any rotation of a degenerate pair) the coefficient energy sum c_k^2 / lambda_k equals sum z_k^2."""
    g = np.load(os.path.join(golden_dir, "g25_darcy_data.npz"))
    basis = D.kle_basis(P, 0.1, 64, True)
    lam = (basis ** 2).sum(1)
    np.testing.assert_allclose(lam, g[f"P{P}_eigenvalues"], rtol=1e-10)
    phi = basis / np.sqrt(lam)[:, None]
    clusters, k = [], 0
    while k < 64:
        e = k + 1
        while e < 64 and abs(lam[e] - lam[k]) <= 1e-9 * lam[k]:
            e += 1
        clusters.append((k, e))
        k = e
    assert any(e - k == 2 for k, e in clusters)     # degenerate pairs exist
    for s in range(2):
        G = np.log(g[f"P{P}_s{s}_K"])
        c = phi @ G
        assert np.linalg.norm(G - phi.T @ c) <= 1e-8 * np.linalg.norm(G)
        z = g[f"P{P}_s{s}_z"]
        for k, e in clusters:
            np.testing.assert_allclose((c[k:e] ** 2 / lam[k:e]).sum(), (z[k:e] ** 2).sum(), rtol=1e-8, atol=1e-12)


def _golden_solve(golden_dir, P, lib, dev):
    g = np.load(os.path.join(golden_dir, "g25_darcy_data.npz"))
    K = np.stack([g[f"P{P}_s{s}_K"].reshape(P, P) for s in range(2)])
    p, res = D.solve_darcy_pressure(torch.from_numpy(K).to(dev), lib=lib)
    for s in range(2):
        pref, rref = g[f"P{P}_s{s}_p"], float(g[f"P{P}_s{s}_res"])
        assert np.abs(p[s].cpu().numpy().reshape(-1) - pref).max() <= TOL * np.abs(pref).max()
        assert abs(float(res[s]) - rref) <= TOL * rref


def test_golden_solve_p16(backend, golden_dir):
    lib, dev = _emu_or_gpu(backend)
    _golden_solve(golden_dir, 16, lib, dev)


@pytest.mark.gpu
def test_golden_solve_p64(golden_dir):
    _golden_solve(golden_dir, 64, None, torch.device("cuda:0"))


def test_batch_invariance(backend):
    lib, dev = _emu_or_gpu(backend)
    P = 8
    basis = D.kle_basis(P, 0.1, 64, True)
    seeds = list(range(100, 113))
    Kb, pb, _, _ = D.generate_darcy_batch(seeds, P, basis=basis, device=dev, lib=lib)
    K1, p1, _, _ = D.generate_darcy_batch([seeds[7]], P, basis=basis, device=dev, lib=lib)
    assert torch.equal(Kb[7], K1[0]) and torch.equal(pb[7], p1[0])


def test_launch_stats_and_split_invariance(backend):
    """A default (acc=2) call reports its launches; cut into launches of 50 iterations it takes several and returns the same bits."""
    lib, dev = _emu_or_gpu(backend)
    P = 8
    basis = D.kle_basis(P, 0.1, 64, True)
    seeds = [5, 6, 7]
    one, cut = {}, {}
    ref = D.generate_darcy_batch(seeds, P, basis=basis, device=dev, lib=lib, stats=one)
    out = D.generate_darcy_batch(seeds, P, basis=basis, device=dev, lib=lib, stats=cut, iters_per_launch=50)
    assert one["launches"] >= 1 and isinstance(one["longest_launch_s"], float) and one["longest_launch_s"] > 0
    assert isinstance(one["iters_per_launch"], int)
    assert cut["launches"] > 1 and cut["iters_per_launch"] == 50
    for a, b in zip(ref, out):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_dataset_round_trip_into_training(tmp_path):
    import pandas as pd
    from physicsinformeddiffusionmodels_amd.data_utils import Dataset
    from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
    P, n = 64, 6
    out = str(tmp_path / "darcy")
    seeds = D.generate_darcy_dataset(n, out, seed=3, batch=4)
    for name, cols in (("seeds", 1), ("K_data", P * P), ("p_data", P * P), ("res_data", 1)):
        arr = pd.read_csv(os.path.join(out, name + ".csv"), header=None).to_numpy()
        assert arr.shape == (n, cols), name
        with open(os.path.join(out, name + ".csv")) as f:
            assert len(f.readlines()) == n
    assert pd.read_csv(os.path.join(out, "seeds.csv"), header=None).to_numpy()[:, 0].tolist() == seeds
    assert np.load(os.path.join(out, "kle_basis.npy")).shape == (64, P * P)
    ds = Dataset((os.path.join(out, "p_data.csv"), os.path.join(out, "K_data.csv")))
    x = torch.stack([ds[i] for i in range(len(ds))])
    assert tuple(x.shape) == (n, 2, P, P)
    res_csv = pd.read_csv(os.path.join(out, "res_data.csv"), header=None).to_numpy()[:, 0]
    rd = ResidualsDarcy(model=None, fd_acc=2, pixels_per_dim=P, pixels_at_boundary=True, reverse_d1=True, device="cuda:0")
    r = rd.residual_of(x.float().cuda()).double().cpu()
    mean_abs = r.abs().sum(dim=(1, 2)) / (P * P + 4 * P + 1)
    # fp32 bound: each residual row is a sum of stencil terms K * p_00 ~ |K| |p| / h^2 (|p| ~ 0.1-1, 1/h^2 = 3969) that cancel to
    # ~4e-3; with fp32 inputs and arithmetic each row carries an error ~ 1e-7 x (sum of |terms|) ~ 1e-7 x 1e2 ~ 1e-5 absolute,
    # mostly random in sign, so the MEAN of |rows| moves by ~ 1e-5 at most against 4e-3: ~3e-3 relative at worst, 1e-3 typical
    np.testing.assert_allclose(mean_abs.numpy(), res_csv, rtol=5e-3)


def test_errors(backend, tmp_path):
    lib, dev = _emu_or_gpu(backend)
    P = 8
    basis = D.kle_basis(P, 0.1, 64, True)
    with pytest.raises(PidmError, match=r"did not converge.*#0 \(seed 1\).*#1 \(seed 2\)"):
        D.generate_darcy_batch([1, 2], P, basis=basis, device=dev, lib=lib, max_iter=3)
    with pytest.raises(PidmError, match="q="):
        D.kle_basis(P, 0.1, P * P + 1, True)
    with pytest.raises(PidmError):
        D.generate_darcy_batch([1], P, basis=np.zeros((P * P + 1, P * P)), device=dev, lib=lib)
    for bad in (7, 65, 128):
        with pytest.raises(PidmError, match="outside"):
            D.solve_darcy_pressure(torch.ones(1, bad, bad, dtype=torch.float64, device=dev), lib=lib)
    with pytest.raises(PidmError, match="not unique"):
        D.generate_darcy_dataset(3, str(tmp_path), seeds=[4, 5, 4], pixels_per_dim=P, device=dev, lib=lib)
    # the native entry point itself rejects what the Python layer would have caught
    f = torch.zeros(P * P, dtype=torch.float64, device=dev)
    out = torch.zeros(1, P * P, dtype=torch.float64, device=dev)
    from physicsinformeddiffusionmodels_amd._lib import ptr, stream_ptr
    L = lib or __import__("physicsinformeddiffusionmodels_amd._lib", fromlist=["get_lib"]).get_lib()
    zz = torch.zeros(1, P * P + 1, dtype=torch.float64, device=dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    state = torch.zeros(L.pidm_darcy_gen_acc_state_bytes(P, 1) // 8, dtype=torch.float64, device=dev)
    assert L.pidm_darcy_gen_acc(ptr(f), ptr(zz), P * P + 1, None, P, 2, 0.1, 0.1, 1.0, ptr(f), ptr(f), 10, 1e-10, 10, 1, ptr(state),
                                ptr(out), ptr(out), None, None, None, ptr(done), 1, stream_ptr(dev)) != 0
    assert b"darcy_gen_acc" in L.pidm_last_error() and b"q=" in L.pidm_last_error()
    assert L.pidm_darcy_gen_acc(None, None, 0, ptr(out), 128, 2, 0.1, 0.1, 1.0, ptr(f), ptr(f), 10, 1e-10, 10, 1, ptr(state),
                                None, ptr(out), None, None, None, ptr(done), 1, stream_ptr(dev)) != 0
    assert b"darcy_gen_acc" in L.pidm_last_error() and b"P=128" in L.pidm_last_error()


def test_product_library_rejects_cpu_tensors():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(PidmError):
        D.solve_darcy_pressure(torch.ones(1, 16, 16, dtype=torch.float64))
    with pytest.raises(PidmError):
        D.generate_darcy_batch([1], 16, basis=np.zeros((4, 256)), device="cpu")


def test_reference_module_path_reexports():
    import src.darcy_data_generation as S
    for name in ("uniform_points_pixelwise", "create_f_s", "complete_covariance_matrix", "compute_eigenpairs", "KLE_expansion",
                 "create_boundary_idcs", "create_int_cond", "generate_sample", "main", "kle_basis", "generate_darcy_batch",
                 "solve_darcy_pressure", "generate_darcy_dataset"):
        assert getattr(S, name) is getattr(D, name)
