"""Periodic Darcy training-data generation (csrc/k_darcy_gen_per.hip, the `bcs='periodic'` keyword of
physicsinformeddiffusionmodels_amd/darcy_data_generation.py) against a dense float64 least-squares oracle built from
grad_utils.fd_coefficients on wrapped indices, the launch-split protocol, the periodic KLE basis, the engine's own periodic training
residual and one training step on the generated files.  The reference's generator has no periodic mode, so there is no golden."""
import functools
import os

import numpy as np
import pytest
import torch

from physicsinformeddiffusionmodels_amd import darcy_data_generation as D
from physicsinformeddiffusionmodels_amd import grad_utils as G
from physicsinformeddiffusionmodels_amd._lib import PidmError, ptr, stream_ptr
from tests import darcy_gen_ref as R
from tests.darcy_gen_ref import CASES, TOL, emu_or_gpu as _emu_or_gpu

# TOL: the project's figure for this solve (tests/darcy_gen_ref.py), on the max-norm relative error of p and the relative
# error of res.  A NumPy CGLS with the kernel's algorithm (column scaling, rtol 1e-12) stays at or below 1.4e-10 on p against
# lstsq for every periodic system of P <= 32.


def _d(P, h, order, acc):
    """Dense 1-D operator: the central stencil of order acc in every row, tap i + o at column (i + o) mod P."""
    M = np.zeros((P, P))
    for i in range(P):
        for o, w in G.fd_coefficients(order, acc, "C").items():
            M[i, (i + o) % P] += w
    return M / h ** order


_basis, _field = functools.partial(R.basis, bcs="periodic"), functools.partial(R.field, bcs="periodic")
_system, dense_lstsq = functools.partial(R.system, _d, "periodic"), functools.partial(R.dense_lstsq, _d, "periodic")
_dense_case = functools.partial(R.dense_case, _d, "periodic")


def _spectral_field(P, pab, seed, q=64):
    """exp of a sample of the rank-q truncation of the periodic covariance without the P^2 x P^2 eigh (half a minute at P = 64): the
    covariance depends on the ring distance only, so the Fourier modes are its eigenvectors and fft2 of one of its rows holds its
    eigenvalues (test_periodic_kle_basis checks both against kle_basis)."""
    h = 1. / (P - 1) if pab else 1. / P
    r = np.minimum(np.arange(P), P - np.arange(P)) * h
    lam = np.fft.fft2(np.exp(-np.sqrt(r[:, None] ** 2 + r[None, :] ** 2) / 0.1)).real
    cut = np.sort(lam.reshape(-1))[-q]
    w = np.random.RandomState(seed).standard_normal((P, P))
    return np.exp(np.fft.ifft2(np.sqrt(np.where(lam >= cut, lam, 0.)) * np.fft.fft2(w)).real), lam


# ---- 1. dense oracle ------------------------------------------------------------------------------------------------------------

# P = 8 at acc 6: the wrapped stencil spans 7 of the 8 points; P = 10: no multiple of the wave or of the lanes' stride
@pytest.mark.parametrize("acc,P", [(2, 8), (4, 8), (6, 8), (4, 10), (6, 16)])
@pytest.mark.parametrize("pab,rev", CASES)
def test_solve_matches_dense_lstsq(backend, acc, P, pab, rev):
    _dense_case(*_emu_or_gpu(backend), P, pab, rev, acc)


@pytest.mark.gpu
@pytest.mark.parametrize("acc", [2, 6])
@pytest.mark.parametrize("pab,rev", [(True, True), (False, True)])
def test_solve_matches_dense_lstsq_p32(acc, pab, rev):
    _dense_case(None, torch.device("cuda:0"), 32, pab, rev, acc)


# ---- 2. launch split ----------------------------------------------------------------------------------------------------------------

def test_split_invariance(backend):
    """A solve cut into launches of 7 or 100 iterations is bit-identical to the same solve in one launch."""
    lib, dev = _emu_or_gpu(backend)
    P, acc = 10, 6
    runs, stats = [], []
    for n in (10 ** 9, 100, 7):
        st = {}
        runs.append(D.generate_darcy_batch([977, 27], P, basis=_basis(P, True), device=dev, lib=lib, acc=acc, bcs="periodic",
                                           iters_per_launch=n, stats=st))
        stats.append(st)
    K1, p1, r1, it1 = runs[0]
    print(f"iterations {it1.tolist()}, launches {[st['launches'] for st in stats]}")
    assert stats[0]["launches"] == 1
    for (K, p, r, it), st in zip(runs[1:], stats[1:]):
        assert st["launches"] > 1
        assert torch.equal(it, it1)
        assert torch.equal(p, p1)
        assert torch.equal(r, r1)
        assert torch.equal(K, K1)


# ---- 3. batch invariance ----------------------------------------------------------------------------------------------------------------

def test_batch_invariance(backend):
    lib, dev = _emu_or_gpu(backend)
    P = 10
    basis = _basis(P, True)
    seeds = list(range(100, 113))
    Kb, pb, rb, _ = D.generate_darcy_batch(seeds, P, basis=basis, device=dev, lib=lib, acc=4, bcs="periodic")
    K1, p1, r1, _ = D.generate_darcy_batch([seeds[7]], P, basis=basis, device=dev, lib=lib, acc=4, bcs="periodic")
    assert torch.equal(Kb[7], K1[0]) and torch.equal(pb[7], p1[0]) and torch.equal(rb[7], r1[0])


# ---- 4. periodic KLE ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pab", [True, False])
def test_periodic_kle_basis(pab, tmp_path, monkeypatch):
    P, q = 8, 64
    basis = D.kle_basis(P, 0.1, q, pab, bcs="periodic")
    assert basis.shape == (q, P * P)
    pts = D.uniform_points_pixelwise(P, 1., pab)
    h = 1. / (P - 1) if pab else 1. / P
    d = np.abs(pts[:, None, :] - pts[None, :, :])
    d = np.minimum(d, P * h - d)
    cov = np.exp(-np.sqrt((d ** 2).sum(-1)) / 0.1)
    assert np.abs(basis.T @ basis - cov).max() <= 1e-10          # q = P^2: the full decomposition
    # a function of the ring distance only: rolling both grid axes (of both points) leaves it unchanged
    c4 = cov.reshape(P, P, P, P)
    for sx, sy in ((1, 0), (0, 3), (5, 2)):
        assert np.abs(np.roll(c4, (sx, sy, sx, sy), axis=(0, 1, 2, 3)) - c4).max() <= 1e-12
    # the descending order and the scaling of the non-periodic basis: row norms^2 are the eigenvalues
    lam = (basis ** 2).sum(1)
    assert (np.diff(lam) <= 1e-12).all() and lam[-1] > 0
    np.testing.assert_allclose(lam, np.sort(_spectral_field(P, pab, 0)[1].reshape(-1))[::-1], rtol=1e-10)
    # cache: a suffix only when periodic, so existing caches stay valid
    cache = str(tmp_path)
    b_per = D.kle_basis(P, 0.1, q, pab, cache_dir=cache, bcs="periodic")
    b_non = D.kle_basis(P, 0.1, q, pab, cache_dir=cache)
    names = sorted(os.listdir(cache))
    assert names == [f"kle_basis_P8_l0.1_q64_b{int(pab)}_L1.0.npy", f"kle_basis_P8_l0.1_q64_b{int(pab)}_L1.0_periodic.npy"]
    assert np.array_equal(np.load(os.path.join(cache, names[1])), b_per) and np.array_equal(b_per, basis)
    assert np.array_equal(D.kle_basis(P, 0.1, q, pab, cache_dir=cache, bcs="periodic"), basis)       # read back
    # the non-periodic call is what it was
    assert np.array_equal(D.kle_basis(P, 0.1, q, pab, bcs="none"), D.kle_basis(P, 0.1, q, pab))
    assert np.array_equal(b_non, D.kle_basis(P, 0.1, q, pab))
    assert not np.array_equal(b_non, basis)
    # a non-positive eigenvalue among the q used is an error, not a NaN basis
    monkeypatch.setattr(D, "compute_eigenpairs", lambda c, n: (np.array([1., -1e-3]), np.zeros((P * P, 2))))
    with pytest.raises(PidmError, match="non-positive"):
        D.kle_basis(P, 0.1, 2, pab, bcs="periodic")


# ---- 5. consistency with the training residual ----------------------------------------------------------------------------------------------

def _training_residual_case(lib, dev, P, acc, pab, fields, seeds=()):
    """fields [B, P, P]; seeds: those of the fields that come from _field, for the dense comparison with the non-periodic pressures"""
    from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
    rows = P * P + 4 * P + 1
    K = torch.from_numpy(fields).to(dev)
    rd = ResidualsDarcy(model=None, fd_acc=acc, pixels_per_dim=P, pixels_at_boundary=pab, reverse_d1=True, device=dev,
                        bcs="periodic", lib=lib)
    p, res = D.solve_darcy_pressure(K, pab, True, lib=lib, acc=acc, bcs="periodic")
    x = torch.stack([p, K], dim=1).float()
    own = (rd.residual_of(x).double().abs().sum(dim=(1, 2)) / rows).cpu().numpy()
    print(f"acc {acc} P {P} pab {pab}: training residual {own}, generator {res.cpu().numpy()}")
    # fp32 bound of tests/test_darcy_data_generation_acc.py::test_consistent_with_training_residual
    np.testing.assert_allclose(own, res.cpu().numpy(), rtol=5e-3)
    if not seeds:
        return
    # the non-periodic pressures of the same fields are not the minimiser of the periodic rows (both have zero integral)
    pn, _ = D.solve_darcy_pressure(K, pab, True, lib=lib, acc=acc)
    for s, seed in enumerate(seeds):
        _, Abi, b = _system(P, pab, True, acc, seed)
        ss_per = ((Abi @ p[s].cpu().numpy().reshape(-1) - b) ** 2).sum()
        ss_non = ((Abi @ pn[s].cpu().numpy().reshape(-1) - b) ** 2).sum()
        print(f"  seed {seed}: sum of squared periodic rows {ss_per:.6e} (periodic p), {ss_non:.6e} (non-periodic p)")
        assert ss_non > ss_per


@pytest.mark.parametrize("acc", [2, 4])
@pytest.mark.parametrize("pab", [True, False])
def test_consistent_with_training_residual(backend, acc, pab):
    """Why the generator takes bcs: periodic data has, under ResidualsDarcy(bcs='periodic'), the mean |row residual| the generator
    reports, and non-periodic pressures of the same fields leave a strictly larger sum of squared periodic rows."""
    P, seeds = 16, (977, 27)
    _training_residual_case(*_emu_or_gpu(backend), P, acc, pab, np.stack([_field(P, pab, s) for s in seeds]), seeds)


@pytest.mark.gpu
def test_consistent_with_training_residual_p64():
    _training_residual_case(None, torch.device("cuda:0"), 64, 2, False, _spectral_field(64, False, 977)[0][None])


# ---- 6. round trip into training ------------------------------------------------------------------------------------------------------------

def test_dataset_round_trip_into_training(backend, tmp_path):
    """generate_darcy_dataset(bcs='periodic') -> data_utils.Dataset -> one loss + backward step of the circular UNet on the periodic
    residual (after tests/test_darcy_data_generation.py::test_dataset_round_trip_into_training)."""
    import pandas as pd
    from oracle import pidm_oracle as O
    from physicsinformeddiffusionmodels_amd.data_utils import Dataset
    from physicsinformeddiffusionmodels_amd.denoising_utils import DenoisingDiffusion
    from physicsinformeddiffusionmodels_amd.residuals_darcy import ResidualsDarcy
    from physicsinformeddiffusionmodels_amd.unet_model import Unet3D
    lib, dev = _emu_or_gpu(backend)
    P, n = 16, 4
    out = str(tmp_path / "darcy_periodic")
    seeds = D.generate_darcy_dataset(n, out, seed=1, pixels_per_dim=P, bcs="periodic", device=dev, lib=lib)
    assert sorted(os.listdir(out)) == ["K_data.csv", "kle_basis.npy", "p_data.csv", "res_data.csv", "seeds.csv"]
    for name, cols in (("seeds", 1), ("K_data", P * P), ("p_data", P * P), ("res_data", 1)):
        arr = pd.read_csv(os.path.join(out, name + ".csv"), header=None).to_numpy()
        assert arr.shape == (n, cols), name
    assert pd.read_csv(os.path.join(out, "seeds.csv"), header=None).to_numpy()[:, 0].tolist() == seeds
    assert np.array_equal(np.load(os.path.join(out, "kle_basis.npy")), _basis(P, True))
    # the pressures are those of the periodic system of the same fields
    _, pref, rref = dense_lstsq(P, True, True, 2, seeds[0])
    p_csv = pd.read_csv(os.path.join(out, "p_data.csv"), header=None).to_numpy()
    res_csv = pd.read_csv(os.path.join(out, "res_data.csv"), header=None).to_numpy()[:, 0]
    assert np.abs(p_csv[0] - pref).max() <= TOL * np.abs(pref).max()
    assert abs(res_csv[0] - rref) <= TOL * rref
    ds = Dataset((os.path.join(out, "p_data.csv"), os.path.join(out, "K_data.csv")))
    x = torch.stack([ds[i] for i in range(len(ds))]).to(dev)
    assert tuple(x.shape) == (n, 2, P, P)
    m = Unet3D(dim=8, padding_mode="circular")
    m.load_state_dict(O.fill_state_dict(m.state_dict()))
    m = m.to(dev)
    m._pidm_lib = lib
    rd = ResidualsDarcy(model=m, fd_acc=2, pixels_per_dim=P, pixels_at_boundary=True, reverse_d1=True, device=dev, bcs="periodic",
                        lib=lib)
    diff = DenoisingDiffusion(100, dev, lib=lib)
    torch.manual_seed(0)
    loss = diff.model_estimation_loss(x, residual_func=rd, c_data=1., c_residual=1e-3)[0]
    assert torch.isfinite(loss)
    loss.backward()
    grads = [prm.grad for prm in m.parameters() if prm.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert any(float(g.abs().sum()) > 0. for g in grads)


# ---- 7. errors and the command line ---------------------------------------------------------------------------------------------------------

def test_errors(backend):
    lib, dev = _emu_or_gpu(backend)
    one = lambda P: torch.ones(1, P, P, dtype=torch.float64, device=dev)   # noqa: E731
    with pytest.raises(PidmError, match="bcs='dirichlet'"):
        D.solve_darcy_pressure(one(16), lib=lib, bcs="dirichlet")
    with pytest.raises(PidmError, match="bcs='dirichlet'"):
        D.generate_darcy_batch([1], 16, basis=np.zeros((4, 256)), device=dev, lib=lib, bcs="dirichlet")
    with pytest.raises(PidmError, match="bcs='dirichlet'"):
        D.kle_basis(8, 0.1, 4, bcs="dirichlet")
    with pytest.raises(PidmError, match="bcs='dirichlet'"):
        D.DarcyProblem(16, bcs="dirichlet")
    with pytest.raises(PidmError, match="bcs='dirichlet'"):
        D.generate_darcy_dataset(1, "unused", seed=1, pixels_per_dim=16, device=dev, lib=lib, bcs="dirichlet")
    for P in (7, 65):
        for acc in D.ACCS:
            with pytest.raises(PidmError, match=r"outside \[8, 64\]"):
                D.solve_darcy_pressure(one(P), lib=lib, acc=acc, bcs="periodic")
    D.DarcyProblem(8, acc=6, bcs="periodic")      # (the non-periodic system needs 10 points at this order)
    with pytest.raises(PidmError, match="acc=3"):
        D.solve_darcy_pressure(one(16), lib=lib, acc=3, bcs="periodic")
    P = 10
    with pytest.raises(PidmError, match=r"did not converge.*#0 \(seed 1\).*#1 \(seed 2\)"):
        D.generate_darcy_batch([1, 2], P, basis=_basis(P, True), device=dev, lib=lib, acc=4, bcs="periodic", max_iter=3)
    with pytest.raises(PidmError, match="iters_per_launch"):
        D.solve_darcy_pressure(one(P), lib=lib, acc=4, bcs="periodic", iters_per_launch=0)
    # the native entry point itself rejects what the Python layer would have caught
    L = lib or __import__("physicsinformeddiffusionmodels_amd._lib", fromlist=["get_lib"]).get_lib()
    f = torch.zeros(P * P, dtype=torch.float64, device=dev)
    Kin = torch.ones(1, P * P, dtype=torch.float64, device=dev)
    out = torch.zeros(1, P * P, dtype=torch.float64, device=dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    state = torch.zeros(L.pidm_darcy_gen_acc_state_bytes(P, 1) // 8, dtype=torch.float64, device=dev)

    def call(acc=4, P_=P, st=state, n=10, o=out, fs=f, dn=done, kin=Kin):
        return L.pidm_darcy_gen_periodic(None, None, 0, ptr(kin), P_, acc, 0.1, 0.1, 1.0, ptr(Kin), ptr(fs), 10, 1e-10, n, 1, ptr(st),
                                         None, ptr(o), None, None, None, ptr(dn), 1, stream_ptr(dev))
    assert call(acc=3) != 0 and b"acc=3" in L.pidm_last_error()
    assert call(P_=65) != 0 and b"outside" in L.pidm_last_error()
    assert call(P_=7) != 0 and b"outside" in L.pidm_last_error()
    assert call(n=0) != 0 and b"iters_this_launch" in L.pidm_last_error()
    assert call(st=None) != 0 and b"state" in L.pidm_last_error()
    assert call(o=None) != 0 and b"null buffer" in L.pidm_last_error()
    assert call(fs=None) != 0 and b"null buffer" in L.pidm_last_error()
    assert call(dn=None) != 0 and b"done" in L.pidm_last_error()
    assert call(kin=None) != 0 and b"K_in" in L.pidm_last_error()
    assert call() == 0          # (and the same arguments untouched are accepted)
    for acc in D.ACCS:
        assert L.pidm_darcy_gen_periodic_lds_bytes(64, acc) == (4 * 64 * 64 + 4 * 64 + (acc + 2) * 2 + 8) * 8 <= 160 * 1024
    assert L.pidm_darcy_gen_periodic_lds_bytes(64, 5) == 0


def test_cli(backend, tmp_path, monkeypatch):
    import pandas as pd
    lib, dev = _emu_or_gpu(backend)
    if lib is not None:       # the command line has no library argument: hand the emulated one to the module's device lookup
        monkeypatch.setattr(D, "_resolve", lambda device, L: (dev, lib))
    out = str(tmp_path / "cli")
    D.main(["--n-samples", "2", "--pixels-per-dim", "8", "--bcs", "periodic", "--out", out])
    for name, cols in (("seeds", 1), ("K_data", 64), ("p_data", 64), ("res_data", 1)):
        assert pd.read_csv(os.path.join(out, name + ".csv"), header=None).to_numpy().shape == (2, cols), name
    K = pd.read_csv(os.path.join(out, "K_data.csv"), header=None).to_numpy()
    seeds = pd.read_csv(os.path.join(out, "seeds.csv"), header=None).to_numpy()[:, 0]
    for i in range(2):        # fields of the periodic basis
        np.testing.assert_allclose(K[i], np.exp(_basis(8, True).T @ D.z_of_seed(seeds[i], 64)), rtol=1e-12)
    with pytest.raises(SystemExit):
        D.main(["--n-samples", "2", "--bcs", "dirichlet", "--out", out])
