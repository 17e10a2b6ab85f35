"""Darcy training data: the reference's `src/darcy_data_generation.py` with the solve on the gfx950 engine.

The reference draws a log-permeability field from a Karhunen-Loeve expansion (KLE) of an exponential covariance, assembles the
dense (P^2+4P+1) x P^2 finite-difference system of -div(K grad p) = f_s with Neumann rows and an integral row, and solves it
with `scipy.linalg.lstsq` (7.2 s per 64 x 64 sample on one CPU core).  Here the same functions keep their names and signatures,
and the solve runs in `csrc/k_darcy_gen_cgls.h`: one workgroup per sample, KLE synthesis and matrix-free column-scaled CGLS in
fp64 ("Darcy data generation"), in launches of a bounded number of iterations that carry the CGLS state between them.
`acc` (the reference's finite-difference order, 2 / 4 / 6) selects the operators of `csrc/k_darcy_gen_acc.hip`.
`bcs='periodic'` solves the system of `ResidualsDarcy(bcs='periodic')` instead - every operator central, on wrapped indices -
with those of `csrc/k_darcy_gen_per.hip`, on permeability fields of a wrapped-distance covariance.  Host-side pieces are the
grid, the eigendecomposition of the covariance (the reference's exact full `eigh`, cached) and the CSV writing.  There is no CPU
fallback for the solve.

    python -m physicsinformeddiffusionmodels_amd.darcy_data_generation --n-samples 10000 --out ./data/darcy/train
    python -m physicsinformeddiffusionmodels_amd.darcy_data_generation --n-samples 10000 --out ./data/darcy/train4 --acc 4
    python -m physicsinformeddiffusionmodels_amd.darcy_data_generation --n-samples 10000 --out ./data/darcy/trainp --bcs periodic
"""
from __future__ import annotations

import argparse
import itertools
import os
import time

import numpy as np
import torch

from ._lib import PidmError, get_lib, ptr, stream_ptr

# reference main() defaults (src/darcy_data_generation.py:166-185)
DEFAULTS = dict(pixels_per_dim=64, pixels_at_boundary=True, domain_length=1., length_scale=0.1, q=64, reverse_dy=True)
RTOL = 1e-12          # ||S A^T r|| / ||S A^T b|| at which a sample counts as solved (tests/test_darcy_data_generation.py)
MAX_ITER = 200000     # P = 64 takes ~40-50k iterations
ACCS = (2, 4, 6)
BCS = ('none', 'periodic')     # the reference's main.py: bcs = 'none' # 'none', 'periodic'
# max_iter=None: about twice the largest count measured at P = 64 (profiles/darcy_gen_bench_acc.txt)
MAX_ITER_ACC = {2: MAX_ITER, 4: 1000000, 6: 4000000}     # measured maxima at P = 64, batch 256: 494 k (acc 4), 2.04 M (acc 6)
# iterations per launch for a batch of at most one workgroup per compute unit: a launch at P = 64, acc 6, batch 256 then takes
# 0.60 s (30 us per iteration; bound: 2 s); _launch divides it by ceil(B / compute units)
ITERS_PER_LAUNCH = 20000


# ---- the reference's host functions (same names, signatures and results) ----------------------------------------------------

def uniform_points_pixelwise(n, domain_length, boundary=False, dim=2):
    xi = []
    for _ in range(dim):
        pixel_size = domain_length / n
        start, end = (0, domain_length) if boundary else (pixel_size / 2, domain_length - pixel_size / 2)
        xi.append(np.linspace(start, end, num=n))
    return np.array(list(itertools.product(*xi)))     # x is the outer index


def create_f_s(x, y, w=0.125, r=10.):
    c1 = np.abs(x - 0.5 * w) <= 0.5 * w
    c2 = np.abs(x - 1 + 0.5 * w) <= 0.5 * w
    c3 = np.abs(y - 0.5 * w) <= 0.5 * w
    c4 = np.abs(y - 1 + 0.5 * w) <= 0.5 * w
    out = np.zeros_like(x)
    out[np.logical_and(c1, c3)] = r
    out[np.logical_and(c2, c4)] = -r
    return out


def complete_covariance_matrix(grid, l):
    dx = grid[:, None, 0] - grid[None, :, 0]
    dy = grid[:, None, 1] - grid[None, :, 1]
    return np.exp(-np.sqrt(dx ** 2 + dy ** 2) / l)


def periodic_covariance_matrix(grid, l, period):
    """complete_covariance_matrix with each axis distance taken around the ring: min(|d|, period - |d|)."""
    dx = np.abs(grid[:, None, 0] - grid[None, :, 0])
    dy = np.abs(grid[:, None, 1] - grid[None, :, 1])
    dx, dy = np.minimum(dx, period - dx), np.minimum(dy, period - dy)
    return np.exp(-np.sqrt(dx ** 2 + dy ** 2) / l)


def compute_eigenpairs(cov_matrix, q):
    """First q eigenpairs of the covariance, descending (the full scipy.linalg.eigh, as the reference)."""
    from scipy.linalg import eigh
    w, v = eigh(cov_matrix)
    idx = np.argsort(w)[::-1]
    return w[idx][:q], v[:, idx][:, :q]


def KLE_expansion(eigenvalues, eigenvectors, q, grid_points, seed=None):
    """G = sum_k sqrt(lambda_k) z_k phi_k with z ~ N(0, 1)^q drawn after np.random.seed(seed) (the reference's norm.rvs draws the
    same numbers as np.random.standard_normal)."""
    if seed is not None:
        np.random.seed(seed)
    z = np.random.standard_normal(q)
    G = np.zeros(grid_points)
    for k in range(q):
        G += np.sqrt(eigenvalues[k]) * z[k] * eigenvectors[:, k]
    return G, z


def create_boundary_idcs(shape):
    masks = []
    for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)):
        m = np.zeros(shape, dtype=np.bool_)
        m[sl] = 1
        masks.append(m.reshape(-1))
    return tuple(masks)          # xmin, xmax, ymin, ymax


def create_int_cond(use_trapezoid, shape, d0):
    if use_trapezoid:
        c = np.full(shape, 4.)
        c[0, :] = c[-1, :] = c[:, 0] = c[:, -1] = 2.
        c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = 1.
        return c * (d0 ** 2 / 4.)
    return np.ones(shape).reshape(-1, 1) / (shape[0] ** 2)


def z_of_seed(seed, q):
    """The KLE coefficients a seed stands for (KLE_expansion without touching the global numpy state)."""
    return np.random.RandomState(int(seed)).standard_normal(q)


# ---- the engine --------------------------------------------------------------------------------------------------------------

def min_pixels(acc, bcs='none'):
    """Smallest grid of order acc: rows below acc/2 use forward stencils, and the second-derivative one of row acc/2 - 1 reaches
    column 3 acc/2 (9 at acc 6); 8 below that.  Periodic: 8 at every order (the widest wrapped stencil spans 7 points)."""
    return 8 if bcs == 'periodic' else max(8, 3 * acc // 2 + 1)


def _check_bcs(bcs):
    if bcs not in BCS:
        raise PidmError(f"darcy data generation: bcs={bcs!r} is not one of {BCS}")
    return bcs == 'periodic'


class DarcyProblem:
    """Grid-dependent, sample-independent data of the reference system: spacings, boundary sign, f_s and integral weights."""

    def __init__(self, P, pixels_at_boundary=True, reverse_dy=True, domain_length=1., acc=2, bcs='none'):
        if acc not in ACCS:
            raise PidmError(f"darcy data generation: acc={acc!r} is not one of the orders {ACCS} the gfx950 solve implements")
        self.periodic = _check_bcs(bcs)
        pmin = min_pixels(acc, bcs)
        if not pmin <= P <= 64:
            why = ("the wrapped stencil of order 6 spans 7 points" if self.periodic else
                   f"a one-sided second derivative of order {acc} spans {acc + 2} points")
            raise PidmError(f"darcy data generation: pixels_per_dim={P} outside [{pmin}, 64] at acc={acc}, bcs={bcs!r} ({why}; the "
                            f"solve keeps four fp64 P x P fields in LDS)")
        self.P, self.pixels_at_boundary, self.reverse_dy, self.acc = P, bool(pixels_at_boundary), bool(reverse_dy), acc
        self.bcs = bcs
        self.d0 = domain_length / (P - 1) if pixels_at_boundary else domain_length / P
        self.d1 = -self.d0 if reverse_dy else self.d0
        # y-min row: +D1 p with reverse_dy, -D1 p without (y-max the opposite), src/darcy_data_generation.py:147-150
        self.bc_sign = 1.0 if reverse_dy else -1.0
        pts = uniform_points_pixelwise(P, domain_length, pixels_at_boundary)
        self.points = pts
        self.f_s = create_f_s(pts[:, 0], pts[:, 1]).astype(np.float64)
        self.int_w = np.ascontiguousarray(create_int_cond(self.pixels_at_boundary, (P, P), self.d0), dtype=np.float64).reshape(-1)
        self._dev = {}

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.f_s).to(device), torch.from_numpy(self.int_w).to(device))
        return self._dev[key]


def _resolve(device, lib):
    device = torch.device(device) if device is not None else torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    if lib is None:
        if device.type != "cuda":
            raise PidmError("darcy data generation needs an MI355X (device cuda): the gfx950 solve has no CPU fallback")
        lib = get_lib()
    return device, lib


def _basis_file(P, l, q, pixels_at_boundary, domain_length, periodic=False):
    return (f"kle_basis_P{P}_l{l!r}_q{q}_b{int(bool(pixels_at_boundary))}_L{domain_length!r}" + ("_periodic" if periodic else "")
            + ".npy")


def kle_basis(P=64, l=0.1, q=64, pixels_at_boundary=True, cache_dir=None, domain_length=1., bcs='none'):
    """[q, P*P] float64: row k = sqrt(lambda_k) phi_k, the reference's eigenpairs (full eigh of the P^2 x P^2 covariance,
    descending).  Cached as .npy under cache_dir, keyed by the arguments.  Degenerate eigenpairs make the rows inside a pair
    depend on the LAPACK build; their span does not.  bcs='periodic': the covariance of the wrapped distance, period
    P x grid spacing (the spacing of DarcyProblem), so the fields continue smoothly across the edges the wrapped stencils cross."""
    periodic = _check_bcs(bcs)
    if q < 1 or q > P * P:
        raise PidmError(f"kle_basis: q={q} outside [1, P^2={P * P}]")
    path = os.path.join(cache_dir, _basis_file(P, l, q, pixels_at_boundary, domain_length, periodic)) if cache_dir else None
    if path and os.path.exists(path):
        return np.load(path)
    pts = uniform_points_pixelwise(P, domain_length, pixels_at_boundary)
    if periodic:
        period = P * (domain_length / (P - 1) if pixels_at_boundary else domain_length / P)
        lam, phi = compute_eigenpairs(periodic_covariance_matrix(pts, l, period), q)
        if not (lam > 0).all():      # (the wrapped exponential kernel is not positive definite by construction)
            raise PidmError(f"kle_basis: the wrapped covariance at P={P}, l={l!r} has a non-positive eigenvalue among its first "
                            f"{q} ({lam.min():.3e}): lower q")
    else:
        lam, phi = compute_eigenpairs(complete_covariance_matrix(pts, l), q)
    basis = np.ascontiguousarray((np.sqrt(lam)[None, :] * phi).T)
    if path:
        os.makedirs(cache_dir, exist_ok=True)
        np.save(path, basis)
    return basis


def _check_converged(relres, rtol, labels):
    bad = [labels[i] for i in np.nonzero(~(relres <= rtol))[0]]
    if bad:
        raise PidmError(f"darcy solve did not converge (||S A^T r|| / ||S A^T b|| > {rtol:g}) for sample(s) {bad}: raise max_iter")


def _outputs(B, P, device):
    """K, p [B, P^2], res [B], iters [B] (int32), relres [B]: what either entry writes"""
    f64 = dict(dtype=torch.float64, device=device)
    return (torch.empty(B, P * P, **f64), torch.empty(B, P * P, **f64), torch.empty(B, **f64),
            torch.empty(B, dtype=torch.int32, device=device), torch.empty(B, **f64))


def _launch(lib, device, prob, *, basis=None, z=None, K_in=None, B, max_iter, rtol, iters_per_launch=None, stats=None):
    """pidm_darcy_gen_acc, or pidm_darcy_gen_periodic for a periodic problem (same arguments, same state): launches of at most
    `iters_per_launch` iterations per sample until every sample is done; the B done flags are read back after each launch.  A
    batch larger than the device's compute units runs its workgroups one behind the other, so the budget of a launch is divided by
    ceil(B / compute units)."""
    P = prob.P
    name = "pidm_darcy_gen_periodic" if prob.periodic else "pidm_darcy_gen_acc"
    entry = getattr(lib, name)
    f_s, int_w = prob.on(device)
    if iters_per_launch is None:
        iters_per_launch = ITERS_PER_LAUNCH
    iters_per_launch = int(iters_per_launch)
    if iters_per_launch < 1:
        raise PidmError(f"darcy data generation: iters_per_launch={iters_per_launch} must be >= 1")
    if device.type == "cuda" and B > 0:
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        iters_per_launch = max(1, iters_per_launch // -(-B // cus))
    iters_per_launch = min(iters_per_launch, 2 ** 31 - 1)
    K, p, res, iters, relres = _outputs(B, P, device)
    done = torch.zeros(B, dtype=torch.int32, device=device)
    state = torch.empty(max(1, lib.pidm_darcy_gen_acc_state_bytes(P, B) // 8), dtype=torch.float64, device=device)
    q = 0 if z is None else z.shape[1]
    launches, longest, first = 0, 0., 1
    most = int(max_iter) // iters_per_launch + 2         # every launch advances every unfinished sample by iters_per_launch
    while True:
        t0 = time.perf_counter()
        lib.check(entry(ptr(basis), ptr(z), q, ptr(K_in), P, prob.acc, prob.d0, prob.d1, prob.bc_sign, ptr(int_w), ptr(f_s),
                        int(max_iter), float(rtol), iters_per_launch, first, ptr(state), ptr(K), ptr(p), ptr(res), ptr(iters),
                        ptr(relres), ptr(done), B, stream_ptr(device)), name)
        finished = bool(done.cpu().all())                # (a few hundred bytes; also waits for the launch)
        longest = max(longest, time.perf_counter() - t0)
        launches, first = launches + 1, 0
        if finished:
            break
        if launches >= most:
            raise PidmError(f"{name}: samples unfinished after {launches} launches of {iters_per_launch} iterations "
                            f"(max_iter={max_iter})")
    if stats is not None:
        stats.update(launches=launches, longest_launch_s=longest, iters_per_launch=iters_per_launch)
    return K, p, res, iters, relres


def generate_darcy_batch(seeds, pixels_per_dim=64, q=64, length_scale=0.1, pixels_at_boundary=True, reverse_dy=True,
                         domain_length=1., basis=None, max_iter=None, rtol=RTOL, cache_dir=None, device=None, lib=None, acc=2,
                         iters_per_launch=None, stats=None, bcs='none'):
    """Samples for the given seeds: K = exp(KLE(z(seed))) and the reference's least-squares pressure p at finite-difference order
    `acc` (2, 4 or 6).  Returns (K [B,P*P], p [B,P*P], res [B], iters [B]) on the device, fp64 (res = mean |row residual| over all
    P^2+4P+1 rows).  `basis` ([q, P*P], see kle_basis) overrides the eigendecomposition.  max_iter=None: MAX_ITER_ACC[acc].
    The solve runs in launches of at most `iters_per_launch` iterations (None: ITERS_PER_LAUNCH, scaled to the batch); `stats` (a
    dict) receives `launches`, `longest_launch_s` and `iters_per_launch`.  bcs='periodic': the periodic system (wrapped central
    operators) on fields of the periodic kle_basis."""
    device, lib = _resolve(device, lib)
    P = pixels_per_dim
    prob = DarcyProblem(P, pixels_at_boundary, reverse_dy, domain_length, acc, bcs)
    max_iter = MAX_ITER_ACC[acc] if max_iter is None else max_iter
    seeds = [int(s) for s in seeds]
    if basis is None:
        basis = kle_basis(P, length_scale, q, pixels_at_boundary, cache_dir, domain_length, bcs)
    basis = np.ascontiguousarray(basis, dtype=np.float64)
    if basis.ndim != 2 or basis.shape[1] != P * P or not 1 <= basis.shape[0] <= P * P:
        raise PidmError(f"KLE basis of shape {basis.shape} does not fit q <= P^2 = {P * P} modes of {P} x {P}")
    q = basis.shape[0]
    z = torch.from_numpy(np.stack([z_of_seed(s, q) for s in seeds]) if seeds else np.zeros((0, q))).to(device)
    bt = torch.from_numpy(basis).to(device)
    K, p, res, iters, relres = _launch(lib, device, prob, basis=bt, z=z.contiguous(), B=len(seeds), max_iter=max_iter, rtol=rtol,
                                       iters_per_launch=iters_per_launch, stats=stats)
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    _check_converged(relres.cpu().numpy(), rtol, [f"#{i} (seed {s})" for i, s in enumerate(seeds)])
    return K, p, res, iters


def solve_darcy_pressure(K, pixels_at_boundary=True, reverse_dy=True, domain_length=1., max_iter=None, rtol=RTOL, lib=None,
                         return_iters=False, acc=2, iters_per_launch=None, bcs='none'):
    """The reference's least-squares pressure for given permeability fields K ([B,P,P] or [P,P], fp64 on the device) at
    finite-difference order `acc`.  Returns (p shaped like K, res [B]) - and iters [B] with return_iters.  max_iter,
    iters_per_launch, bcs: see generate_darcy_batch."""
    if not isinstance(K, torch.Tensor):
        raise PidmError("solve_darcy_pressure: K must be a torch tensor on the device")
    if lib is None and not K.is_cuda:
        raise PidmError("solve_darcy_pressure needs tensors on an MI355X: the gfx950 solve has no CPU fallback")
    lib = lib or get_lib()
    shape = K.shape
    if K.dim() == 2:
        K = K.unsqueeze(0)
    if K.dim() != 3 or K.shape[1] != K.shape[2]:
        raise PidmError(f"solve_darcy_pressure: K of shape {tuple(shape)} is not [B,P,P] or [P,P]")
    B, P = K.shape[0], K.shape[1]
    prob = DarcyProblem(P, pixels_at_boundary, reverse_dy, domain_length, acc, bcs)
    max_iter = MAX_ITER_ACC[acc] if max_iter is None else max_iter
    Kin = K.to(torch.float64).reshape(B, P * P).contiguous()
    _, p, res, iters, relres = _launch(lib, K.device, prob, K_in=Kin, B=B, max_iter=max_iter, rtol=rtol,
                                       iters_per_launch=iters_per_launch)
    if K.is_cuda:
        torch.cuda.synchronize(K.device)
    _check_converged(relres.cpu().numpy(), rtol, [f"#{i}" for i in range(B)])
    p = p.reshape(shape)
    return (p, res, iters) if return_iters else (p, res)


def _unique_seeds(n, seed=None):
    """n distinct seeds in [0, 2^32) - from `seed` when given, else fresh entropy (unique per run, as the reference's
    pid * time seeds)."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        for s in rng.integers(0, 2 ** 32, size=n - len(out), dtype=np.uint64).tolist():
            if s not in seen:
                seen.add(s)
                out.append(s)
    return out


def generate_darcy_dataset(n_samples, out_dir, seed=None, seeds=None, batch=256, pixels_per_dim=64, q=64, length_scale=0.1,
                           pixels_at_boundary=True, reverse_dy=True, domain_length=1., max_iter=None, rtol=RTOL,
                           cache_dir=None, device=None, lib=None, verbose=False, acc=2, iters_per_launch=None, bcs='none'):
    """Writes out_dir/{seeds,K_data,p_data,res_data}.csv exactly as the reference main() (no header, no index, one row per
    sample) plus kle_basis.npy (the scaled basis the seeds were expanded in: a seed fixes K only together with it).
    `seeds` (explicit, must be distinct) or `seed` (draws n_samples distinct seeds reproducibly); neither: fresh ones.
    `acc`: the finite-difference order of the system the pressures solve (use the fd_acc the model will be trained with);
    `bcs`: 'none' or 'periodic', likewise the bcs of the training residual."""
    import pandas as pd
    if seeds is None:
        seeds = _unique_seeds(n_samples, seed)
    seeds = [int(s) for s in seeds]
    if len(seeds) != n_samples:
        raise PidmError(f"generate_darcy_dataset: {len(seeds)} seeds for {n_samples} samples")
    if len(set(seeds)) != len(seeds):
        dup = sorted({s for s in seeds if seeds.count(s) > 1})
        raise PidmError(f"Seeds are not unique: {dup}")
    if batch < 1:
        raise PidmError("generate_darcy_dataset: batch must be >= 1")
    P = pixels_per_dim
    DarcyProblem(P, pixels_at_boundary, reverse_dy, domain_length, acc, bcs)     # argument checks before the eigendecomposition
    basis = kle_basis(P, length_scale, q, pixels_at_boundary, cache_dir, domain_length, bcs)
    Ks, ps, rs = [], [], []
    t0 = time.time()
    for lo in range(0, n_samples, batch):
        K, p, res, iters = generate_darcy_batch(seeds[lo:lo + batch], P, q, length_scale, pixels_at_boundary, reverse_dy,
                                                domain_length, basis=basis, max_iter=max_iter, rtol=rtol, device=device, lib=lib,
                                                acc=acc, iters_per_launch=iters_per_launch, bcs=bcs)
        Ks.append(K.cpu().numpy())
        ps.append(p.cpu().numpy())
        rs.append(res.cpu().numpy())
        if verbose:
            it = iters.cpu().numpy()
            print(f"samples {lo}..{lo + len(it) - 1}: iterations {it.min()}..{it.max()}, {time.time() - t0:.1f} s")
    os.makedirs(out_dir, exist_ok=True)
    pd.DataFrame(seeds).to_csv(os.path.join(out_dir, "seeds.csv"), index=False, header=False)
    pd.DataFrame(np.concatenate(Ks) if Ks else np.zeros((0, P * P))).to_csv(os.path.join(out_dir, "K_data.csv"), index=False, header=False)
    pd.DataFrame(np.concatenate(ps) if ps else np.zeros((0, P * P))).to_csv(os.path.join(out_dir, "p_data.csv"), index=False, header=False)
    pd.DataFrame(np.concatenate(rs) if rs else np.zeros(0)).to_csv(os.path.join(out_dir, "res_data.csv"), index=False, header=False)
    np.save(os.path.join(out_dir, "kle_basis.npy"), basis)
    return seeds


def generate_sample(args):
    """The reference's per-sample worker: same argument tuple, same (K, p, mean |residual|, seed) result; K from the given
    eigenpairs on the host, the least-squares solve on the engine.  The tuple has no bcs: always the non-periodic system."""
    (i, eigenvalues, eigenvectors, q, pixels_per_dim, shape, acc, d0, d1, f_s, int_cond, xmin_bd, xmax_bd, ymin_bd, ymax_bd,
     reverse_dy) = args
    if acc not in ACCS:
        raise PidmError(f"the gfx950 solve implements acc in {ACCS}, not {acc!r}")
    unique_seed = os.getpid() * int(time.time() * 1000) % (2 ** 32)
    G, _ = KLE_expansion(eigenvalues, eigenvectors, q, pixels_per_dim ** 2, seed=unique_seed)
    K = np.exp(G.reshape(shape))
    P = pixels_per_dim
    pixels_at_boundary = np.shape(int_cond) == tuple(shape)      # create_int_cond: trapezoid weights [P,P], else a mean [P^2,1]
    p, res = solve_darcy_pressure(torch.from_numpy(K).to(_resolve(None, None)[0]), pixels_at_boundary=pixels_at_boundary,
                                  reverse_dy=reverse_dy, domain_length=abs(d0) * ((P - 1) if pixels_at_boundary else P), acc=acc)
    return K.flatten(), p.cpu().numpy().flatten(), float(res.cpu()[0]), unique_seed


def main(argv=None):
    ap = argparse.ArgumentParser(description="Darcy training data (reference src/darcy_data_generation.py) on the MI355X")
    ap.add_argument("--n-samples", type=int, default=10)
    ap.add_argument("--out", default="./data/darcy/")
    ap.add_argument("--seed", type=int, default=None, help="draw the sample seeds reproducibly (default: fresh per run)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pixels-per-dim", type=int, default=DEFAULTS["pixels_per_dim"])
    ap.add_argument("--q", type=int, default=DEFAULTS["q"])
    ap.add_argument("--length-scale", type=float, default=DEFAULTS["length_scale"])
    ap.add_argument("--pixels-at-boundary", type=int, default=1)
    ap.add_argument("--reverse-dy", type=int, default=1)
    ap.add_argument("--acc", type=int, default=2, choices=ACCS, help="finite-difference order of the system (the model's fd_acc)")
    ap.add_argument("--bcs", default="none", choices=BCS, help="boundary conditions of the system and the fields (the model's bcs)")
    ap.add_argument("--max-iter", type=int, default=None, help="default: MAX_ITER_ACC of the order")
    ap.add_argument("--iters-per-launch", type=int, default=None,
                    help="CGLS iterations per kernel launch for a batch of one workgroup per compute unit")
    ap.add_argument("--rtol", type=float, default=RTOL)
    ap.add_argument("--cache-dir", default=None, help="where the KLE basis is cached (default: not cached)")
    a = ap.parse_args(argv)
    t0 = time.time()
    generate_darcy_dataset(a.n_samples, a.out, seed=a.seed, batch=a.batch, pixels_per_dim=a.pixels_per_dim, q=a.q,
                           length_scale=a.length_scale, pixels_at_boundary=bool(a.pixels_at_boundary),
                           reverse_dy=bool(a.reverse_dy), max_iter=a.max_iter, rtol=a.rtol, cache_dir=a.cache_dir, verbose=True,
                           acc=a.acc, iters_per_launch=a.iters_per_launch, bcs=a.bcs)
    print(f"Data generation finished: {a.n_samples} samples in {time.time() - t0:.1f} s -> {a.out}")


if __name__ == "__main__":
    main()
