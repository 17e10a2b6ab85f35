"""Mechanics (topology-optimisation) training data on the gfx950 engine.

The reference trains its second study on one `.npy` per sample ([65,65,10]: vf, strain energy density, von Mises stress, disp_x,
disp_y, E_field, BC_node_x, BC_node_y, load_x, load_y; `main.py:90-101`, `src/data_utils.py:118`) but never generated those
files - they were downloaded.  This module produces them: a batched SIMP (solid isotropic material with penalisation) compliance
minimiser, one `pidm_simp_step` launch per iteration (csrc/k_mech_gen.hip: fp64 matrix-free PCG, sensitivity filter and
optimality-criteria update, one workgroup per sample), then a final FE solve of the stored field under the training operator
(`pidm_mech_solve`) and the two conditioning fields of the uniform domain (`pidm_mech_fields`).  DESIGN.md section 4b.  Host-side
pieces are the random problem draw and the file writing.  There is no CPU fallback.
`filter='density'` / `'heaviside'` run the three-field form instead (`pidm_simp_step_filtered`: design variables -> density filter
-> tanh projection with beta continuation), whose near-binary result the 0.5 cut hardly changes; `binarize='volume'` makes the stored
solid fraction equal vf.  The defaults write the files they always wrote.

Support scenarios of `sample_problem` (node grid [row, col], row 0 is the top edge; every one removes the three rigid-body modes):
  0  left edge clamped              1  right edge clamped
  2  top edge clamped               3  bottom edge clamped
  4  bottom-left corner pinned, bottom-right corner on a y-roller (pinned in y only)
  5  top-left corner pinned, top-right corner on a y-roller
  6  left edge on x-rollers (pinned in x only), bottom-right corner pinned in y
  7  bottom edge on y-rollers (pinned in y only), top-left corner pinned in x

    python -m physicsinformeddiffusionmodels_amd.mechanics_data_generation --n-samples 1000 --out ./data/mechanics/train/fields
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from ._lib import PidmError, get_lib, ptr, stream_ptr
from .darcy_data_generation import _unique_seeds
from .residuals_mechanics_K import StiffnessMatrix

N_SCENARIOS = 8
NU = 0.3              # Poisson's ratio of the element stiffness (StiffnessMatrix)
E_VOID = 1e-3         # Young's modulus of void in the stored field (the evaluation block binarises to the same pair)
FINAL_RTOL = 1e-10    # the stored displacements: ||r|| / ||f|| of the final solves


# ---- the random problem (host, plain NumPy) ----------------------------------------------------------------------------------

def _supports(scenario, nel):
    """bc_x, bc_y [nn,nn] bool masks of a support scenario (module docstring)."""
    nn = nel + 1
    bx, by = np.zeros((nn, nn), dtype=bool), np.zeros((nn, nn), dtype=bool)
    if scenario == 0:
        bx[:, 0] = by[:, 0] = True
    elif scenario == 1:
        bx[:, nel] = by[:, nel] = True
    elif scenario == 2:
        bx[0, :] = by[0, :] = True
    elif scenario == 3:
        bx[nel, :] = by[nel, :] = True
    elif scenario == 4:
        bx[nel, 0] = by[nel, 0] = by[nel, nel] = True
    elif scenario == 5:
        bx[0, 0] = by[0, 0] = by[0, nel] = True
    elif scenario == 6:
        bx[:, 0] = True
        by[nel, nel] = True
    elif scenario == 7:
        by[nel, :] = True
        bx[0, 0] = True
    else:
        raise PidmError(f"sample_problem: unknown support scenario {scenario}")
    return bx, by


def sample_problem(seed, nel=64, n_loads=1, scenario=None):
    """One random compliance problem: (bcs [4,nn,nn] float32 = (BC_node_x, BC_node_y, load_x, load_y), vf).
    Drawn from np.random.RandomState(seed): a support scenario (module docstring), vf ~ U[0.3, 0.5] and n_loads unit point loads,
    each on a boundary node without a pinned dof at least nel/4 away from every pinned node, at an angle that is a multiple of
    30 degrees.  `scenario` fixes the support scenario instead of drawing it."""
    if nel < 4:
        raise PidmError(f"sample_problem: nel={nel} must be >= 4")
    if n_loads not in (1, 2):
        raise PidmError(f"sample_problem: n_loads={n_loads} must be 1 or 2")
    rs = np.random.RandomState(int(seed))
    drawn = int(rs.randint(N_SCENARIOS))
    bx, by = _supports(drawn if scenario is None else int(scenario), nel)
    vf = float(rs.uniform(0.3, 0.5))
    nn = nel + 1
    r, c = np.meshgrid(np.arange(nn), np.arange(nn), indexing="ij")
    pinned = bx | by
    pr, pc = r[pinned], c[pinned]
    dist = np.sqrt((r[..., None] - pr) ** 2 + (c[..., None] - pc) ** 2).min(-1)
    boundary = (r == 0) | (r == nel) | (c == 0) | (c == nel)
    cand = np.argwhere(boundary & ~pinned & (dist >= nel / 4.))
    bcs = np.zeros((4, nn, nn), dtype=np.float32)
    bcs[0], bcs[1] = bx, by
    placed = []
    while len(placed) < n_loads:
        rr, cc = (int(v) for v in cand[rs.randint(len(cand))])
        ang = np.deg2rad(30. * rs.randint(12))
        fx, fy = np.round(np.cos(ang), 12), np.round(np.sin(ang), 12)
        # redraw a load that would act on pinned dofs only (cannot happen on a node without pinned dofs; kept as the rule) or
        # that lands on a node already loaded
        if (rr, cc) in placed or not ((fx != 0 and not bx[rr, cc]) or (fy != 0 and not by[rr, cc])):
            continue
        bcs[2, rr, cc], bcs[3, rr, cc] = fx, fy
        placed.append((rr, cc))
    return bcs, vf


# ---- the engine --------------------------------------------------------------------------------------------------------------

_meshes: dict = {}


def _mesh(nel, device):
    key = (int(nel), str(device))
    if key not in _meshes:
        _meshes[key] = StiffnessMatrix(no_BC_folder=None, nels_per_side=nel, device=device, dtype=torch.float32)
    return _meshes[key]


def _resolve(device, lib):
    device = torch.device(device) if device is not None else torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    if lib is None:
        if device.type != "cuda":
            raise PidmError("mechanics data generation needs an MI355X (device cuda): the gfx950 SIMP step has no CPU fallback")
        lib = get_lib()
    return device, lib


def _check_converged(relres, rtol, labels, what="mechanics solve"):
    bad = [labels[i] for i in np.nonzero(~(relres <= rtol))[0]]
    if bad:
        raise PidmError(f"{what} did not converge (||r|| / ||f|| > {rtol:g}) for sample(s) {bad}: raise pcg_max_iter")


FILTERS = {"sensitivity": 0, "density": 1, "heaviside": 2}   # the `filter` argument -> pidm_simp_step (0) / pidm_simp_step_filtered's mode


def _check_filter(who, filter, beta, eta):
    if filter not in FILTERS:
        raise PidmError(f"{who}: unknown filter {filter!r} (one of {', '.join(FILTERS)})")
    if not beta > 0:
        raise PidmError(f"{who}: beta={beta} must be positive")
    if not 0 < eta < 1:
        raise PidmError(f"{who}: eta={eta} must lie in (0, 1)")
    return FILTERS[filter]


def simp_step(x, u, bcs, vf, nel, *, active=None, penal=3., e_min=1e-3, rmin=1.5, move=0.2, n_bisect=60, pcg_rtol=1e-8,
              pcg_max_iter=20000, out=None, lib=None, filter="sensitivity", beta=1., eta=0.5):
    """One `pidm_simp_step`: (x [B,E], u [B,ndof]) fp64 -> dict(x, u, compliance, change, pcg_iters, relres) of new tensors (or the
    ones given in `out`, whose scalar entries of inactive samples are left untouched).
    filter = 'density' / 'heaviside': one `pidm_simp_step_filtered` (density filter; plus the tanh projection at `beta`, `eta`).  x are
    the design variables then, and the dict gains x_phys [B,E], the physical (filtered, projected) density of the new design."""
    if not isinstance(x, torch.Tensor):
        raise PidmError("simp_step: x must be a torch tensor on the device")
    mode = _check_filter("simp_step", filter, beta, eta)
    device, lib = _resolve(x.device, lib)
    st = _mesh(nel, device)
    B = x.shape[0]
    E, ndof = nel * nel, st.neq
    if tuple(x.shape) != (B, E) or tuple(u.shape) != (B, ndof) or tuple(bcs.shape) != (B, 4, nel + 1, nel + 1) or tuple(vf.shape) != (B,):
        raise PidmError(f"simp_step: x / u / bcs / vf must be [B,{E}] / [B,{ndof}] / [B,4,{nel + 1},{nel + 1}] / [B]")
    if x.dtype != torch.float64 or u.dtype != torch.float64 or bcs.dtype != torch.float32 or vf.dtype != torch.float32:
        raise PidmError("simp_step: x, u are float64 and bcs, vf float32")
    if active is not None and (active.dtype != torch.int32 or tuple(active.shape) != (B,)):
        raise PidmError("simp_step: active must be int32 [B]")
    x, u, bcs, vf = x.contiguous(), u.contiguous(), bcs.contiguous(), vf.contiguous()
    if out is None:
        out = dict(x=torch.empty_like(x), u=torch.empty_like(u), compliance=torch.zeros(B, dtype=torch.float64, device=device),
                   change=torch.zeros(B, dtype=torch.float64, device=device), pcg_iters=torch.zeros(B, dtype=torch.int32, device=device),
                   relres=torch.zeros(B, dtype=torch.float64, device=device))
    ws = out.get("ws")
    if ws is None:
        ws = out["ws"] = torch.empty(lib.pidm_simp_ws_bytes(nel, B), dtype=torch.uint8, device=device)
    head = (ptr(x), ptr(u), ptr(bcs), ptr(vf), ptr(active), ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), ptr(st.dof_elems32), nel,
            float(penal), float(e_min), float(rmin), float(move), int(n_bisect), int(pcg_max_iter), float(pcg_rtol))
    tail = (ptr(out["u"]), ptr(out["compliance"]), ptr(out["change"]), ptr(out["pcg_iters"]), ptr(out["relres"]), ptr(ws), B,
            stream_ptr(device))
    if mode == 0:
        lib.check(lib.pidm_simp_step(*head, ptr(out["x"]), *tail), "pidm_simp_step")
    else:
        if out.get("x_phys") is None:
            out["x_phys"] = torch.empty_like(x)
        lib.check(lib.pidm_simp_step_filtered(*head, mode, float(beta), float(eta), ptr(out["x"]), ptr(out["x_phys"]), *tail),
                  "pidm_simp_step_filtered")
    return out


def simp_optimize(bcs, vf, nel, *, penal=3., e_min=1e-3, rmin=1.5, move=0.2, n_bisect=60, max_iter=100, tol=0.01, pcg_rtol=1e-8,
                  pcg_max_iter=20000, check_every=5, labels=None, device=None, lib=None, filter="sensitivity", beta_max=8., beta_every=25,
                  eta=0.5):
    """SIMP compliance minimisation of a batch: starts from x = vf, u = 0 and calls `pidm_simp_step` until every sample's
    change = max |x_new - x| is below tol, or max_iter.  change is read back only every check_every iterations; samples that are
    done are switched off (`active`) and cost nothing afterwards.  bcs [B,4,nn,nn] float32, vf [B].
    Returns (x [B,E] fp64, u [B,ndof] fp64, compliance history [iterations,B] fp64 (NaN where a sample was already done),
    dict(simp=[B] SIMP iterations per sample, pcg=[iterations,B] CG iterations of every step)), all on the device.
    filter = 'density' / 'heaviside' (`pidm_simp_step_filtered`): the first tensor is the physical density of the last design and
    the design variables are the dict's 'design'.  'heaviside' runs iteration k (from 0) at beta = min(beta_max, 2^(k // beta_every))
    for the whole batch, and change < tol switches a sample off only once beta has reached beta_max.
    Raises PidmError naming the samples whose solve ended above pcg_rtol."""
    if not isinstance(bcs, torch.Tensor):
        bcs = torch.from_numpy(np.asarray(bcs, dtype=np.float32))
    device, lib = _resolve(device if device is not None else bcs.device, lib)
    if max_iter < 1 or check_every < 1:
        raise PidmError("simp_optimize: max_iter and check_every must be >= 1")
    mode = _check_filter("simp_optimize", filter, beta_max, eta)
    if mode == 2 and beta_every < 1:
        raise PidmError("simp_optimize: beta_every must be >= 1")
    st = _mesh(nel, device)
    bcs = bcs.to(device=device, dtype=torch.float32).contiguous()
    B = bcs.shape[0]
    vf = torch.as_tensor(np.asarray(vf, dtype=np.float32) if not isinstance(vf, torch.Tensor) else vf).to(device=device, dtype=torch.float32).reshape(B).contiguous()
    labels = labels or [f"#{i}" for i in range(B)]
    E, ndof = nel * nel, st.neq
    f64 = dict(dtype=torch.float64, device=device)
    x = vf.to(torch.float64).reshape(B, 1).repeat(1, E).contiguous()
    u = torch.zeros(B, ndof, **f64)
    x2, u2 = torch.empty_like(x), torch.empty_like(u)
    # one row per iteration, written by the kernel: nothing is read back between the checks
    comp = torch.full((max_iter, B), float("nan"), **f64)
    relres = torch.zeros(max_iter, B, **f64)
    pcg = torch.zeros(max_iter, B, dtype=torch.int32, device=device)
    change = torch.zeros(B, **f64)
    active = torch.ones(B, dtype=torch.int32, device=device)
    n_simp = np.zeros(B, dtype=np.int64)
    alive = np.ones(B, dtype=bool)
    ws = None
    x_phys = torch.empty_like(x) if mode else None
    beta = float(beta_max)
    done, checked = 0, 0
    for it in range(max_iter):
        out = dict(x=x2, u=u2, compliance=comp[it], change=change, pcg_iters=pcg[it], relres=relres[it], ws=ws)
        if mode:
            out["x_phys"] = x_phys
        if mode == 2:
            beta = min(float(beta_max), 2. ** (it // beta_every))
        simp_step(x, u, bcs, vf, nel, active=active, penal=penal, e_min=e_min, rmin=rmin, move=move, n_bisect=n_bisect,
                  pcg_rtol=pcg_rtol, pcg_max_iter=pcg_max_iter, out=out, lib=lib, filter=filter, beta=beta, eta=eta)
        ws = out["ws"]
        x, x2, u, u2 = x2, x, u2, u
        done = it + 1
        n_simp[alive] += 1
        if done % check_every == 0 or done == max_iter:
            _check_converged(relres[checked:done].max(dim=0).values.cpu().numpy(), pcg_rtol, labels)
            checked = done
            if beta >= beta_max:           # (the continuation is not over before: a design that rests at a lower beta is not done)
                alive &= ~(change.cpu().numpy() < tol)
            if not alive.any():
                break
            active.copy_(torch.from_numpy(alive.astype(np.int32)))
    iters = dict(simp=torch.from_numpy(n_simp).to(device), pcg=pcg[:done])
    if mode:
        iters["design"] = x
        return x_phys, u, comp[:done], iters
    return x, u, comp[:done], iters


def _fe_solve(lib, st, nel, E_field, bcs, rtol, max_iter, labels, what):
    """u [B,ndof] float32 of K_closed(E_field) u = f: `pidm_mech_solve` with linear scaling and no threshold."""
    B, dev = E_field.shape[0], E_field.device
    u = torch.empty(B, st.neq, dtype=torch.float32, device=dev)
    comp = torch.empty(B, dtype=torch.float32, device=dev)
    relres = torch.empty(B, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.pidm_mech_solve_ws_bytes(nel, B), dtype=torch.uint8, device=dev)
    lib.check(lib.pidm_mech_solve(ptr(E_field), ptr(bcs), ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), ptr(st.dof_elems32), nel,
                                  -1.0, 1.0, E_VOID, int(max_iter), float(rtol), ptr(u), ptr(comp), None, None, ptr(relres), ptr(ws), B,
                                  stream_ptr(dev)), "pidm_mech_solve")
    _check_converged(relres.double().cpu().numpy(), float(np.float32(rtol)), labels, what)
    return u


def mech_fields(u_dofs, rho, nel, lib=None):
    """[B,2,nn,nn] float32 (strain energy density, von Mises stress) of the state u_dofs [B,ndof] float32 with moduli rho [B,E]
    float32 (`pidm_mech_fields`)."""
    if not isinstance(u_dofs, torch.Tensor):
        raise PidmError("mech_fields: u_dofs must be a torch tensor on the device")
    device, lib = _resolve(u_dofs.device, lib)
    st = _mesh(nel, device)
    B = u_dofs.shape[0]
    if tuple(u_dofs.shape) != (B, st.neq) or tuple(rho.shape) != (B, nel * nel) or u_dofs.dtype != torch.float32 or rho.dtype != torch.float32:
        raise PidmError(f"mech_fields: u_dofs / rho must be float32 [B,{st.neq}] / [B,{nel * nel}]")
    out = torch.empty(B, 2, nel + 1, nel + 1, dtype=torch.float32, device=device)
    lib.check(lib.pidm_mech_fields(ptr(u_dofs.contiguous()), ptr(rho.contiguous()), ptr(st.kloc_dev), st.kloc_stride, ptr(st.elem_dofs32), nel,
                                   NU, ptr(out), B, stream_ptr(device)), "pidm_mech_fields")
    return out


def _binarize(x, vf, how):
    """E_field [B,E] float32 of the density x [B,E]: True / 'threshold' cuts at 0.5, 'volume' keeps the round(vf E) densest elements of
    every sample (ties go to the lower element index), False stores clip(x, E_VOID, 1)."""
    if how is False:
        return x.clamp(E_VOID, 1.0).float().contiguous()
    if how is True or how == "threshold":
        return torch.where(x > 0.5, 1.0, E_VOID).float().contiguous()
    E = x.shape[1]
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    k = torch.round(vf.double() * E).long().view(-1, 1)
    solid = torch.zeros_like(x, dtype=torch.bool).scatter_(1, order, torch.arange(E, device=x.device).view(1, E) < k)
    return torch.where(solid, 1.0, E_VOID).float().contiguous()


def generate_mechanics_batch(seeds, nel=64, binarize=True, n_loads=1, final_rtol=FINAL_RTOL, return_info=False, device=None, lib=None,
                             filter="sensitivity", **simp):
    """Samples for the given seeds, [B,10,nn,nn] float32 on the device in the reference's channel order: vf (constant image),
    strain energy density and von Mises stress of the uniform domain E = 1 under the sample's supports and loads, disp_x, disp_y,
    E_field (zero-padded to nn: last row and column 0), BC_node_x, BC_node_y, load_x, load_y.  E_field = where(x > 0.5, 1, 1e-3)
    of the SIMP result (clip(x, 1e-3, 1) without `binarize`); the displacements are the FE solution of exactly that field under
    the training operator.  binarize = 'volume': E_field is 1 on the round(vf E) elements of largest density instead, so that its solid
    fraction is vf to half an element.  `filter` and `simp`: keyword arguments of simp_optimize; with filter = 'density' / 'heaviside'
    x is the physical density, which return_info's dict then holds as 'x_phys' ([B,E] fp64; the design variables are iters['design'])."""
    if not (isinstance(binarize, bool) or binarize in ("threshold", "volume")):
        raise PidmError(f"generate_mechanics_batch: binarize={binarize!r} must be True, False, 'threshold' or 'volume'")
    _check_filter("generate_mechanics_batch", filter, simp.get("beta_max", 8.), simp.get("eta", 0.5))
    device, lib = _resolve(device, lib)
    seeds = [int(s) for s in seeds]
    B, nn = len(seeds), nel + 1
    if B == 0:
        return torch.zeros(0, 10, nn, nn, dtype=torch.float32, device=device)
    labels = [f"#{i} (seed {s})" for i, s in enumerate(seeds)]
    probs = [sample_problem(s, nel, n_loads) for s in seeds]
    bcs = torch.from_numpy(np.stack([p[0] for p in probs])).to(device)
    vf = torch.tensor([p[1] for p in probs], dtype=torch.float32, device=device)
    x, _, comp, iters = simp_optimize(bcs, vf, nel, labels=labels, device=device, lib=lib, filter=filter, **simp)
    E_field = _binarize(x, vf, binarize)
    st = _mesh(nel, device)
    max_iter = simp.get("pcg_max_iter", 20000)
    u = _fe_solve(lib, st, nel, E_field, bcs, final_rtol, max_iter, labels, "final mechanics solve")
    ones = torch.ones_like(E_field)
    u_uni = _fe_solve(lib, st, nel, ones, bcs, final_rtol, max_iter, labels, "uniform-domain mechanics solve")
    out = torch.zeros(B, 10, nn, nn, dtype=torch.float32, device=device)
    out[:, 0] = vf.view(B, 1, 1)
    out[:, 1:3] = mech_fields(u_uni, ones, nel, lib=lib)
    out[:, 3:5] = u.view(B, nn, nn, 2).permute(0, 3, 1, 2)
    out[:, 5, :nel, :nel] = E_field.view(B, nel, nel)
    out[:, 6:10] = bcs
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    info = dict(compliance=comp, iters=iters)
    if filter != "sensitivity":
        info["x_phys"] = x
    return (out, info) if return_info else out


def generate_mechanics_dataset(n_samples, out_dir, seed=None, seeds=None, batch=256, nel=64, n_loads=1, binarize=True, device=None,
                               lib=None, verbose=False, filter="sensitivity", **simp):
    """Writes out_dir/<i>.npy, i = 0 .. n_samples-1, each [nn,nn,10] float32 - what `Dataset_Paths` reads (it transposes to
    [10,nn,nn] and sorts by the integer name).  `seeds` (explicit, must be distinct) or `seed` (draws n_samples distinct seeds
    reproducibly); neither: fresh ones.  `binarize`, `filter` and `simp` as in generate_mechanics_batch.  Returns the seeds."""
    if seeds is None:
        seeds = _unique_seeds(n_samples, seed)
    seeds = [int(s) for s in seeds]
    if len(seeds) != n_samples:
        raise PidmError(f"generate_mechanics_dataset: {len(seeds)} seeds for {n_samples} samples")
    if len(set(seeds)) != len(seeds):
        dup = sorted({s for s in seeds if seeds.count(s) > 1})
        raise PidmError(f"Seeds are not unique: {dup}")
    if batch < 1:
        raise PidmError("generate_mechanics_dataset: batch must be >= 1")
    device, lib = _resolve(device, lib)
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    for lo in range(0, n_samples, batch):
        data, info = generate_mechanics_batch(seeds[lo:lo + batch], nel, binarize, n_loads, return_info=True, device=device, lib=lib,
                                              filter=filter, **simp)
        arr = data.permute(0, 2, 3, 1).contiguous().cpu().numpy()
        for k in range(arr.shape[0]):
            np.save(os.path.join(out_dir, f"{lo + k}.npy"), arr[k])
        if verbose:
            ns = info["iters"]["simp"].cpu().numpy()
            print(f"samples {lo}..{lo + len(ns) - 1}: SIMP iterations {ns.min()}..{ns.max()}, {time.time() - t0:.1f} s", flush=True)
    return seeds


def main(argv=None):
    ap = argparse.ArgumentParser(description="Mechanics (topology-optimisation) training data on the MI355X")
    ap.add_argument("--n-samples", type=int, default=10)
    ap.add_argument("--out", default="./data/mechanics/train/fields")
    ap.add_argument("--nel", type=int, default=64)
    ap.add_argument("--n-loads", type=int, default=1, help="point loads per sample (2: the harder test level)")
    ap.add_argument("--seed", type=int, default=None, help="draw the sample seeds reproducibly (default: fresh per run)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--max-iter", type=int, default=100, help="SIMP iterations at most")
    ap.add_argument("--no-binarize", action="store_true", help="store clip(x, 1e-3, 1) instead of the 0.5-thresholded field")
    ap.add_argument("--filter", choices=sorted(FILTERS, key=FILTERS.get), default="sensitivity",
                    help="sensitivity filter (default), density filter, or density filter + tanh projection with beta continuation")
    ap.add_argument("--beta-max", type=float, default=8., help="heaviside: the projection's beta doubles from 1 up to this")
    ap.add_argument("--beta-every", type=int, default=25, help="heaviside: SIMP iterations per beta")
    ap.add_argument("--binarize", choices=["threshold", "volume"], default="threshold",
                    help="threshold: cut at 0.5; volume: keep the round(vf E) densest elements (solid fraction = vf)")
    a = ap.parse_args(argv)
    t0 = time.time()
    extra = dict(beta_max=a.beta_max, beta_every=a.beta_every) if a.filter == "heaviside" else {}
    generate_mechanics_dataset(a.n_samples, a.out, seed=a.seed, batch=a.batch, nel=a.nel, n_loads=a.n_loads,
                               binarize=False if a.no_binarize else (True if a.binarize == "threshold" else a.binarize),
                               max_iter=a.max_iter, verbose=True, filter=a.filter, **extra)
    print(f"Data generation finished: {a.n_samples} samples in {time.time() - t0:.1f} s -> {a.out}")


if __name__ == "__main__":
    main()
