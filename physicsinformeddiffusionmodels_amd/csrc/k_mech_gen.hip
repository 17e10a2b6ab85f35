// Mechanics training-data generation for gfx950: one SIMP (solid isotropic material with penalisation) compliance-minimisation
// step for a whole batch per launch, and the nodal conditioning fields of a solved state.
//
// Replaces nothing in the reference: it never generated the topology-optimisation samples it trains on, they were downloaded.
// This supplies the data main.py:90-101 expects (one [65,65,10] .npy per sample; channel order src/data_utils.py:118), on the
// mesh and element stiffness of k_mech.hip, so that the stored displacements solve the TRAINING operator K_closed(E) u = f.
//
// simp_step_kernel, one workgroup per sample, everything in fp64, reductions in a fixed order (no atomics):
//   1. E_e = e_min + x_e^penal (1 - e_min)
//   2. K_closed(E) u = f by Jacobi-preconditioned CG on the matrix-free operator of mech_pcg_kernel (pinned dofs are identity
//      rows with f = 0), warm-started from the caller's u; stops at ||r|| <= rtol ||f|| (the initial residual included) or max_iter
//   3. ce_e = u_e^T k_e u_e,  c = sum E_e ce_e,  dc_e = -penal x_e^(penal-1) (1 - e_min) max(ce_e, 0)
//   4. sensitivity filter  dc~_e = sum_j H_ej x_j dc_j / (max(1e-3, x_e) sum_j H_ej),  H_ej = max(0, rmin - dist(e, j))
//   5. optimality criteria: n_bisect bisection steps on lambda in [0, 1e9] (fixed count, no tolerance exit)
//      x_new = max(0, max(x - move, min(1, min(x + move, x sqrt(-dc~ / lambda))))),  mean(x_new) > vf => l1 = lambda else l2 = lambda
// One launch is one SIMP iteration (a launch stays bounded by max_iter CG iterations); the host loop lives in
// mechanics_data_generation.py.
//
// LDS (doubles): P[ndof] | E[E].  P holds the CG search direction, then u for phase 3; from phase 4 on the same bytes hold
// x[E] | dc~[E] (2 E <= ndof) while the E region holds x dc, so the filter and the n_bisect passes never leave the chip.
// The lane's part of the iterate, of the residual and of 1/diag stay in registers during the CG loop (dof tid + k 512); A p goes
// through the workspace (2 ndof doubles per sample, each element touched by one lane only).  100 KB of LDS at nel = 64.
#include <math.h>

#include "pidm_common.h"

namespace pidm {

constexpr int SG_THREADS = 512;   // 8 waves: two per SIMD
constexpr int SG_WAVES = SG_THREADS / 64;

struct GenMesh {
  const int* elem_dofs;   // [E][8]
  const int* dof_elems;   // [ndof][4][2] = (element, local index) or (-1, -1)
  const float* kloc;      // [E][8][8] or [1][8][8] when kloc_stride == 0
  int kloc_stride;
  int E, ndof, nel, nn;
};

struct SimpPar {
  double penal, e_min, rmin, move, rtol;
  int n_bisect, max_iter;
};

__device__ __forceinline__ double sg_sum(double v, double* red) {   // all SG_THREADS lanes; result broadcast
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < SG_WAVES; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ void sg_sum2(double& a, double& b, double* red) {   // two sums behind one pair of barriers
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off);
    b += __shfl_xor(b, off);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = a;
    red[SG_WAVES + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  double sa = 0.0, sb = 0.0;
#pragma unroll
  for (int w = 0; w < SG_WAVES; ++w) {
    sa += red[w];
    sb += red[SG_WAVES + w];
  }
  a = sa;
  b = sb;
}

__device__ __forceinline__ double sg_max(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < SG_WAVES; ++w) s = fmax(s, red[w]);
  return s;
}

__device__ __forceinline__ double oc_update(double x, double dcf, double lam, double move) {
  return fmax(0.0, fmax(x - move, fmin(1.0, fmin(x + move, x * sqrt(-dcf / lam)))));
}

// sum_q k[a][q] P[D[q]] for one (element, local row): a row of k_e and an element's dof list are 32-byte rows, fetched as two
// 16-byte loads each (the per-lane addresses are scattered: the number of load instructions, not their bytes, sets the pace)
__device__ __forceinline__ double row_dot(const float* krow, const int* D, const double* P) {
  const float4 k0 = *reinterpret_cast<const float4*>(krow), k1 = *reinterpret_cast<const float4*>(krow + 4);
  const int4 d0 = *reinterpret_cast<const int4*>(D), d1 = *reinterpret_cast<const int4*>(D + 4);
  double acc = 0.0;
  acc += (double)k0.x * P[d0.x];
  acc += (double)k0.y * P[d0.y];
  acc += (double)k0.z * P[d0.z];
  acc += (double)k0.w * P[d0.w];
  acc += (double)k1.x * P[d1.x];
  acc += (double)k1.y * P[d1.y];
  acc += (double)k1.z * P[d1.z];
  acc += (double)k1.w * P[d1.w];
  return acc;
}

// u_e^T k_e u_e of element e for the nodal vector U (LDS or registers behind a pointer)
__device__ __forceinline__ double elem_energy(const GenMesh& ms, int e, const double* ue) {
  const float* k = ms.kloc + (size_t)e * ms.kloc_stride;
  double ce = 0.0;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) t += (double)k[a * 8 + q] * ue[q];
    ce += ue[a] * t;
  }
  return ce;
}

// The solve of K_closed(E) u = f shared by simp_step_kernel and simp_step_filtered_kernel: the warm start ub (zero on pinned dofs)
// -> sP, then Jacobi-preconditioned CG on the matrix-free operator with the moduli in sE (written by the caller, published by the
// first barrier here).  On return u is in X (global) and in sP, behind a barrier; it / relres are the CG's exit state.
template <int PTS>   // dofs per lane: PTS * SG_THREADS >= ndof
__device__ __forceinline__ void simp_solve(const GenMesh& ms, const float* bb, const double* ub, const SimpPar& sp, double* sP,
                                           const double* sE, double* AP, double* T, double* red, double* X, int& it_out,
                                           double& relres_out) {
  const int tid = threadIdx.x, nn = ms.nn, ndof = ms.ndof;
  for (int i = tid; i < ndof; i += SG_THREADS) {
    const bool masked = bb[(size_t)(i & 1) * nn * nn + (i >> 1)] != 0.f;
    sP[i] = masked ? 0.0 : ub[i];
  }
  __syncthreads();

  // r = f - K_closed u, Minv = 1 / diag, then PCG
  double rz = 0.0, rr = 0.0, ff_l = 0.0;
  for (int i = tid; i < ndof; i += SG_THREADS) {
    const int node = i >> 1, d = i & 1;
    const bool masked = bb[(size_t)d * nn * nn + node] != 0.f;
    double diag = 0.0, ku = 0.0;
    for (int s = 0; s < 4; ++s) {
      const int2 ea = *reinterpret_cast<const int2*>(ms.dof_elems + (i * 4 + s) * 2);
      const int e = ea.x, a = ea.y;
      if (e < 0) continue;
      const float* k = ms.kloc + (size_t)e * ms.kloc_stride + a * 8;
      ku += sE[e] * row_dot(k, ms.elem_dofs + (size_t)e * 8, sP);
      diag += sE[e] * (double)k[a];
    }
    const double f = masked ? 0.0 : (double)bb[(size_t)(2 + d) * nn * nn + node];
    const double mi = masked ? 1.0 : 1.0 / diag;
    const double r = masked ? 0.0 : f - ku;
    AP[i] = r;
    T[i] = mi;
    rz += r * mi * r;
    rr += r * r;
    ff_l += f * f;
  }
  sg_sum2(rz, rr, red);
  const double r0 = sqrt(sg_sum(ff_l, red));   // (every read of the warm start in sP is behind these barriers)
  // the lane's part of the iterate, the residual and the preconditioner stay in registers from here on (dof tid + u SG_THREADS)
  double rX[PTS], rR[PTS], rMI[PTS];
#pragma unroll
  for (int u = 0; u < PTS; ++u) {
    const int i = tid + u * SG_THREADS;
    const bool in = i < ndof;
    rX[u] = in ? sP[i] : 0.0;
    rR[u] = in ? AP[i] : 0.0;
    rMI[u] = in ? T[i] : 0.0;
    if (in) sP[i] = rMI[u] * rR[u];
  }
  __syncthreads();
  double relres = r0 > 0.0 ? sqrt(rr) / r0 : 0.0;
  int it = 0;
  while (it < sp.max_iter && relres > sp.rtol) {
    double pap_l = 0.0;
    for (int i = tid; i < ndof; i += SG_THREADS) {
      const int node = i >> 1, d = i & 1;
      const bool masked = bb[(size_t)d * nn * nn + node] != 0.f;
      double ku = 0.0;
      if (!masked) {
        for (int s = 0; s < 4; ++s) {
          const int2 ea = *reinterpret_cast<const int2*>(ms.dof_elems + (i * 4 + s) * 2);
          if (ea.x < 0) continue;
          ku += sE[ea.x] * row_dot(ms.kloc + (size_t)ea.x * ms.kloc_stride + ea.y * 8, ms.elem_dofs + (size_t)ea.x * 8, sP);
        }
      } else {
        ku = sP[i];
      }
      AP[i] = ku;
      pap_l += sP[i] * ku;
    }
    const double pap = sg_sum(pap_l, red);
    const double alpha = rz / pap;
    double rz_n = 0.0, rr_n = 0.0;
#pragma unroll
    for (int u = 0; u < PTS; ++u) {
      const int i = tid + u * SG_THREADS;
      if (i < ndof) {
        rX[u] += alpha * sP[i];
        const double r = rR[u] - alpha * AP[i];
        rR[u] = r;
        rz_n += r * rMI[u] * r;
        rr_n += r * r;
      }
    }
    sg_sum2(rz_n, rr_n, red);
    rr = rr_n;
    relres = sqrt(rr) / r0;
    ++it;
    if (!(relres > sp.rtol)) break;
    const double beta = rz_n / rz;
    rz = rz_n;
#pragma unroll
    for (int u = 0; u < PTS; ++u) {
      const int i = tid + u * SG_THREADS;
      if (i < ndof) sP[i] = rMI[u] * rR[u] + beta * sP[i];
    }
    __syncthreads();
  }

  // u -> output and LDS
  // (the last reads of other lanes' sP entries are behind the barriers of the reductions above)
#pragma unroll
  for (int u = 0; u < PTS; ++u) {
    const int i = tid + u * SG_THREADS;
    if (i < ndof) {
      X[i] = rX[u];
      sP[i] = rX[u];
    }
  }
  __syncthreads();
  it_out = it;
  relres_out = relres;
}

template <int PTS>   // dofs per lane: PTS * SG_THREADS >= ndof
__global__ void __launch_bounds__(SG_THREADS) simp_step_kernel(GenMesh ms, const double* __restrict__ x_in,   // [B][E]
                                                               const double* __restrict__ u_in,               // [B][ndof]
                                                               const float* __restrict__ bcs,                 // [B][4][nn][nn]
                                                               const float* __restrict__ vf,                  // [B]
                                                               const int* __restrict__ active,                // [B] or null
                                                               SimpPar sp, double* __restrict__ ws,           // [B][2][ndof]
                                                               double* __restrict__ x_out, double* __restrict__ u_out,
                                                               double* __restrict__ comp_out, double* __restrict__ change_out,
                                                               int* __restrict__ iters_out, double* __restrict__ relres_out) {
  HIP_DYNAMIC_SHARED(double, smem)
  __shared__ double red[2 * SG_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nel = ms.nel, nn = ms.nn, E = ms.E, ndof = ms.ndof;
  const double* xb = x_in + (size_t)b * E;
  const double* ub = u_in + (size_t)b * ndof;
  double* xo = x_out + (size_t)b * E;
  double* X = u_out + (size_t)b * ndof;
  if (active && active[b] == 0) {   // a finished sample: passed through, its scalar outputs are left as they are
    for (int e = tid; e < E; e += SG_THREADS) xo[e] = xb[e];
    for (int i = tid; i < ndof; i += SG_THREADS) X[i] = ub[i];
    return;
  }
  double* sP = smem;
  double* sE = smem + ndof;
  double* AP = ws + (size_t)b * 2 * ndof;
  double* T = AP + ndof;
  const float* bb = bcs + (size_t)b * 4 * nn * nn;

  // ---- 1: Young's moduli; the warm start (zero on pinned dofs) -> LDS ----
  for (int e = tid; e < E; e += SG_THREADS) sE[e] = sp.e_min + pow(xb[e], sp.penal) * (1.0 - sp.e_min);

  // ---- 2: K_closed(E) u = f; u -> output and LDS ----
  int it;
  double relres;
  simp_solve<PTS>(ms, bb, ub, sp, sP, sE, AP, T, red, X, it, relres);

  // ---- 3: element energies, compliance, sensitivities (x dc replaces E in LDS) ----
  double c_l = 0.0;
  for (int e = tid; e < E; e += SG_THREADS) {
    const int* D = ms.elem_dofs + (size_t)e * 8;
    double ue[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) ue[q] = sP[D[q]];
    const double ce = elem_energy(ms, e, ue);
    const double xe = xb[e];
    c_l += sE[e] * ce;
    // (k_e is stored in fp32 and therefore indefinite by ~6e-8 |k_e|: an element that moves almost rigidly can show ce < 0, which
    //  would make dc~ positive and the update's square root undefined; such an element has no sensitivity)
    const double dc = -sp.penal * pow(xe, sp.penal - 1.0) * (1.0 - sp.e_min) * fmax(ce, 0.0);
    sE[e] = xe * dc;
  }
  const double comp = sg_sum(c_l, red);   // (publishes x dc, retires every read of u)

  // ---- 4: sensitivity filter; x | dc~ take the place of u ----
  double* sX = smem;
  double* sD = smem + E;
  const int win = (int)ceil(sp.rmin) - 1;
  for (int e = tid; e < E; e += SG_THREADS) {
    const int ey = e / nel, ex = e - ey * nel;
    double num = 0.0, den = 0.0;
    for (int dy = -win; dy <= win; ++dy) {
      const int yy = ey + dy;
      if (yy < 0 || yy >= nel) continue;
      for (int dx = -win; dx <= win; ++dx) {
        const int xx = ex + dx;
        if (xx < 0 || xx >= nel) continue;
        const double h = sp.rmin - sqrt((double)(dy * dy + dx * dx));
        if (h > 0.0) {
          num += h * sE[yy * nel + xx];
          den += h;
        }
      }
    }
    const double xe = xb[e];
    sX[e] = xe;
    sD[e] = num / (fmax(1e-3, xe) * den);
  }
  // (each lane reads back only the sX / sD entries it wrote: no barrier needed before the passes below)

  // ---- 5: optimality criteria, n_bisect bisection steps ----
  const double vfb = (double)vf[b];
  double l1 = 0.0, l2 = 1e9, lmid = 0.0;
  for (int s = 0; s < sp.n_bisect; ++s) {
    lmid = 0.5 * (l1 + l2);
    double sum_l = 0.0;
    for (int e = tid; e < E; e += SG_THREADS) sum_l += oc_update(sX[e], sD[e], lmid, sp.move);
    const double mean = sg_sum(sum_l, red) / (double)E;
    if (mean > vfb) l1 = lmid;
    else l2 = lmid;
  }
  double chg_l = 0.0;
  for (int e = tid; e < E; e += SG_THREADS) {
    const double xn = oc_update(sX[e], sD[e], lmid, sp.move);
    xo[e] = xn;
    chg_l = fmax(chg_l, fabs(xn - sX[e]));
  }
  const double chg = sg_max(chg_l, red);
  if (tid == 0) {
    comp_out[b] = comp;
    change_out[b] = chg;
    iters_out[b] = it;
    relres_out[b] = relres;
  }
}

// ---- the three-field variant: design x -> density filter x~ = (H x) / Hs -> projection x^ (pidm_simp_step_filtered) ----
//
// simp_step_filtered_kernel, launched like simp_step_kernel (one workgroup per sample, fp64, fixed-order reductions):
//   1. x~ = (H x) / Hs,  x^ = x~ (mode 1) or (tanh(b h) + tanh(b (x~ - h))) / (tanh(b h) + tanh(b (1 - h))) (mode 2; b = beta, h = eta),
//      d = dx^/dx~ = 1 or b (1 - tanh^2(b (x~ - h))) / (tanh(b h) + tanh(b (1 - h))),  E_e = e_min + x^_e^penal (1 - e_min)
//   2. K_closed(E) u = f: simp_solve, the CG phase of simp_step_kernel
//   3. ce_e = u_e^T k_e u_e,  c = sum E_e ce_e,  g_e = -penal x^_e^(penal-1) (1 - e_min) max(ce_e, 0)
//   4. the chain rule through the projection and the (symmetric) filter: dc_e = sum_j H_ej g_j d_j / Hs_j,  dv_e = sum_j H_ej d_j / Hs_j
//   5. n_bisect bisection steps on lambda in [0, 1e9]: x_new = oc_update(x, dc / dv, lambda), mean(x^(x~(x_new))) > vf => l1 = lambda
//      else l2 = lambda: every step stages x_new in LDS, applies the window and the projection, and reduces
//   6. x_new, x^(x~(x_new)), u, c, max |x_new - x|
// H_ej = max(0, rmin - dist(e, j)) over the window of simp_step_kernel; Hs_e is recomputed from the window wherever it is needed.
//
// LDS: the layout of simp_step_kernel, P[ndof] | E[E], with three E-sized arrays in it (2 E <= ndof):
//   phase 1   E: x, then the moduli            P[0:E): x^
//   phase 3   E: g d / Hs (in place of the moduli)          P: u       d / Hs goes through the workspace (lane-private entries)
//   phase 4   E: g d / Hs    P[0:E): d / Hs    P[E:2E): dc / dv
//   phase 5   E: x           P[0:E): the trial x_new        P[E:2E): dc / dv
struct ProjPar {
  int mode;           // 1: density filter, 2: density filter + projection
  double beta, eta;
  double tb, den;     // tanh(beta eta), tanh(beta eta) + tanh(beta (1 - eta))
};

// distance of the window offset (dy, dx), the same for every lane: the centre and its four neighbours (all the taps but the corners
// at the default rmin = 1.5) need no square root, and 0 and 1 are what sqrt gives for them
__device__ __forceinline__ double tap_dist(int dy, int dx) {
  const int r2 = dy * dy + dx * dx;
  return r2 <= 1 ? (double)r2 : sqrt((double)r2);
}

// sum_j H_ej v_j of element e over the clipped window (v in LDS or global memory); den = Hs_e
__device__ __forceinline__ double win_sum(const double* v, int e, int nel, int win, double rmin, double& den) {
  const int ey = e / nel, ex = e - ey * nel;
  double num = 0.0;
  den = 0.0;
  for (int dy = -win; dy <= win; ++dy) {
    const int yy = ey + dy;
    if (yy < 0 || yy >= nel) continue;
    for (int dx = -win; dx <= win; ++dx) {
      const int xx = ex + dx;
      if (xx < 0 || xx >= nel) continue;
      const double h = rmin - tap_dist(dy, dx);
      if (h > 0.0) {
        num += h * v[yy * nel + xx];
        den += h;
      }
    }
  }
  return num;
}

__device__ __forceinline__ double project(const ProjPar& pj, double xt) {
  return pj.mode == 2 ? (pj.tb + tanh(pj.beta * (xt - pj.eta))) / pj.den : xt;
}

// dx^/dx~; 1 - tanh^2 is taken as 1 / cosh^2, which does not cancel where the projection saturates
__device__ __forceinline__ double project_slope(const ProjPar& pj, double xt) {
  if (pj.mode != 2) return 1.0;
  const double ch = cosh(pj.beta * (xt - pj.eta));
  return pj.beta / (ch * ch * pj.den);
}

template <int PTS>
__global__ void __launch_bounds__(SG_THREADS) simp_step_filtered_kernel(GenMesh ms, const double* __restrict__ x_in,   // [B][E]
                                                                        const double* __restrict__ u_in,               // [B][ndof]
                                                                        const float* __restrict__ bcs, const float* __restrict__ vf,
                                                                        const int* __restrict__ active, SimpPar sp, ProjPar pj,
                                                                        double* __restrict__ ws,                       // [B][2][ndof]
                                                                        double* __restrict__ x_out, double* __restrict__ xphys_out,
                                                                        double* __restrict__ u_out, double* __restrict__ comp_out,
                                                                        double* __restrict__ change_out, int* __restrict__ iters_out,
                                                                        double* __restrict__ relres_out) {
  HIP_DYNAMIC_SHARED(double, smem)
  __shared__ double red[2 * SG_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nel = ms.nel, nn = ms.nn, E = ms.E, ndof = ms.ndof;
  const double* xb = x_in + (size_t)b * E;
  const double* ub = u_in + (size_t)b * ndof;
  double* xo = x_out + (size_t)b * E;
  double* xpo = xphys_out + (size_t)b * E;
  double* X = u_out + (size_t)b * ndof;
  const int win = (int)ceil(sp.rmin) - 1;
  if (active && active[b] == 0) {   // a finished sample: passed through with the physical density of its design at this beta
    for (int e = tid; e < E; e += SG_THREADS) {
      double hs;
      const double num = win_sum(xb, e, nel, win, sp.rmin, hs);
      xo[e] = xb[e];
      xpo[e] = project(pj, num / hs);
    }
    for (int i = tid; i < ndof; i += SG_THREADS) X[i] = ub[i];
    return;
  }
  double* sP = smem;
  double* sE = smem + ndof;
  double* sR = smem + E;
  double* AP = ws + (size_t)b * 2 * ndof;
  double* T = AP + ndof;
  const float* bb = bcs + (size_t)b * 4 * nn * nn;

  // ---- 1: x -> LDS, x^ = project(filter(x)), Young's moduli ----
  for (int e = tid; e < E; e += SG_THREADS) sE[e] = xb[e];
  __syncthreads();
  for (int e = tid; e < E; e += SG_THREADS) {
    double hs;
    const double num = win_sum(sE, e, nel, win, sp.rmin, hs);
    sP[e] = project(pj, num / hs);
  }
  __syncthreads();   // (every window read of x is done: the moduli may replace it)
  // (a lane reads back the sP entries it wrote, and simp_solve's warm start overwrites sP at the same lane's indices tid + k 512)
  for (int e = tid; e < E; e += SG_THREADS) sE[e] = sp.e_min + pow(sP[e], sp.penal) * (1.0 - sp.e_min);

  // ---- 2: K_closed(E) u = f; u -> output and LDS ----
  int it;
  double relres;
  simp_solve<PTS>(ms, bb, ub, sp, sP, sE, AP, T, red, X, it, relres);

  // ---- 3: element energies, compliance; g d / Hs replaces E in LDS, d / Hs -> workspace (the CG is done with it) ----
  double c_l = 0.0;
  for (int e = tid; e < E; e += SG_THREADS) {
    const int* D = ms.elem_dofs + (size_t)e * 8;
    double ue[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) ue[q] = sP[D[q]];
    const double ce = elem_energy(ms, e, ue);
    double hs;
    const double xt = win_sum(xb, e, nel, win, sp.rmin, hs) / hs;   // (the same sum in the same order as in phase 1)
    const double xp = project(pj, xt);
    const double dh = project_slope(pj, xt) / hs;
    c_l += sE[e] * ce;
    // (max(ce, 0): see simp_step_kernel)
    sE[e] = -sp.penal * pow(xp, sp.penal - 1.0) * (1.0 - sp.e_min) * fmax(ce, 0.0) * dh;
    T[e] = dh;
  }
  const double comp = sg_sum(c_l, red);   // (publishes g d / Hs, retires every read of u)
  for (int e = tid; e < E; e += SG_THREADS) sP[e] = T[e];   // (written by this lane)
  __syncthreads();

  // ---- 4: the filter's transpose (H is symmetric): dc / dv -> P[E:2E) ----
  for (int e = tid; e < E; e += SG_THREADS) {
    const int ey = e / nel, ex = e - ey * nel;
    double dc = 0.0, dv = 0.0;
    for (int dy = -win; dy <= win; ++dy) {
      const int yy = ey + dy;
      if (yy < 0 || yy >= nel) continue;
      for (int dx = -win; dx <= win; ++dx) {
        const int xx = ex + dx;
        if (xx < 0 || xx >= nel) continue;
        const double h = sp.rmin - tap_dist(dy, dx);
        if (h > 0.0) {
          dc += h * sE[yy * nel + xx];
          dv += h * sP[yy * nel + xx];
        }
      }
    }
    sR[e] = dc / dv;
  }
  __syncthreads();   // (every window read is done: x takes the moduli region, the trial design P[0:E))
  for (int e = tid; e < E; e += SG_THREADS) sE[e] = xb[e];
  // (each lane reads back only the sE / sR entries it wrote)

  // ---- 5: optimality criteria, n_bisect bisection steps with the volume of the physical density ----
  const double vfb = (double)vf[b];
  double l1 = 0.0, l2 = 1e9;
  for (int s = 0; s < sp.n_bisect; ++s) {
    const double lmid = 0.5 * (l1 + l2);
    for (int e = tid; e < E; e += SG_THREADS) sP[e] = oc_update(sE[e], sR[e], lmid, sp.move);
    __syncthreads();
    double sum_l = 0.0;
    for (int e = tid; e < E; e += SG_THREADS) {
      double hs;
      const double num = win_sum(sP, e, nel, win, sp.rmin, hs);
      sum_l += project(pj, num / hs);
    }
    const double mean = sg_sum(sum_l, red) / (double)E;   // (its barriers retire the window reads before the next trial is staged)
    if (mean > vfb) l1 = lmid;
    else l2 = lmid;
  }

  // ---- 6: the last trial is the result ----
  double chg_l = 0.0;
  for (int e = tid; e < E; e += SG_THREADS) {
    double hs;
    const double num = win_sum(sP, e, nel, win, sp.rmin, hs);
    const double xn = sP[e];
    xo[e] = xn;
    xpo[e] = project(pj, num / hs);
    chg_l = fmax(chg_l, fabs(xn - sE[e]));
  }
  const double chg = sg_max(chg_l, red);
  if (tid == 0) {
    comp_out[b] = comp;
    change_out[b] = chg;
    iters_out[b] = it;
    relres_out[b] = relres;
  }
}

// Strain energy density and von Mises stress at the element centres (unit-square elements, local nodes [bl, br, tr, tl] as
// synthetic_mesh numbers them: B(0,0) has dN/dx = (-1, 1, 1, -1) / 2, dN/dy = (-1, -1, 1, 1) / 2), averaged to the nodes.
// LDS: W[E] | V[E] doubles.
__global__ void __launch_bounds__(256) mech_fields_kernel(GenMesh ms, const float* __restrict__ u,     // [B][ndof]
                                                          const float* __restrict__ rho,               // [B][E]
                                                          double nu, float* __restrict__ out) {        // [B][2][nn][nn]
  HIP_DYNAMIC_SHARED(double, smem)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nel = ms.nel, nn = ms.nn, E = ms.E, ndof = ms.ndof;
  double* sW = smem;
  double* sV = smem + E;
  const float* ub = u + (size_t)b * ndof;
  for (int e = tid; e < E; e += 256) {
    const int* D = ms.elem_dofs + (size_t)e * 8;
    double ue[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) ue[q] = (double)ub[D[q]];
    const double Ee = (double)rho[(size_t)b * E + e];
    sW[e] = 0.5 * Ee * elem_energy(ms, e, ue);   // element area 1
    const double ex = 0.5 * (-ue[0] + ue[2] + ue[4] - ue[6]);
    const double ey = 0.5 * (-ue[1] - ue[3] + ue[5] + ue[7]);
    const double gxy = 0.5 * (-ue[0] - ue[2] + ue[4] + ue[6]) + 0.5 * (-ue[1] + ue[3] + ue[5] - ue[7]);
    const double cf = Ee / (1.0 - nu * nu);
    const double sx = cf * (ex + nu * ey), sy = cf * (nu * ex + ey), txy = cf * 0.5 * (1.0 - nu) * gxy;
    sV[e] = sqrt(sx * sx - sx * sy + sy * sy + 3.0 * txy * txy);
  }
  __syncthreads();
  for (int node = tid; node < nn * nn; node += 256) {
    const int r = node / nn, c = node - r * nn;
    double w = 0.0, v = 0.0;
    int cnt = 0;
    for (int er = r - 1; er <= r; ++er) {
      if (er < 0 || er >= nel) continue;
      for (int ec = c - 1; ec <= c; ++ec) {
        if (ec < 0 || ec >= nel) continue;
        w += sW[er * nel + ec];
        v += sV[er * nel + ec];
        ++cnt;
      }
    }
    out[((size_t)b * 2 + 0) * nn * nn + node] = (float)(w / cnt);
    out[((size_t)b * 2 + 1) * nn * nn + node] = (float)(v / cnt);
  }
}

}  // namespace pidm

using namespace pidm;

static const size_t kGenLdsMax = 150 * 1024;

static size_t simp_lds_bytes(int nel) {
  const size_t nn = (size_t)nel + 1;
  return (2 * nn * nn + (size_t)nel * nel) * sizeof(double);
}

extern "C" size_t pidm_simp_ws_bytes(int nel, int B) {
  if (nel < 1 || B < 1) return 256;
  return (size_t)B * 2 * (2 * (size_t)(nel + 1) * (nel + 1)) * sizeof(double) + 256;
}

// the argument checks shared by pidm_simp_step and pidm_simp_step_filtered (who: the entry's name in the message)
static int simp_check_args(const char* who, const double* x, const double* u, const float* bcs, const float* vf, const float* kloc,
                           int kloc_stride, const int32_t* elem_dofs, const int32_t* dof_elems, int nel, double penal, double e_min,
                           double rmin, double move, int n_bisect, int pcg_max_iter, double pcg_rtol, const double* x_new,
                           const double* u_out, const double* compliance, const double* change, const int32_t* pcg_iters,
                           const double* relres, const void* workspace, int B) {
  if (!kloc || !elem_dofs || !dof_elems) return fail("%s: null mesh table", who);
  if (!x || !u || !bcs || !vf || !x_new || !u_out || !compliance || !change || !pcg_iters || !relres || !workspace)
    return fail("%s: null buffer", who);
  if (x == x_new || u == u_out) return fail("%s: x_new / u_out must not alias x / u", who);
  if (((reinterpret_cast<size_t>(kloc) | reinterpret_cast<size_t>(elem_dofs) | reinterpret_cast<size_t>(dof_elems)) & 15) != 0)
    return fail("%s: the mesh tables must be 16-byte aligned (their rows are read as 16-byte pieces)", who);
  if (nel < 2 || simp_lds_bytes(nel) > kGenLdsMax)
    return fail("%s: nel=%d outside [2, 79] (the search direction and the moduli, (2 (nel+1)^2 + nel^2) doubles, must fit LDS)", who, nel);
  if (B <= 0) return fail("%s: B=%d must be positive", who, B);
  if (kloc_stride != 0 && kloc_stride != 64) return fail("%s: kloc_stride must be 0 or 64", who);
  if (!(rmin > 1.0)) return fail("%s: rmin=%g must be > 1 (a filter radius of one element or less filters nothing)", who, rmin);
  if (!(rmin <= (double)nel)) return fail("%s: rmin=%g larger than the mesh", who, rmin);
  if (n_bisect < 1) return fail("%s: n_bisect=%d must be >= 1", who, n_bisect);
  if (!(penal >= 1.0)) return fail("%s: penal=%g must be >= 1", who, penal);
  if (!(e_min > 0.0 && e_min < 1.0)) return fail("%s: e_min=%g must lie in (0, 1)", who, e_min);
  if (!(move > 0.0)) return fail("%s: move=%g must be positive", who, move);
  if (pcg_max_iter < 0 || !(pcg_rtol > 0.0)) return fail("%s: pcg_max_iter >= 0 and pcg_rtol > 0 required", who);
  return 0;
}

extern "C" int pidm_simp_step(const double* x, const double* u, const float* bcs, const float* vf, const int32_t* active,
                              const float* kloc, int kloc_stride, const int32_t* elem_dofs, const int32_t* dof_elems, int nel,
                              double penal, double e_min, double rmin, double move, int n_bisect, int pcg_max_iter,
                              double pcg_rtol, double* x_new, double* u_out, double* compliance, double* change,
                              int32_t* pcg_iters, double* relres, void* workspace, int B, void* stream) {
  if (const int rc = simp_check_args("simp_step", x, u, bcs, vf, kloc, kloc_stride, elem_dofs, dof_elems, nel, penal, e_min, rmin, move,
                                     n_bisect, pcg_max_iter, pcg_rtol, x_new, u_out, compliance, change, pcg_iters, relres, workspace, B))
    return rc;
  const int E = nel * nel, nn = nel + 1, ndof = 2 * nn * nn;
  GenMesh ms{elem_dofs, dof_elems, kloc, kloc_stride, E, ndof, nel, nn};
  SimpPar sp{penal, e_min, rmin, move, pcg_rtol, n_bisect, pcg_max_iter};
  double* ws = reinterpret_cast<double*>((reinterpret_cast<size_t>(workspace) + 255) & ~(size_t)255);
  // dofs per lane (a register array per CG vector): 4 up to nel = 31, 17 up to nel = 64, 25 up to nel = 79
  const int pts = cdiv(ndof, SG_THREADS);
#define PIDM_SIMP_LAUNCH(P_)                                                                                                     \
  do {                                                                                                                           \
    static bool attr = false;                                                                                                    \
    if (!attr) {                                                                                                                 \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&simp_step_kernel<P_>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                (int)kGenLdsMax);                                                                                \
      attr = true;                                                                                                               \
    }                                                                                                                            \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(simp_step_kernel<P_>), dim3(B), dim3(SG_THREADS), simp_lds_bytes(nel), as_stream(stream), ms, x, \
                       u, bcs, vf, active, sp, ws, x_new, u_out, compliance, change, pcg_iters, relres);                         \
  } while (0)
  if (pts <= 4) PIDM_SIMP_LAUNCH(4);
  else if (pts <= 17) PIDM_SIMP_LAUNCH(17);
  else PIDM_SIMP_LAUNCH(25);
#undef PIDM_SIMP_LAUNCH
  PIDM_CHECK_LAUNCH("simp_step_kernel");
  return 0;
}

extern "C" int pidm_simp_step_filtered(const double* x, const double* u, const float* bcs, const float* vf, const int32_t* active,
                                       const float* kloc, int kloc_stride, const int32_t* elem_dofs, const int32_t* dof_elems, int nel,
                                       double penal, double e_min, double rmin, double move, int n_bisect, int pcg_max_iter,
                                       double pcg_rtol, int filter, double beta, double eta, double* x_new, double* x_phys_new,
                                       double* u_out, double* compliance, double* change, int32_t* pcg_iters, double* relres,
                                       void* workspace, int B, void* stream) {
  if (!x_phys_new) return fail("simp_step_filtered: null buffer");
  if (x == x_phys_new || x_new == x_phys_new) return fail("simp_step_filtered: x_phys_new must not alias x / x_new");
  if (filter != 1 && filter != 2) return fail("simp_step_filtered: filter=%d must be 1 (density filter) or 2 (density filter + projection)", filter);
  if (!(beta > 0.0)) return fail("simp_step_filtered: beta=%g must be positive", beta);
  if (!(eta > 0.0 && eta < 1.0)) return fail("simp_step_filtered: eta=%g must lie in (0, 1)", eta);
  if (const int rc = simp_check_args("simp_step_filtered", x, u, bcs, vf, kloc, kloc_stride, elem_dofs, dof_elems, nel, penal, e_min, rmin,
                                     move, n_bisect, pcg_max_iter, pcg_rtol, x_new, u_out, compliance, change, pcg_iters, relres,
                                     workspace, B))
    return rc;
  const int E = nel * nel, nn = nel + 1, ndof = 2 * nn * nn;
  GenMesh ms{elem_dofs, dof_elems, kloc, kloc_stride, E, ndof, nel, nn};
  SimpPar sp{penal, e_min, rmin, move, pcg_rtol, n_bisect, pcg_max_iter};
  const double tb = tanh(beta * eta);
  ProjPar pj{filter, beta, eta, tb, tb + tanh(beta * (1.0 - eta))};
  double* ws = reinterpret_cast<double*>((reinterpret_cast<size_t>(workspace) + 255) & ~(size_t)255);
  const int pts = cdiv(ndof, SG_THREADS);   // (as pidm_simp_step)
#define PIDM_SIMP_LAUNCH(P_)                                                                                                          \
  do {                                                                                                                                \
    static bool attr = false;                                                                                                         \
    if (!attr) {                                                                                                                      \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&simp_step_filtered_kernel<P_>),                                        \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGenLdsMax);                                         \
      attr = true;                                                                                                                    \
    }                                                                                                                                 \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(simp_step_filtered_kernel<P_>), dim3(B), dim3(SG_THREADS), simp_lds_bytes(nel),                \
                       as_stream(stream), ms, x, u, bcs, vf, active, sp, pj, ws, x_new, x_phys_new, u_out, compliance, change,        \
                       pcg_iters, relres);                                                                                            \
  } while (0)
  if (pts <= 4) PIDM_SIMP_LAUNCH(4);
  else if (pts <= 17) PIDM_SIMP_LAUNCH(17);
  else PIDM_SIMP_LAUNCH(25);
#undef PIDM_SIMP_LAUNCH
  PIDM_CHECK_LAUNCH("simp_step_filtered_kernel");
  return 0;
}

extern "C" int pidm_mech_fields(const float* u_dofs, const float* rho, const float* kloc, int kloc_stride, const int32_t* elem_dofs,
                                int nel, double nu, float* fields, int B, void* stream) {
  if (!kloc || !elem_dofs) return fail("mech_fields: null mesh table");
  if (!u_dofs || !rho || !fields) return fail("mech_fields: null buffer");
  const size_t lds = 2 * (size_t)(nel > 0 ? nel : 0) * (size_t)(nel > 0 ? nel : 0) * sizeof(double);
  if (nel < 1 || lds > kGenLdsMax) return fail("mech_fields: nel=%d outside [1, 97] (two fp64 element fields must fit LDS)", nel);
  if (B <= 0) return fail("mech_fields: B=%d must be positive", B);
  if (kloc_stride != 0 && kloc_stride != 64) return fail("mech_fields: kloc_stride must be 0 or 64");
  if (!(nu > -1.0 && nu < 1.0)) return fail("mech_fields: nu=%g outside (-1, 1)", nu);
  const int E = nel * nel, nn = nel + 1, ndof = 2 * nn * nn;
  GenMesh ms{elem_dofs, nullptr, kloc, kloc_stride, E, ndof, nel, nn};
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mech_fields_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGenLdsMax);
    attr = true;
  }
  hipLaunchKernelGGL(mech_fields_kernel, dim3(B), dim3(256), lds, as_stream(stream), ms, u_dofs, rho, nu, fields);
  PIDM_CHECK_LAUNCH("mech_fields_kernel");
  return 0;
}
