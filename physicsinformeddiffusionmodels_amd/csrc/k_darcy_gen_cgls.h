// Darcy training-data generation for gfx950: KLE permeability synthesis and the fp64 least-squares pressure solve, shared by the
// generators of k_darcy_gen_acc.hip (findiff's classed operators) and k_darcy_gen_per.hip (wrapped central operators): everything
// but the enumeration of a 1-D operator and of its transpose.
//
// Replaces (reference path): src/darcy_data_generation.py:118-163 (generate_sample), which per sample assembles the dense
// (P^2+4P+1) x P^2 system  [A; boundary rows; integral row] p = [f_s; 0; 0]  with findiff and solves it with
// scipy.linalg.lstsq (7.2 s per 64x64 sample on a CPU core).  Here one workgroup per sample runs matrix-free CGLS in fp64:
//
//   A p        = -K p_00 - K_0 p_0 - K p_11 - K_1 p_1        (P^2 rows; D0, D00, D1, D11 and K_0 = D0 K, K_1 = D1 K from `Ops`)
//   boundary   = -D0 p on the x-min row, +D0 p on x-max, bc_sign * D1 p on y-min, -bc_sign * D1 p on y-max   (4P rows)
//   integral   = int_w . p                                                                                    (1 row)
//
// A_bc (the first P^2 + 4P rows) annihilates the constant field, so its least-squares solutions are q + c 1.  The solve
// therefore runs on A_bc alone (the constant mode no longer sets the smallest singular value) and deflates at the end:
// p = q - (int_w . q / int_w . 1) 1 is the least-squares solution of the full system (the integral row is then exactly
// satisfied and leaves the other rows unchanged).  Columns are scaled by 1 / ||A_bc e_j||; CGLS on A_bc S y = b, p = S y,
// stops at ||S A_bc^T r|| <= rtol ||S A_bc^T b|| or max_iter.  DESIGN.md section "Darcy data generation" has the measured
// iteration counts.
//
// Everything stays on chip inside the loop: each lane keeps the search direction, scaled gradient, column scales, row
// residuals and K, K_0, K_1 of its points in registers, its part of the iterate in LDS.  Neighbour access goes through one LDS
// region of three fp64 fields: S p_hat while A is applied (F1 then holds A S p_hat until the step length is known), then
// K r | K_0 r | K_1 r (the adjoint needs the neighbours' coefficients: A^T r = -D00^T (K r) - D0^T (K_0 r) - D11^T (K r) -
// D1^T (K_1 r)) plus the 4P boundary residuals.  The table of unit-spacing stencil coefficients lives in LDS as well.  Two block
// reductions per iteration (||A S p_hat||^2 and ||s||^2); their barriers also order the reuse of the LDS region.
//
// A kernel file supplies `Ops`, a stateless struct per finite-difference order whose static __device__ __forceinline__ members
// all take the coefficient table (in LDS) and P:
//
//   TAB_DOUBLES, fill(TAB)                       size of the table of unit-spacing coefficients and its fill (one lane)
//   taps(TAB, P, F, i, j, v0, v00, v1, v11)      forward tap sums of point (i, j) on the field F: D0 F, D00 F, D1 F, D11 F
//   boundary_sum(TAB, P, F, side, e, t)          (D F)(e) along the line t of axis side / 2, e = 0 | P-1 (no sign, no spacing)
//   pde_colnorm2(TAB, P, F0, F1, F2, a, bb, i0, i00, i1, i11)   the PDE rows' part of ||A_bc e_m||^2, m = (a, bb)
//   d1(TAB, P, last, m)                          first-derivative weight D[e][m] of row e = 0 (last: P-1)
//   adjoint_sums(TAB, P, F0, F1, F2, a, bb, s0, s00, s1, s11)   the four transposed sums of column m = (a, bb)
//
// 1/d and 1/d^2 multiply the sums here, where they are used.  Every floating-point expression below keeps the operand order and
// grouping the two kernels had when each carried its own copy: iteration counts depend on them.
//
// Launch protocol: a launch runs at most iters_this_launch CGLS iterations per unfinished sample and leaves the complete CGLS
// state (iterate, search direction, row and boundary residuals, gamma, gamma0, iteration count, done flag) in `state`; the next
// launch recomputes K, K_0, K_1 and the column scales (deterministic) and continues from it.  The launch in which a sample
// converges or reaches max_iter runs the deflation and the residual pass for it, once.  The loop is entered from the same values
// whether they come from the initialisation or from `state`, so a solve cut into launches of any size is bit-identical to the same
// solve in one launch.
#pragma once
#include <math.h>

#include "pidm_common.h"

namespace pidm {

constexpr int DGC_THREADS = 512;   // 8 waves: two per SIMD
constexpr int DGC_PTS = 8;         // points per lane at P = 64 (4096 / 512)
constexpr int DGC_RED = DGC_THREADS / 64;
constexpr size_t DGC_LDS_LIMIT = 160 * 1024;   // LDS of one gfx950 workgroup
// Between the points of a lane (and, in the classed operators, between groups of taps): the scheduler may not gather the LDS loads
// of a whole pass in front of their uses (13 candidates x 4 weights and 4 values in fp64 are 208 registers at classed acc 6; next
// to the 128 that the lane's eight points hold for good that spills).
#define DGC_POINT_FENCE() __builtin_amdgcn_sched_barrier(0)

// unit-spacing coefficient of tap k (offset k - acc/2; 0 for k > acc) of the central first (der 1) / second (der 2) derivative
constexpr double dgc_central(int acc, int der, int k) {
  const double c1_2[8] = {-1.0 / 2, 0.0, 1.0 / 2, 0, 0, 0, 0, 0};
  const double c1_4[8] = {1.0 / 12, -2.0 / 3, 0.0, 2.0 / 3, -1.0 / 12, 0, 0, 0};
  const double c1_6[8] = {-1.0 / 60, 3.0 / 20, -3.0 / 4, 0.0, 3.0 / 4, -3.0 / 20, 1.0 / 60, 0};
  const double c2_2[8] = {1.0, -2.0, 1.0, 0, 0, 0, 0, 0};
  const double c2_4[8] = {-1.0 / 12, 4.0 / 3, -5.0 / 2, 4.0 / 3, -1.0 / 12, 0, 0, 0};
  const double c2_6[8] = {1.0 / 90, -3.0 / 20, 3.0 / 2, -49.0 / 18, 3.0 / 2, -3.0 / 20, 1.0 / 90, 0};
  const double* c1 = acc == 2 ? c1_2 : (acc == 4 ? c1_4 : c1_6);
  const double* c2 = acc == 2 ? c2_2 : (acc == 4 ? c2_4 : c2_6);
  return der == 1 ? c1[k] : c2[k];
}

__device__ __forceinline__ double dgc_block_sum(double v, double* red) {   // all DGC_THREADS lanes; result broadcast
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < DGC_RED; ++w) s += red[w];
  return s;
}

// doubles of one sample's state: iterate | search direction | row residuals (P^2 each) | boundary residuals (4P) | gamma | gamma0 |
// one double's room for two int32: iterations done, done flag (pidm_darcy_gen_acc_state_bytes sizes the buffer of both entries)
__host__ __device__ inline size_t dgc_state_doubles(int P) { return (size_t)3 * P * P + 4 * (size_t)P + 3; }

// bytes of dynamic LDS (doubles): F0 | F1 | F2 | Y (P^2 each) | RB (4P) | TAB | RED (8)
inline size_t dgc_lds_bytes(int P, size_t tab_doubles) {
  return ((size_t)4 * P * P + 4 * (size_t)P + tab_doubles + DGC_RED) * sizeof(double);
}

template <class Ops>
__device__ __forceinline__ void darcy_gen_cgls_body(
    const double* __restrict__ basis, const double* __restrict__ z, int q, const double* __restrict__ K_in, int P, double d0, double d1,
    double bc_sign, const double* __restrict__ int_w, const double* __restrict__ f_s, int max_iter, double rtol, int iters_this_launch,
    int first_launch, double* __restrict__ state, double* __restrict__ K_out, double* __restrict__ p_out, double* __restrict__ res_mean,
    int32_t* __restrict__ iters_out, double* __restrict__ relres_out, int32_t* __restrict__ done_out) {
  HIP_DYNAMIC_SHARED(double, smem)
  const int b = blockIdx.x, tid = threadIdx.x, N = P * P, NB = 4 * P;
  double* st = state + (size_t)b * dgc_state_doubles(P);
  double* stY = st;
  double* stP = st + N;
  double* stR = st + 2 * N;
  double* stB = st + 3 * N;
  double* stG = st + 3 * N + NB;                                   // gamma, gamma0
  int32_t* stI = reinterpret_cast<int32_t*>(st + 3 * N + NB + 2);  // iterations, done
  if (!first_launch && stI[1] != 0) return;   // (the flag is written after the last barrier of the launch that finishes the sample)

  double* F0 = smem;
  double* F1 = smem + N;
  double* F2 = smem + 2 * N;
  double* Y = smem + 3 * N;     // the iterate: lane-private, in LDS to keep the register file for the vectors the stencils use
  double* RB = smem + 4 * N;
  double* TAB = smem + 4 * N + NB;
  double* red = TAB + Ops::TAB_DOUBLES;
  const double i0 = 1.0 / d0, i00 = 1.0 / (d0 * d0), i1 = 1.0 / d1, i11 = 1.0 / (d1 * d1);

  // ---- prologue (every launch): coefficient table, K = exp(B z) (or K_in), K_0, K_1, column scales -------------------------
  if (tid == 0) Ops::fill(TAB);
  double K[DGC_PTS], K0[DGC_PTS], K1[DGC_PTS], sc[DGC_PTS];
#pragma unroll
  for (int u = 0; u < DGC_PTS; ++u) {
    const int n = tid + u * DGC_THREADS;
    double k = 1.0;
    if (n < N) {
      if (z) {
        const double* zb = z + (size_t)b * q;
        double g = 0.0;
        for (int kk = 0; kk < q; ++kk) g += basis[(size_t)kk * N + n] * zb[kk];
        k = exp(g);
      } else {
        k = K_in[(size_t)b * N + n];
      }
      if (K_out && first_launch) K_out[(size_t)b * N + n] = k;
      F0[n] = k;
    }
    K[u] = k;
  }
  __syncthreads();

  // boundary row tq (< 4P) applied to the field F: x-min / x-max rows (0 | P-1, t) = -+ D0, y-min / y-max rows (t, 0 | P-1) =
  // +- bc_sign D1 (without the sign when `plain`)
  auto boundary_row = [&](const double* F, int tq, bool plain) -> double {
    const int side = tq / P, t = tq - side * P;
    const int e = side & 1 ? P - 1 : 0;
    double v = Ops::boundary_sum(TAB, P, F, side, e, t);
    v *= side < 2 ? i0 : i1;
    if (plain) return v;
    return side == 0 ? -v : (side == 1 ? v : (side == 2 ? bc_sign * v : -bc_sign * v));
  };

#pragma unroll
  for (int u = 0; u < DGC_PTS; ++u) {
    const int n = tid + u * DGC_THREADS;
    double g0 = 0.0, g1 = 0.0;
    if (n < N) {
      const int i = n / P, j = n - i * P;
      double v00, v11;
      Ops::taps(TAB, P, F0, i, j, g0, v00, g1, v11);
      g0 *= i0;
      g1 *= i1;
    }
    K0[u] = g0;
    K1[u] = g1;
    DGC_POINT_FENCE();
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < DGC_PTS; ++u) {
    const int n = tid + u * DGC_THREADS;
    if (n < N) { F1[n] = K0[u]; F2[n] = K1[u]; }
  }
  __syncthreads();
  // ||A_bc e_m||^2, m = (a, bb): the PDE rows whose stencils touch m (Ops::pde_colnorm2) and the four boundary rows that touch m
#pragma unroll
  for (int u = 0; u < DGC_PTS; ++u) {
    const int n = tid + u * DGC_THREADS;
    double s2 = 1.0;
    if (n < N) {
      const int a = n / P, bb = n - a * P;
      s2 = Ops::pde_colnorm2(TAB, P, F0, F1, F2, a, bb, i0, i00, i1, i11);
      double w;
      w = Ops::d1(TAB, P, false, a) * i0;    // x-min row (0, bb)
      s2 += w * w;
      w = Ops::d1(TAB, P, true, a) * i0;     // x-max row (P-1, bb)
      s2 += w * w;
      w = Ops::d1(TAB, P, false, bb) * i1;   // y-min row (a, 0)
      s2 += w * w;
      w = Ops::d1(TAB, P, true, bb) * i1;    // y-max row (a, P-1)
      s2 += w * w;
    }
    sc[u] = 1.0 / sqrt(s2);
    DGC_POINT_FENCE();
  }

  // ---- CGLS on A_bc S ---------------------------------------------------------------------------------------------------
  double ph[DGC_PTS], s[DGC_PTS], r[DGC_PTS];
  double rb = 0.0;                               // boundary row tid (tid < 4P)

  // s = S A_bc^T r (reads F0..F2 / RB after its own barrier); returns the lane's partial ||s||^2
  auto adjoint = [&](int tq) -> double {
    PIDM_OPAQUE_I32(tq);   // (nor may the indices of the forward pass stay live for the transposed one)
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) {
      const int n = tq + u * DGC_THREADS;
      if (n < N) { F0[n] = K[u] * r[u]; F1[n] = K0[u] * r[u]; F2[n] = K1[u] * r[u]; }
    }
    if (tq < NB) RB[tq] = rb;
    __syncthreads();
    double part = 0.0;
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) {
      const int n = tq + u * DGC_THREADS;
      double v = 0.0;
      if (n < N) {
        const int a = n / P, bb = n - a * P;
        double s0, s00, s1, s11;
        Ops::adjoint_sums(TAB, P, F0, F1, F2, a, bb, s0, s00, s1, s11);
        v = -(s00 * i00 + s0 * i0 + s11 * i11 + s1 * i1);
        // boundary rows: x-min (0, bb) = -D0 row 0, x-max (P-1, bb) = +D0 row P-1, y-min (a, 0) = bc_sign D1 row 0, y-max -bc_sign
        v -= Ops::d1(TAB, P, false, a) * i0 * RB[bb];
        v += Ops::d1(TAB, P, true, a) * i0 * RB[P + bb];
        v += bc_sign * (Ops::d1(TAB, P, false, bb) * i1) * RB[2 * P + a];
        v -= bc_sign * (Ops::d1(TAB, P, true, bb) * i1) * RB[3 * P + a];
        v *= sc[u];
      }
      s[u] = v;
      part += v * v;
      DGC_POINT_FENCE();
    }
    return part;
  };

  double gamma, gamma0;
  int it;
  __syncthreads();                               // (every read of the column-scale pass is done before F0..F2 are rewritten)
  if (first_launch) {
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) {
      const int n = tid + u * DGC_THREADS;
      if (n < N) Y[n] = 0.0;
      r[u] = n < N ? f_s[n] : 0.0;
    }
    gamma = dgc_block_sum(adjoint(tid), red);
    gamma0 = gamma;
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) ph[u] = s[u];
    it = 0;
  } else {
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) {
      const int n = tid + u * DGC_THREADS;
      if (n < N) Y[n] = stY[n];
      ph[u] = n < N ? stP[n] : 0.0;
      r[u] = n < N ? stR[n] : 0.0;
    }
    if (tid < NB) rb = stB[tid];
    gamma = stG[0];
    gamma0 = stG[1];
    it = stI[0];
  }
  const double stop = rtol * rtol * gamma0;
  for (int budget = iters_this_launch; budget > 0 && it < max_iter && gamma > stop; --budget, ++it) {
    // The stencil taps of a lane's points depend on the point only; hoisted out of the loop they would fill the register file.  An
    // index the compiler cannot see through keeps them inside: recomputing them is a few selects and table reads.
    int tq = tid;
    PIDM_OPAQUE_I32(tq);
    // q = A_bc S p_hat
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) {
      const int n = tq + u * DGC_THREADS;
      if (n < N) F0[n] = sc[u] * ph[u];
    }
    __syncthreads();
    double qb = 0.0, part = 0.0;
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) {
      const int n = tq + u * DGC_THREADS;
      double v = 0.0;
      if (n < N) {
        const int i = n / P, j = n - i * P;
        double v0, v00, v1, v11;
        Ops::taps(TAB, P, F0, i, j, v0, v00, v1, v11);
        v = -K[u] * (v00 * i00) - K0[u] * (v0 * i0) - K[u] * (v11 * i11) - K1[u] * (v1 * i1);
      }
      if (n < N) F1[n] = v;   // (lane-private until the adjoint rewrites F1: the lane reads it back after the reduction)
      part += v * v;
      DGC_POINT_FENCE();
    }
    if (tq < NB) {
      qb = boundary_row(F0, tq, false);
      part += qb * qb;
    }
    const double delta = dgc_block_sum(part, red);   // (its barriers also retire every read of S p_hat)
    const double alpha = delta > 0.0 ? gamma / delta : 0.0;
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) {
      const int n = tq + u * DGC_THREADS;
      if (n < N) {
        Y[n] += alpha * ph[u];
        r[u] -= alpha * F1[n];
      }
    }
    rb -= alpha * qb;
    const double gnew = dgc_block_sum(adjoint(tq), red);
    const double beta = gnew / gamma;
    gamma = gnew;
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) ph[u] = s[u] + beta * ph[u];
  }

  if (it < max_iter && gamma > stop) {
    // ---- not finished: leave the state for the next launch --------------------------------------------------------------
#pragma unroll
    for (int u = 0; u < DGC_PTS; ++u) {
      const int n = tid + u * DGC_THREADS;
      if (n < N) { stY[n] = Y[n]; stP[n] = ph[u]; stR[n] = r[u]; }
    }
    if (tid < NB) stB[tid] = rb;
    if (tid == 0) {
      stG[0] = gamma;
      stG[1] = gamma0;
      stI[0] = it;
      stI[1] = 0;
      done_out[b] = 0;
    }
    return;
  }

  // ---- finished: deflation p = S y - (c . S y / c . 1) 1, then the residual of all P^2 + 4P + 1 rows ---------------------------
  double cx = 0.0, c1 = 0.0;
#pragma unroll
  for (int u = 0; u < DGC_PTS; ++u) {
    const int n = tid + u * DGC_THREADS;
    if (n < N) {
      const double x = Y[n] * sc[u];
      Y[n] = x;
      cx += int_w[n] * x;
      c1 += int_w[n];
    }
  }
  cx = dgc_block_sum(cx, red);
  c1 = dgc_block_sum(c1, red);
  const double shift = cx / c1;
  double cp = 0.0;
#pragma unroll
  for (int u = 0; u < DGC_PTS; ++u) {
    const int n = tid + u * DGC_THREADS;
    if (n < N) {
      const double p = Y[n] - shift;
      F0[n] = p;
      p_out[(size_t)b * N + n] = p;
      cp += int_w[n] * p;
    }
  }
  __syncthreads();
  double rabs = 0.0;
#pragma unroll
  for (int u = 0; u < DGC_PTS; ++u) {
    const int n = tid + u * DGC_THREADS;
    if (n < N) {
      const int i = n / P, j = n - i * P;
      double v0, v00, v1, v11;
      Ops::taps(TAB, P, F0, i, j, v0, v00, v1, v11);
      rabs += fabs(-K[u] * (v00 * i00) - K0[u] * (v0 * i0) - K[u] * (v11 * i11) - K1[u] * (v1 * i1) - f_s[n]);
    }
    DGC_POINT_FENCE();
  }
  if (tid < NB) rabs += fabs(boundary_row(F0, tid, true));   // |-+v| = |v|
  rabs = dgc_block_sum(rabs, red);
  cp = dgc_block_sum(cp, red);
  if (tid == 0) {
    if (res_mean) res_mean[b] = (rabs + fabs(cp)) / (double)(N + NB + 1);
    if (iters_out) iters_out[b] = it;
    if (relres_out) relres_out[b] = gamma0 > 0.0 ? sqrt(gamma / gamma0) : 0.0;
    stI[0] = it;
    stI[1] = 1;
    done_out[b] = 1;
  }
}

// one launch of KERNEL, an instantiation of darcy_gen_acc_kernel / darcy_gen_per_kernel (`label`: its template's name)
template <auto KERNEL>
static int darcy_gen_launch(const char* label, const double* basis, const double* z, int q, const double* K_in, int P, double d0,
                            double d1, double bc_sign, const double* int_w, const double* f_s, int max_iter, double rtol,
                            int iters_this_launch, int first_launch, double* state, double* K_out, double* p_out, double* res_mean,
                            int32_t* iters, double* relres, int32_t* done, int B, size_t lds, void* stream) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DGC_LDS_LIMIT);
    attr = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(B), dim3(DGC_THREADS), lds, as_stream(stream), basis, z, q, K_in, P, d0, d1, bc_sign, int_w, f_s,
                     max_iter, rtol, iters_this_launch, first_launch, state, K_out, p_out, res_mean, iters, relres, done);
  PIDM_CHECK_LAUNCH(label);
  return 0;
}

// What both extern "C" entries do: the argument checks (`name` heads every message; P must lie in [pmin, 64], `p_note` ends that
// message) and the launch of the order's instantiation K2 / K4 / K6 with `lds` bytes of dynamic LDS.
template <auto K2, auto K4, auto K6>
static int darcy_gen_entry(const char* name, const char* label, int pmin, const char* p_note, size_t lds, const double* basis,
                           const double* z, int q, const double* K_in, int P, int acc, double d0, double d1, double bc_sign,
                           const double* int_w, const double* f_s, int max_iter, double rtol, int iters_this_launch, int first_launch,
                           void* state, double* K_out, double* p_out, double* res_mean, int32_t* iters, double* relres, int32_t* done,
                           int B, void* stream) {
  if (acc != 2 && acc != 4 && acc != 6) return fail("%s: acc=%d is not one of 2, 4, 6", name, acc);
  if (P < pmin || P > 64) return fail("%s: P=%d outside [%d, 64]%s", name, P, pmin, p_note);
  if (B < 0) return fail("%s: B=%d must be >= 0", name, B);
  if (z) {
    if (!basis) return fail("%s: z given without a basis", name);
    if (q < 1 || q > P * P) return fail("%s: q=%d outside [1, P^2=%d]", name, q, P * P);
  } else if (!K_in) {
    return fail("%s: neither z (KLE synthesis) nor K_in given", name);
  }
  if (!int_w || !f_s || !p_out) return fail("%s: null buffer", name);
  if (!state) return fail("%s: null state buffer (pidm_darcy_gen_acc_state_bytes(P, B) bytes)", name);
  if (!done) return fail("%s: null done flags", name);
  if (iters_this_launch < 1) return fail("%s: iters_this_launch=%d must be >= 1", name, iters_this_launch);
  if (max_iter < 0 || !(rtol > 0.0)) return fail("%s: max_iter >= 0 and rtol > 0 required", name);
  if (!(d0 != 0.0) || !(d1 != 0.0)) return fail("%s: zero grid spacing", name);
  if (lds > DGC_LDS_LIMIT)
    return fail("%s: P=%d at acc=%d needs %zu bytes of LDS, a gfx950 workgroup has %zu", name, P, acc, lds, DGC_LDS_LIMIT);
  if (B == 0) return 0;
  double* st = static_cast<double*>(state);
  const int fl = first_launch != 0;
#define PIDM_DGC_ARGS label, basis, z, q, K_in, P, d0, d1, bc_sign, int_w, f_s, max_iter, rtol, iters_this_launch, fl, st, K_out, \
                      p_out, res_mean, iters, relres, done, B, lds, stream
  if (acc == 2) return darcy_gen_launch<K2>(PIDM_DGC_ARGS);
  if (acc == 4) return darcy_gen_launch<K4>(PIDM_DGC_ARGS);
  return darcy_gen_launch<K6>(PIDM_DGC_ARGS);
#undef PIDM_DGC_ARGS
}

}  // namespace pidm
