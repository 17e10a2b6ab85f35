// Darcy training-data generation at finite-difference order acc = 2, 4, 6: the solve of k_darcy_gen.hip with findiff's classed
// operators of any of the three orders, in bounded, resumable launches.
//
// Replaces (reference path): src/darcy_data_generation.py:129-163 with `acc` as the reference passes it to every
// FinDiff(..., acc=acc).  The system, the row order, the column scaling, the deflation by the integral row and the stopping rule
// are those of k_darcy_gen.hip (read its header first); what changes is the 1-D operators:
//
//   rows i < mio use the forward stencil (taps i .. i+n-1), rows i > P-1-mio the backward one (taps i-n+1 .. i), all others the
//   central one (taps i-mio .. i+mio), mio = acc / 2 for both derivatives; central stencils have acc+1 taps, one-sided first
//   derivatives acc+1, one-sided second derivatives acc+2 (grad_utils.fd_offsets / fd_coefficients state the same rule).
//
// One table of unit-spacing coefficients serves both axes and lives in LDS: entry (class, k) = (first-derivative weight, second-
// derivative weight) of the tap at column base(i) + k, k < NT = acc+2, base = i (low class), i - mio (central), i - (acc+1) (high);
// taps a stencil does not have carry weight 0.  1/d and 1/d^2 multiply the tap sums where they are used.  The transposed
// operators (column scales, adjoint) enumerate the rows that touch column m by class, each exactly once: the acc+1 central rows
// m-mio .. m+mio that ARE central rows, the mio low-edge rows and the mio high-edge rows - 2 acc + 1 candidates, whatever P.
//
// Launch protocol: a launch runs at most iters_this_launch CGLS iterations per unfinished sample and leaves the complete CGLS
// state (iterate, search direction, row and boundary residuals, gamma, gamma0, iteration count, done flag) in `state`; the next
// launch recomputes K, K_0, K_1 and the column scales (deterministic) and continues from it.  The launch in which a sample
// converges or reaches max_iter runs the deflation and the residual pass for it, once.  The loop is entered from the same values
// whether they come from the initialisation or from `state`, so a solve cut into launches of any size is bit-identical to the same
// solve in one launch.
#include <math.h>

#include "pidm_common.h"

namespace pidm {

constexpr int DGA_THREADS = 512;   // 8 waves: two per SIMD
constexpr int DGA_PTS = 8;         // points per lane at P = 64 (4096 / 512)
constexpr int DGA_RED = DGA_THREADS / 64;
constexpr size_t DGA_LDS_LIMIT = 160 * 1024;   // LDS of one gfx950 workgroup
// Between the points of a lane and between groups of taps: the scheduler may not gather the LDS loads of a whole pass in front of
// their uses (13 candidates x 4 weights and 4 values in fp64 are 208 registers at acc 6; next to the 128 that the lane's eight
// points hold for good that spills).
#define DGA_POINT_FENCE() __builtin_amdgcn_sched_barrier(0)

// (class, k, derivative) -> unit-spacing coefficient, classes 0 low / 1 central / 2 high; see the header
template <int ACC>
struct DgaTable {
  static constexpr int NT = ACC + 2;
  double w[(3 * NT + 1) * 2];   // (the last pair is zero)
};
template <int ACC>
constexpr DgaTable<ACC> dga_make_table() {
  constexpr int NT = ACC + 2;
  // forward first / second derivative (acc+1 / acc+2 taps) and central first / second derivative (acc+1 taps); the backward
  // stencils are the mirrored forward ones (first derivative: negated)
  const double f1_2[8] = {-3.0 / 2, 2.0, -1.0 / 2, 0, 0, 0, 0, 0};
  const double f1_4[8] = {-25.0 / 12, 4.0, -3.0, 4.0 / 3, -1.0 / 4, 0, 0, 0};
  const double f1_6[8] = {-49.0 / 20, 6.0, -15.0 / 2, 20.0 / 3, -15.0 / 4, 6.0 / 5, -1.0 / 6, 0};
  const double f2_2[8] = {2.0, -5.0, 4.0, -1.0, 0, 0, 0, 0};
  const double f2_4[8] = {15.0 / 4, -77.0 / 6, 107.0 / 6, -13.0, 61.0 / 12, -5.0 / 6, 0, 0};
  const double f2_6[8] = {469.0 / 90, -223.0 / 10, 879.0 / 20, -949.0 / 18, 41.0, -201.0 / 10, 1019.0 / 180, -7.0 / 10};
  const double c1_2[8] = {-1.0 / 2, 0.0, 1.0 / 2, 0, 0, 0, 0, 0};
  const double c1_4[8] = {1.0 / 12, -2.0 / 3, 0.0, 2.0 / 3, -1.0 / 12, 0, 0, 0};
  const double c1_6[8] = {-1.0 / 60, 3.0 / 20, -3.0 / 4, 0.0, 3.0 / 4, -3.0 / 20, 1.0 / 60, 0};
  const double c2_2[8] = {1.0, -2.0, 1.0, 0, 0, 0, 0, 0};
  const double c2_4[8] = {-1.0 / 12, 4.0 / 3, -5.0 / 2, 4.0 / 3, -1.0 / 12, 0, 0, 0};
  const double c2_6[8] = {1.0 / 90, -3.0 / 20, 3.0 / 2, -49.0 / 18, 3.0 / 2, -3.0 / 20, 1.0 / 90, 0};
  const double* f1 = ACC == 2 ? f1_2 : (ACC == 4 ? f1_4 : f1_6);
  const double* f2 = ACC == 2 ? f2_2 : (ACC == 4 ? f2_4 : f2_6);
  const double* c1 = ACC == 2 ? c1_2 : (ACC == 4 ? c1_4 : c1_6);
  const double* c2 = ACC == 2 ? c2_2 : (ACC == 4 ? c2_4 : c2_6);
  DgaTable<ACC> t{};
  for (int k = 0; k < NT; ++k) {
    const int j = ACC + 1 - k;   // high class: tap k sits at offset -j
    t.w[(0 * NT + k) * 2 + 0] = f1[k];
    t.w[(0 * NT + k) * 2 + 1] = f2[k];
    t.w[(1 * NT + k) * 2 + 0] = k <= ACC ? c1[k] : 0.0;
    t.w[(1 * NT + k) * 2 + 1] = k <= ACC ? c2[k] : 0.0;
    t.w[(2 * NT + k) * 2 + 0] = j <= ACC ? -f1[j] : 0.0;
    t.w[(2 * NT + k) * 2 + 1] = f2[j];
  }
  return t;
}

__device__ __forceinline__ int dga_clamp(int v, int P) { return v < 0 ? 0 : (v > P - 1 ? P - 1 : v); }

// class of row i and the column of its tap 0
template <int ACC>
__device__ __forceinline__ void dga_row(int i, int P, int& cls, int& base) {
  constexpr int MIO = ACC / 2;
  cls = i < MIO ? 0 : (i > P - 1 - MIO ? 2 : 1);
  base = cls == 0 ? i : (cls == 1 ? i - MIO : i - (ACC + 1));
}

// candidate c (a constant in the unrolled loops, c < 2 ACC + 1) of the rows that touch column m: row i (clamped into the grid),
// table entry e = class * NT + k of D[i][m] (the zero entry 3 NT otherwise: the hot loops read weights without a branch), and
// whether the row exists and reaches m.  c <= ACC: the central rows m-mio .. m+mio;
// then the mio low-edge rows 0 .. mio-1; then the mio high-edge rows P-1 .. P-mio.  The three sets are disjoint by class.
template <int ACC>
__device__ __forceinline__ bool dga_cand(int c, int m, int P, int& i, int& e) {
  constexpr int MIO = ACC / 2, NT = ACC + 2;
  bool ok;
  if (c <= ACC) {
    i = m - MIO + c;
    ok = i >= MIO && i <= P - 1 - MIO;
    e = ok ? NT + (ACC - c) : 3 * NT;
  } else {
    const bool low = c <= ACC + MIO;
    const int t = low ? c - ACC - 1 : c - ACC - MIO - 1;
    i = low ? t : P - 1 - t;
    const int k = low ? m - t : m - (i - (ACC + 1));
    ok = k >= 0 && k < NT;
    e = ok ? (low ? 0 : 2 * NT) + k : 3 * NT;
  }
  i = dga_clamp(i, P);
  return ok;
}
// the candidates that are row 0 and row P-1 (the boundary rows' operators)
template <int ACC> constexpr int dga_cand_first() { return ACC + 1; }
template <int ACC> constexpr int dga_cand_last() { return ACC + ACC / 2 + 1; }

__device__ __forceinline__ double dga_block_sum(double v, double* red) {   // all DGA_THREADS lanes; result broadcast
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < DGA_RED; ++w) s += red[w];
  return s;
}

// doubles of one sample's state: iterate | search direction | row residuals (P^2 each) | boundary residuals (4P) | gamma | gamma0 |
// one double's room for two int32: iterations done, done flag
__host__ __device__ inline size_t dga_state_doubles(int P) { return (size_t)3 * P * P + 4 * (size_t)P + 3; }

// LDS (doubles): F0 | F1 | F2 | Y (P^2 each) | RB (4P) | TAB ((3 NT + 1) * 2) | RED (8)
template <int ACC>
__global__ void __launch_bounds__(DGA_THREADS)
    darcy_gen_acc_kernel(const double* __restrict__ basis, const double* __restrict__ z, int q, const double* __restrict__ K_in, int P,
                         double d0, double d1, double bc_sign, const double* __restrict__ int_w, const double* __restrict__ f_s,
                         int max_iter, double rtol, int iters_this_launch, int first_launch, double* __restrict__ state,
                         double* __restrict__ K_out, double* __restrict__ p_out, double* __restrict__ res_mean,
                         int32_t* __restrict__ iters_out, double* __restrict__ relres_out, int32_t* __restrict__ done_out) {
  constexpr int NT = ACC + 2, NC = 2 * ACC + 1;
  HIP_DYNAMIC_SHARED(double, smem)
  const int b = blockIdx.x, tid = threadIdx.x, N = P * P, NB = 4 * P;
  double* st = state + (size_t)b * dga_state_doubles(P);
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
  double* red = TAB + (3 * NT + 1) * 2;
  const double i0 = 1.0 / d0, i00 = 1.0 / (d0 * d0), i1 = 1.0 / d1, i11 = 1.0 / (d1 * d1);

  // ---- prologue (every launch): coefficient table, K = exp(B z) (or K_in), K_0, K_1, column scales -------------------------
  if (tid == 0) {
    constexpr DgaTable<ACC> tab = dga_make_table<ACC>();
#pragma unroll
    for (int e = 0; e < (3 * NT + 1) * 2; ++e) TAB[e] = tab.w[e];
  }
  double K[DGA_PTS], K0[DGA_PTS], K1[DGA_PTS], sc[DGA_PTS];
#pragma unroll
  for (int u = 0; u < DGA_PTS; ++u) {
    const int n = tid + u * DGA_THREADS;
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

  // forward taps of point (i, j) on the field F: the four unit-spacing sums D0 F, D00 F, D1 F, D11 F
  auto stencils = [&](const double* F, int i, int j, double& v0, double& v00, double& v1, double& v11) {
    int ci, bi, cj, bj;
    dga_row<ACC>(i, P, ci, bi);
    dga_row<ACC>(j, P, cj, bj);
    v0 = v00 = v1 = v11 = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const double xa = F[dga_clamp(bi + k, P) * P + j], xb = F[i * P + dga_clamp(bj + k, P)];
      const double* wa = TAB + (ci * NT + k) * 2;
      const double* wb = TAB + (cj * NT + k) * 2;
      v0 += wa[0] * xa;
      v00 += wa[1] * xa;
      v1 += wb[0] * xb;
      v11 += wb[1] * xb;
      if (k % 4 == 3) DGA_POINT_FENCE();
    }
  };
  // boundary row tq (< 4P) applied to the field F: x-min / x-max rows (0 | P-1, t) = -+ D0, y-min / y-max rows (t, 0 | P-1) =
  // +- bc_sign D1 (without the sign when `plain`)
  auto boundary_row = [&](const double* F, int tq, bool plain) -> double {
    const int side = tq / P, t = tq - side * P;
    const int e = side & 1 ? P - 1 : 0;
    int ce, be;
    dga_row<ACC>(e, P, ce, be);
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int col = dga_clamp(be + k, P);
      v += TAB[(ce * NT + k) * 2] * (side < 2 ? F[col * P + t] : F[t * P + col]);
    }
    v *= side < 2 ? i0 : i1;
    if (plain) return v;
    return side == 0 ? -v : (side == 1 ? v : (side == 2 ? bc_sign * v : -bc_sign * v));
  };

#pragma unroll
  for (int u = 0; u < DGA_PTS; ++u) {
    const int n = tid + u * DGA_THREADS;
    double g0 = 0.0, g1 = 0.0;
    if (n < N) {
      const int i = n / P, j = n - i * P;
      double v00, v11;
      stencils(F0, i, j, g0, v00, g1, v11);
      g0 *= i0;
      g1 *= i1;
    }
    K0[u] = g0;
    K1[u] = g1;
    DGA_POINT_FENCE();
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < DGA_PTS; ++u) {
    const int n = tid + u * DGA_THREADS;
    if (n < N) { F1[n] = K0[u]; F2[n] = K1[u]; }
  }
  __syncthreads();
  // ||A_bc e_m||^2, m = (a, bb): the rows (i, bb) whose axis-0 stencil touches a (row (a, bb) also carries the axis-1 diagonal), the
  // rows (a, j != bb) whose axis-1 stencil touches bb, and the four boundary rows that touch m
#pragma unroll
  for (int u = 0; u < DGA_PTS; ++u) {
    const int n = tid + u * DGA_THREADS;
    double s2 = 1.0;
    if (n < N) {
      const int a = n / P, bb = n - a * P;
      int cb, bsb;
      dga_row<ACC>(bb, P, cb, bsb);
      const double dd1 = TAB[(cb * NT + (bb - bsb)) * 2], dd2 = TAB[(cb * NT + (bb - bsb)) * 2 + 1];
      s2 = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        int i, e;
        {   // (a row that does not reach the column reads the zero entry: v = 0)
          const bool ok = dga_cand<ACC>(c, a, P, i, e);
          const int r = i * P + bb;
          double v = -F0[r] * (TAB[2 * e + 1] * i00) - F1[r] * (TAB[2 * e] * i0);
          if (ok && i == a) v += -F0[r] * (dd2 * i11) - F2[r] * (dd1 * i1);
          s2 += v * v;
        }
        {
          int j;
          const bool ok = dga_cand<ACC>(c, bb, P, j, e);
          const int r = a * P + j;
          const double v = ok && j != bb ? -F0[r] * (TAB[2 * e + 1] * i11) - F2[r] * (TAB[2 * e] * i1) : 0.0;
          s2 += v * v;
        }
        if (c % 3 == 2) DGA_POINT_FENCE();
      }
      int i, e;
      double w;
      dga_cand<ACC>(dga_cand_first<ACC>(), a, P, i, e);    // x-min row (0, bb)
      w = TAB[2 * e] * i0;
      s2 += w * w;
      dga_cand<ACC>(dga_cand_last<ACC>(), a, P, i, e);     // x-max row (P-1, bb)
      w = TAB[2 * e] * i0;
      s2 += w * w;
      dga_cand<ACC>(dga_cand_first<ACC>(), bb, P, i, e);   // y-min row (a, 0)
      w = TAB[2 * e] * i1;
      s2 += w * w;
      dga_cand<ACC>(dga_cand_last<ACC>(), bb, P, i, e);    // y-max row (a, P-1)
      w = TAB[2 * e] * i1;
      s2 += w * w;
    }
    sc[u] = 1.0 / sqrt(s2);
    DGA_POINT_FENCE();
  }

  // ---- CGLS on A_bc S ---------------------------------------------------------------------------------------------------
  double ph[DGA_PTS], s[DGA_PTS], r[DGA_PTS];
  double rb = 0.0;                               // boundary row tid (tid < 4P)

  // s = S A_bc^T r (reads F0..F2 / RB after its own barrier); returns the lane's partial ||s||^2
  auto adjoint = [&](int tq) -> double {
    PIDM_OPAQUE_I32(tq);   // (nor may the indices of the forward pass stay live for the transposed one)
#pragma unroll
    for (int u = 0; u < DGA_PTS; ++u) {
      const int n = tq + u * DGA_THREADS;
      if (n < N) { F0[n] = K[u] * r[u]; F1[n] = K0[u] * r[u]; F2[n] = K1[u] * r[u]; }
    }
    if (tq < NB) RB[tq] = rb;
    __syncthreads();
    double part = 0.0;
#pragma unroll
    for (int u = 0; u < DGA_PTS; ++u) {
      const int n = tq + u * DGA_THREADS;
      double v = 0.0;
      if (n < N) {
        const int a = n / P, bb = n - a * P;
        double s0 = 0.0, s00 = 0.0, s1 = 0.0, s11 = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          int ia, ea, jb, eb;
          dga_cand<ACC>(c, a, P, ia, ea);
          dga_cand<ACC>(c, bb, P, jb, eb);
          const double wa1 = TAB[2 * ea], wa2 = TAB[2 * ea + 1], wb1 = TAB[2 * eb], wb2 = TAB[2 * eb + 1];
          const int ra = ia * P + bb, rr = a * P + jb;
          s00 += wa2 * F0[ra];
          s0 += wa1 * F1[ra];
          s11 += wb2 * F0[rr];
          s1 += wb1 * F2[rr];
          if (c % 3 == 2) DGA_POINT_FENCE();   // (the loads of at most three candidates in flight)
        }
        v = -(s00 * i00 + s0 * i0 + s11 * i11 + s1 * i1);
        // boundary rows: x-min (0, bb) = -D0 row 0, x-max (P-1, bb) = +D0 row P-1, y-min (a, 0) = bc_sign D1 row 0, y-max -bc_sign
        int i, e;
        dga_cand<ACC>(dga_cand_first<ACC>(), a, P, i, e);
        v -= TAB[2 * e] * i0 * RB[bb];
        dga_cand<ACC>(dga_cand_last<ACC>(), a, P, i, e);
        v += TAB[2 * e] * i0 * RB[P + bb];
        dga_cand<ACC>(dga_cand_first<ACC>(), bb, P, i, e);
        v += bc_sign * (TAB[2 * e] * i1) * RB[2 * P + a];
        dga_cand<ACC>(dga_cand_last<ACC>(), bb, P, i, e);
        v -= bc_sign * (TAB[2 * e] * i1) * RB[3 * P + a];
        v *= sc[u];
      }
      s[u] = v;
      part += v * v;
      DGA_POINT_FENCE();
    }
    return part;
  };

  double gamma, gamma0;
  int it;
  __syncthreads();                               // (every read of the column-scale pass is done before F0..F2 are rewritten)
  if (first_launch) {
#pragma unroll
    for (int u = 0; u < DGA_PTS; ++u) {
      const int n = tid + u * DGA_THREADS;
      if (n < N) Y[n] = 0.0;
      r[u] = n < N ? f_s[n] : 0.0;
    }
    gamma = dga_block_sum(adjoint(tid), red);
    gamma0 = gamma;
#pragma unroll
    for (int u = 0; u < DGA_PTS; ++u) ph[u] = s[u];
    it = 0;
  } else {
#pragma unroll
    for (int u = 0; u < DGA_PTS; ++u) {
      const int n = tid + u * DGA_THREADS;
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
    for (int u = 0; u < DGA_PTS; ++u) {
      const int n = tq + u * DGA_THREADS;
      if (n < N) F0[n] = sc[u] * ph[u];
    }
    __syncthreads();
    double qb = 0.0, part = 0.0;
#pragma unroll
    for (int u = 0; u < DGA_PTS; ++u) {
      const int n = tq + u * DGA_THREADS;
      double v = 0.0;
      if (n < N) {
        const int i = n / P, j = n - i * P;
        double v0, v00, v1, v11;
        stencils(F0, i, j, v0, v00, v1, v11);
        v = -K[u] * (v00 * i00) - K0[u] * (v0 * i0) - K[u] * (v11 * i11) - K1[u] * (v1 * i1);
      }
      if (n < N) F1[n] = v;   // (lane-private until the adjoint rewrites F1: the lane reads it back after the reduction)
      part += v * v;
      DGA_POINT_FENCE();
    }
    if (tq < NB) {
      qb = boundary_row(F0, tq, false);
      part += qb * qb;
    }
    const double delta = dga_block_sum(part, red);   // (its barriers also retire every read of S p_hat)
    const double alpha = delta > 0.0 ? gamma / delta : 0.0;
#pragma unroll
    for (int u = 0; u < DGA_PTS; ++u) {
      const int n = tq + u * DGA_THREADS;
      if (n < N) {
        Y[n] += alpha * ph[u];
        r[u] -= alpha * F1[n];
      }
    }
    rb -= alpha * qb;
    const double gnew = dga_block_sum(adjoint(tq), red);
    const double beta = gnew / gamma;
    gamma = gnew;
#pragma unroll
    for (int u = 0; u < DGA_PTS; ++u) ph[u] = s[u] + beta * ph[u];
  }

  if (it < max_iter && gamma > stop) {
    // ---- not finished: leave the state for the next launch --------------------------------------------------------------
#pragma unroll
    for (int u = 0; u < DGA_PTS; ++u) {
      const int n = tid + u * DGA_THREADS;
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
  for (int u = 0; u < DGA_PTS; ++u) {
    const int n = tid + u * DGA_THREADS;
    if (n < N) {
      const double x = Y[n] * sc[u];
      Y[n] = x;
      cx += int_w[n] * x;
      c1 += int_w[n];
    }
  }
  cx = dga_block_sum(cx, red);
  c1 = dga_block_sum(c1, red);
  const double shift = cx / c1;
  double cp = 0.0;
#pragma unroll
  for (int u = 0; u < DGA_PTS; ++u) {
    const int n = tid + u * DGA_THREADS;
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
  for (int u = 0; u < DGA_PTS; ++u) {
    const int n = tid + u * DGA_THREADS;
    if (n < N) {
      const int i = n / P, j = n - i * P;
      double v0, v00, v1, v11;
      stencils(F0, i, j, v0, v00, v1, v11);
      rabs += fabs(-K[u] * (v00 * i00) - K0[u] * (v0 * i0) - K[u] * (v11 * i11) - K1[u] * (v1 * i1) - f_s[n]);
    }
    DGA_POINT_FENCE();
  }
  if (tid < NB) rabs += fabs(boundary_row(F0, tid, true));   // |-+v| = |v|
  rabs = dga_block_sum(rabs, red);
  cp = dga_block_sum(cp, red);
  if (tid == 0) {
    if (res_mean) res_mean[b] = (rabs + fabs(cp)) / (double)(N + NB + 1);
    if (iters_out) iters_out[b] = it;
    if (relres_out) relres_out[b] = gamma0 > 0.0 ? sqrt(gamma / gamma0) : 0.0;
    stI[0] = it;
    stI[1] = 1;
    done_out[b] = 1;
  }
}

template <int ACC>
static int dga_launch(const double* basis, const double* z, int q, const double* K_in, int P, double d0, double d1, double bc_sign,
                      const double* int_w, const double* f_s, int max_iter, double rtol, int iters_this_launch, int first_launch,
                      double* state, double* K_out, double* p_out, double* res_mean, int32_t* iters, double* relres, int32_t* done,
                      int B, size_t lds, void* stream) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&darcy_gen_acc_kernel<ACC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)DGA_LDS_LIMIT);
    attr = true;
  }
  hipLaunchKernelGGL(darcy_gen_acc_kernel<ACC>, dim3(B), dim3(DGA_THREADS), lds, as_stream(stream), basis, z, q, K_in, P, d0, d1,
                     bc_sign, int_w, f_s, max_iter, rtol, iters_this_launch, first_launch, state, K_out, p_out, res_mean, iters, relres,
                     done);
  PIDM_CHECK_LAUNCH("darcy_gen_acc_kernel");
  return 0;
}

}  // namespace pidm

using namespace pidm;

extern "C" size_t pidm_darcy_gen_acc_state_bytes(int P, int B) {
  if (P < 1 || B < 0) return 0;
  return (size_t)B * dga_state_doubles(P) * sizeof(double);
}

extern "C" size_t pidm_darcy_gen_acc_lds_bytes(int P, int acc) {
  if (P < 1 || (acc != 2 && acc != 4 && acc != 6)) return 0;
  return ((size_t)4 * P * P + 4 * (size_t)P + (3 * (size_t)(acc + 2) + 1) * 2 + DGA_RED) * sizeof(double);
}

extern "C" int pidm_darcy_gen_acc(const double* basis, const double* z, int q, const double* K_in, int P, int acc, double d0, double d1,
                                  double bc_sign, const double* int_w, const double* f_s, int max_iter, double rtol,
                                  int iters_this_launch, int first_launch, void* state, double* K_out, double* p_out,
                                  double* res_mean, int32_t* iters, double* relres, int32_t* done, int B, void* stream) {
  if (acc != 2 && acc != 4 && acc != 6) return fail("darcy_gen_acc: acc=%d is not one of 2, 4, 6", acc);
  const int pmin = acc == 6 ? 10 : 8;
  if (P < pmin || P > 64)
    return fail("darcy_gen_acc: P=%d outside [%d, 64] at acc=%d (a one-sided second derivative of order %d spans %d points; four "
                "fp64 fields of P^2 must fit LDS)", P, pmin, acc, acc, acc + 2);
  if (B < 0) return fail("darcy_gen_acc: B=%d must be >= 0", B);
  if (z) {
    if (!basis) return fail("darcy_gen_acc: z given without a basis");
    if (q < 1 || q > P * P) return fail("darcy_gen_acc: q=%d outside [1, P^2=%d]", q, P * P);
  } else if (!K_in) {
    return fail("darcy_gen_acc: neither z (KLE synthesis) nor K_in given");
  }
  if (!int_w || !f_s || !p_out) return fail("darcy_gen_acc: null buffer");
  if (!state) return fail("darcy_gen_acc: null state buffer (pidm_darcy_gen_acc_state_bytes(P, B) bytes)");
  if (!done) return fail("darcy_gen_acc: null done flags");
  if (iters_this_launch < 1) return fail("darcy_gen_acc: iters_this_launch=%d must be >= 1", iters_this_launch);
  if (max_iter < 0 || !(rtol > 0.0)) return fail("darcy_gen_acc: max_iter >= 0 and rtol > 0 required");
  if (!(d0 != 0.0) || !(d1 != 0.0)) return fail("darcy_gen_acc: zero grid spacing");
  const size_t lds = pidm_darcy_gen_acc_lds_bytes(P, acc);
  if (lds > DGA_LDS_LIMIT)
    return fail("darcy_gen_acc: P=%d at acc=%d needs %zu bytes of LDS, a gfx950 workgroup has %zu", P, acc, lds, DGA_LDS_LIMIT);
  if (B == 0) return 0;
  double* st = static_cast<double*>(state);
  const int fl = first_launch != 0;
#define PIDM_DGA_ARGS basis, z, q, K_in, P, d0, d1, bc_sign, int_w, f_s, max_iter, rtol, iters_this_launch, fl, st, K_out, p_out, \
                      res_mean, iters, relres, done, B, lds, stream
  if (acc == 2) return dga_launch<2>(PIDM_DGA_ARGS);
  if (acc == 4) return dga_launch<4>(PIDM_DGA_ARGS);
  return dga_launch<6>(PIDM_DGA_ARGS);
#undef PIDM_DGA_ARGS
}
