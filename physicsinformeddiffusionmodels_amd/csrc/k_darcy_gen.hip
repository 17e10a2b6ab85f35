// Darcy training-data generation for gfx950: KLE permeability synthesis and the fp64 least-squares pressure solve.
//
// Replaces (reference path): src/darcy_data_generation.py:118-163 (generate_sample), which per sample assembles the dense
// (P^2+4P+1) x P^2 system  [A; boundary rows; integral row] p = [f_s; 0; 0]  with findiff and solves it with
// scipy.linalg.lstsq (7.2 s per 64x64 sample on a CPU core).  Here one workgroup per sample runs matrix-free CGLS in fp64:
//
//   A p        = -K p_00 - K_0 p_0 - K p_11 - K_1 p_1        (P^2 rows, acc-2 stencils, one-sided at the edges)
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
// region of three fp64 fields: S p_hat while A is applied, then K r | K_0 r | K_1 r (the adjoint needs the neighbours'
// coefficients: A^T r = -D00^T (K r) - D0^T (K_0 r) - D11^T (K r) - D1^T (K_1 r)) plus the 4P boundary residuals.  Two block reductions
// per iteration (||A S p_hat||^2 and ||s||^2); their barriers also order the reuse of the LDS region.
#include <math.h>

#include "pidm_common.h"

namespace pidm {

constexpr int DG_THREADS = 512;   // 8 waves: two per SIMD
constexpr int DG_PTS = 8;         // points per lane at P = 64 (4096 / 512)

// acc-2 coefficients at unit spacing (findiff) of class cls (0 low edge: taps i+k, 1 centre: taps i-1+k, 2 high
// edge: taps i-k) and tap k in [0, 4); out-of-range taps are 0.  Selects, not table loads: inside the unrolled tap loops k is a
// constant and the whole thing folds to a few v_cndmask.
__device__ __forceinline__ double dg_pick(int k, double a0, double a1, double a2, double a3) {
  return k == 0 ? a0 : (k == 1 ? a1 : (k == 2 ? a2 : (k == 3 ? a3 : 0.0)));
}
__device__ __forceinline__ double dg_c1(int cls, int k) {
  return cls == 0 ? dg_pick(k, -1.5, 2.0, -0.5, 0.0) : (cls == 2 ? dg_pick(k, 1.5, -2.0, 0.5, 0.0) : dg_pick(k, -0.5, 0.0, 0.5, 0.0));
}
__device__ __forceinline__ double dg_c2(int cls, int k) {
  return cls == 1 ? dg_pick(k, 1.0, -2.0, 1.0, 0.0) : dg_pick(k, 2.0, -5.0, 4.0, -1.0);
}

// forward taps of row i along one axis: (D a)[i] = sum_k w[k] a[idx[k]]; zero-weight taps point at i
struct DgTaps4 {
  int idx[4];
  double w1[4], w2[4];
};
__device__ __forceinline__ DgTaps4 dg_taps(int i, int P, double ih1, double ih2) {
  DgTaps4 t;
  const int cls = i == 0 ? 0 : (i == P - 1 ? 2 : 1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ix = cls == 0 ? k : (cls == 2 ? P - 1 - k : (k < 3 ? i - 1 + k : i));
    t.idx[k] = ix;
    t.w1[k] = dg_c1(cls, k) * ih1;
    t.w2[k] = dg_c2(cls, k) * ih2;
  }
  return t;
}

// D[i][m] of the first (w1) / second (w2) derivative matrix along one axis (unit spacing)
__device__ __forceinline__ void dg_coef(int i, int m, int P, double& w1, double& w2) {
  const int cls = i == 0 ? 0 : (i == P - 1 ? 2 : 1);
  const int k = cls == 0 ? m : (cls == 2 ? P - 1 - m : m - (i - 1));
  const bool ok = k >= 0 && k < (cls == 1 ? 3 : 4);
  w1 = ok ? dg_c1(cls, k) : 0.0;
  w2 = ok ? dg_c2(cls, k) : 0.0;
}

// transposed taps of column m along one axis: the rows 0, P-1, m-1, m, m+1 (in that order, as fd_taps_T in k_darcy.hip);
// rows that do not touch m get weight 0 and a clamped index
struct DgTaps5 {
  int idx[5];
  double w1[5], w2[5];
};
__device__ __forceinline__ DgTaps5 dg_taps_T(int m, int P, double ih1, double ih2) {
  DgTaps5 t;
  const int rows[5] = {0, P - 1, m - 1, m, m + 1};
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int i = rows[k];
    double a1 = 0.0, a2 = 0.0;
    const bool interior = i >= 1 && i <= P - 2;
    if (k < 2 || interior) dg_coef(i, m, P, a1, a2);
    t.w1[k] = a1 * ih1;
    t.w2[k] = a2 * ih2;
    t.idx[k] = i < 0 ? 0 : (i > P - 1 ? P - 1 : i);
  }
  return t;
}

__device__ __forceinline__ double dg_block_sum(double v, double* red) {   // all DG_THREADS lanes; result broadcast
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < DG_THREADS / 64; ++w) s += red[w];
  return s;
}

// LDS: three fields of P^2 doubles (F0 | F1 | F2), the iterate Y (P^2) and the 4P boundary residuals
__global__ void __launch_bounds__(DG_THREADS) darcy_gen_kernel(const double* __restrict__ basis, const double* __restrict__ z, int q,
                                                               const double* __restrict__ K_in, int P, double d0, double d1,
                                                               double bc_sign, const double* __restrict__ int_w,
                                                               const double* __restrict__ f_s, int max_iter, double rtol,
                                                               double* __restrict__ K_out, double* __restrict__ p_out,
                                                               double* __restrict__ res_mean, int32_t* __restrict__ iters_out,
                                                               double* __restrict__ relres_out) {
  HIP_DYNAMIC_SHARED(double, smem)
  __shared__ double red[DG_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, N = P * P, NB = 4 * P;
  double* F0 = smem;
  double* F1 = smem + N;
  double* F2 = smem + 2 * N;
  double* Y = smem + 3 * N;     // the iterate: lane-private, in LDS to keep the register file for the vectors the stencils use
  double* RB = smem + 4 * N;
  const double i0 = 1.0 / d0, i00 = 1.0 / (d0 * d0), i1 = 1.0 / d1, i11 = 1.0 / (d1 * d1);

  // ---- prologue: K = exp(B z) (or K_in), K_0, K_1, column scales ----------------------------------------------------------
  double K[DG_PTS], K0[DG_PTS], K1[DG_PTS], sc[DG_PTS];
#pragma unroll
  for (int u = 0; u < DG_PTS; ++u) {
    const int n = tid + u * DG_THREADS;
    double k = 1.0;
    if (n < N) {
      if (z) {
        const double* zb = z + (size_t)b * q;
        double g = 0.0;
        for (int kk = 0; kk < q; ++kk) g += basis[(size_t)kk * N + n] * zb[kk];
        k = exp(g);
        if (K_out) K_out[(size_t)b * N + n] = k;
      } else {
        k = K_in[(size_t)b * N + n];
        if (K_out) K_out[(size_t)b * N + n] = k;
      }
      F0[n] = k;
    }
    K[u] = k;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < DG_PTS; ++u) {
    const int n = tid + u * DG_THREADS;
    double g0 = 0.0, g1 = 0.0;
    if (n < N) {
      const int i = n / P, j = n - i * P;
      const DgTaps4 ti = dg_taps(i, P, i0, i00), tj = dg_taps(j, P, i1, i11);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g0 += ti.w1[k] * F0[ti.idx[k] * P + j];
        g1 += tj.w1[k] * F0[i * P + tj.idx[k]];
      }
    }
    K0[u] = g0;
    K1[u] = g1;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < DG_PTS; ++u) {
    const int n = tid + u * DG_THREADS;
    if (n < N) { F1[n] = K0[u]; F2[n] = K1[u]; }
  }
  __syncthreads();
  // ||A_bc e_m||^2: the rows (i, b) along axis 0 (row (a, b) also carries the axis-1 diagonal), the rows (a, j != b) along
  // axis 1, and the boundary rows that touch m.  Candidate rows are enumerated without repeats.
#pragma unroll
  for (int u = 0; u < DG_PTS; ++u) {
    const int n = tid + u * DG_THREADS;
    double s2 = 1.0;
    if (n < N) {
      const int a = n / P, bb = n - a * P;
      double w1, w2, dd1, dd2;
      dg_coef(bb, bb, P, dd1, dd2);
      s2 = 0.0;
      const int cand[5] = {a - 1, a, a + 1, (a >= 2) ? 0 : -1, (a <= P - 3) ? P - 1 : -1};
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int i = cand[k];
        if (i < 0 || i > P - 1) continue;
        dg_coef(i, a, P, w1, w2);
        const int r = i * P + bb;
        double e = -F0[r] * w2 * i00 - F1[r] * w1 * i0;
        if (i == a) e += -F0[r] * dd2 * i11 - F2[r] * dd1 * i1;
        s2 += e * e;
      }
      const int candj[5] = {bb - 1, bb + 1, (bb >= 2) ? 0 : -1, (bb <= P - 3) ? P - 1 : -1, -1};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = candj[k];
        if (j < 0 || j > P - 1) continue;
        dg_coef(j, bb, P, w1, w2);
        const int r = a * P + j;
        const double e = -F0[r] * w2 * i11 - F2[r] * w1 * i1;
        s2 += e * e;
      }
      dg_coef(0, a, P, w1, w2);
      s2 += (w1 * i0) * (w1 * i0);                       // x-min row (0, bb)
      dg_coef(P - 1, a, P, w1, w2);
      s2 += (w1 * i0) * (w1 * i0);                       // x-max row (P-1, bb)
      dg_coef(0, bb, P, w1, w2);
      s2 += (w1 * i1) * (w1 * i1);                       // y-min row (a, 0)
      dg_coef(P - 1, bb, P, w1, w2);
      s2 += (w1 * i1) * (w1 * i1);                       // y-max row (a, P-1)
    }
    sc[u] = 1.0 / sqrt(s2);
  }

  // ---- CGLS on A_bc S ---------------------------------------------------------------------------------------------------
  double ph[DG_PTS], s[DG_PTS], r[DG_PTS];
  double rb = 0.0;                               // boundary row tid (tid < 4P)
#pragma unroll
  for (int u = 0; u < DG_PTS; ++u) {
    const int n = tid + u * DG_THREADS;
    if (n < N) Y[n] = 0.0;
    r[u] = n < N ? f_s[n] : 0.0;
  }

  // s = S A_bc^T r (reads F0..F2 / RB after the caller's barrier); returns the lane's partial ||s||^2
  auto adjoint = [&](int tq) -> double {
#pragma unroll
    for (int u = 0; u < DG_PTS; ++u) {
      const int n = tq + u * DG_THREADS;
      if (n < N) { F0[n] = K[u] * r[u]; F1[n] = K0[u] * r[u]; F2[n] = K1[u] * r[u]; }
    }
    if (tq < NB) RB[tq] = rb;
    __syncthreads();
    double part = 0.0;
#pragma unroll
    for (int u = 0; u < DG_PTS; ++u) {
      const int n = tq + u * DG_THREADS;
      double v = 0.0;
      if (n < N) {
        const int a = n / P, bb = n - a * P;
        const DgTaps5 ta = dg_taps_T(a, P, i0, i00), tb = dg_taps_T(bb, P, i1, i11);
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const int ra = ta.idx[k] * P + bb, rr = a * P + tb.idx[k];
          acc += ta.w2[k] * F0[ra] + ta.w1[k] * F1[ra];
          acc += tb.w2[k] * F0[rr] + tb.w1[k] * F2[rr];
        }
        v = -acc;
        // boundary rows: x-min (0, bb) = -D0 row 0, x-max (P-1, bb) = +D0 row P-1, y-min (a, 0) = bc_sign D1 row 0, y-max -bc_sign
        double w1, w2;
        dg_coef(0, a, P, w1, w2);
        v -= w1 * i0 * RB[bb];
        dg_coef(P - 1, a, P, w1, w2);
        v += w1 * i0 * RB[P + bb];
        dg_coef(0, bb, P, w1, w2);
        v += bc_sign * w1 * i1 * RB[2 * P + a];
        dg_coef(P - 1, bb, P, w1, w2);
        v -= bc_sign * w1 * i1 * RB[3 * P + a];
        v *= sc[u];
      }
      s[u] = v;
      part += v * v;
    }
    return part;
  };

  __syncthreads();                               // (every read of the column-scale pass is done before F0..F2 are rewritten)
  double gamma = dg_block_sum(adjoint(tid), red);
  const double gamma0 = gamma;
#pragma unroll
  for (int u = 0; u < DG_PTS; ++u) ph[u] = s[u];
  const double stop = rtol * rtol * gamma0;
  int it = 0;
  for (; it < max_iter && gamma > stop; ++it) {
    // The stencil taps and weights of a lane's points depend on the point only; hoisted out of the loop they take ~600 VGPRs for
    // eight points.  An index the compiler cannot see through keeps them inside: recomputing them is a few selects.
    int tq = tid;
    PIDM_OPAQUE_I32(tq);
    // q = A_bc S p_hat
#pragma unroll
    for (int u = 0; u < DG_PTS; ++u) {
      const int n = tq + u * DG_THREADS;
      if (n < N) F0[n] = sc[u] * ph[u];
    }
    __syncthreads();
    double aq[DG_PTS], qb = 0.0, part = 0.0;
#pragma unroll
    for (int u = 0; u < DG_PTS; ++u) {
      const int n = tq + u * DG_THREADS;
      double v = 0.0;
      if (n < N) {
        const int i = n / P, j = n - i * P;
        const DgTaps4 ti = dg_taps(i, P, i0, i00), tj = dg_taps(j, P, i1, i11);
        double v0 = 0.0, v00 = 0.0, v1 = 0.0, v11 = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double xa = F0[ti.idx[k] * P + j], xb = F0[i * P + tj.idx[k]];
          v0 += ti.w1[k] * xa;
          v00 += ti.w2[k] * xa;
          v1 += tj.w1[k] * xb;
          v11 += tj.w2[k] * xb;
        }
        v = -K[u] * v00 - K0[u] * v0 - K[u] * v11 - K1[u] * v1;
      }
      aq[u] = v;
      part += v * v;
    }
    if (tq < NB) {
      const int side = tq / P, t = tq - side * P;
      double v = 0.0;
      if (side < 2) {   // x-min / x-max rows (0 | P-1, t): -+ D0
        const int i = side == 0 ? 0 : P - 1;
        const DgTaps4 ti = dg_taps(i, P, i0, i00);
#pragma unroll
        for (int k = 0; k < 4; ++k) v += ti.w1[k] * F0[ti.idx[k] * P + t];
        v = side == 0 ? -v : v;
      } else {          // y-min / y-max rows (t, 0 | P-1): +- bc_sign D1
        const int j = side == 2 ? 0 : P - 1;
        const DgTaps4 tj = dg_taps(j, P, i1, i11);
#pragma unroll
        for (int k = 0; k < 4; ++k) v += tj.w1[k] * F0[t * P + tj.idx[k]];
        v = side == 2 ? bc_sign * v : -bc_sign * v;
      }
      qb = v;
      part += v * v;
    }
    const double delta = dg_block_sum(part, red);   // (its barriers also retire every read of S p_hat)
    const double alpha = delta > 0.0 ? gamma / delta : 0.0;
#pragma unroll
    for (int u = 0; u < DG_PTS; ++u) {
      const int n = tq + u * DG_THREADS;
      if (n < N) Y[n] += alpha * ph[u];
      r[u] -= alpha * aq[u];
    }
    rb -= alpha * qb;
    const double gnew = dg_block_sum(adjoint(tq), red);
    const double beta = gnew / gamma;
    gamma = gnew;
#pragma unroll
    for (int u = 0; u < DG_PTS; ++u) ph[u] = s[u] + beta * ph[u];
  }

  // ---- deflation: p = S y - (c . S y / c . 1) 1, then the residual of all P^2 + 4P + 1 rows ---------------------------------
  double cx = 0.0, c1 = 0.0;
#pragma unroll
  for (int u = 0; u < DG_PTS; ++u) {
    const int n = tid + u * DG_THREADS;
    if (n < N) {
      const double x = Y[n] * sc[u];
      Y[n] = x;
      cx += int_w[n] * x;
      c1 += int_w[n];
    }
  }
  cx = dg_block_sum(cx, red);
  c1 = dg_block_sum(c1, red);
  const double shift = cx / c1;
  double cp = 0.0;
#pragma unroll
  for (int u = 0; u < DG_PTS; ++u) {
    const int n = tid + u * DG_THREADS;
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
  for (int u = 0; u < DG_PTS; ++u) {
    const int n = tid + u * DG_THREADS;
    if (n < N) {
      const int i = n / P, j = n - i * P;
      const DgTaps4 ti = dg_taps(i, P, i0, i00), tj = dg_taps(j, P, i1, i11);
      double v0 = 0.0, v00 = 0.0, v1 = 0.0, v11 = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double xa = F0[ti.idx[k] * P + j], xb = F0[i * P + tj.idx[k]];
        v0 += ti.w1[k] * xa;
        v00 += ti.w2[k] * xa;
        v1 += tj.w1[k] * xb;
        v11 += tj.w2[k] * xb;
      }
      rabs += fabs(-K[u] * v00 - K0[u] * v0 - K[u] * v11 - K1[u] * v1 - f_s[n]);
    }
  }
  if (tid < NB) {
    const int side = tid / P, t = tid - side * P;
    double v = 0.0;
    if (side < 2) {
      const DgTaps4 ti = dg_taps(side == 0 ? 0 : P - 1, P, i0, i00);
#pragma unroll
      for (int k = 0; k < 4; ++k) v += ti.w1[k] * F0[ti.idx[k] * P + t];
    } else {
      const DgTaps4 tj = dg_taps(side == 2 ? 0 : P - 1, P, i1, i11);
#pragma unroll
      for (int k = 0; k < 4; ++k) v += tj.w1[k] * F0[t * P + tj.idx[k]];
    }
    rabs += fabs(v);   // |-+v| = |v|
  }
  rabs = dg_block_sum(rabs, red);
  cp = dg_block_sum(cp, red);
  if (tid == 0) {
    if (res_mean) res_mean[b] = (rabs + fabs(cp)) / (double)(N + NB + 1);
    if (iters_out) iters_out[b] = it;
    if (relres_out) relres_out[b] = gamma0 > 0.0 ? sqrt(gamma / gamma0) : 0.0;
  }
}

}  // namespace pidm

using namespace pidm;

extern "C" size_t pidm_darcy_gen_lds_bytes(int P) { return ((size_t)4 * P * P + 4 * (size_t)P) * sizeof(double); }

extern "C" int pidm_darcy_gen(const double* basis, const double* z, int q, const double* K_in, int P, double d0, double d1,
                              double bc_sign, const double* int_w, const double* f_s, int max_iter, double rtol, double* K_out,
                              double* p_out, double* res_mean, int32_t* iters, double* relres, int B, void* stream) {
  if (P < 8 || P > 64) return fail("darcy_gen: P=%d outside [8, 64] (four fp64 fields of P^2 must fit LDS)", P);
  if (B < 0) return fail("darcy_gen: B=%d must be >= 0", B);
  if (z) {
    if (!basis) return fail("darcy_gen: z given without a basis");
    if (q < 1 || q > P * P) return fail("darcy_gen: q=%d outside [1, P^2=%d]", q, P * P);
  } else if (!K_in) {
    return fail("darcy_gen: neither z (KLE synthesis) nor K_in given");
  }
  if (!int_w || !f_s || !p_out) return fail("darcy_gen: null buffer");
  if (max_iter < 0 || !(rtol > 0.0)) return fail("darcy_gen: max_iter >= 0 and rtol > 0 required");
  if (!(d0 != 0.0) || !(d1 != 0.0)) return fail("darcy_gen: zero grid spacing");
  if (B == 0) return 0;
  const size_t lds = pidm_darcy_gen_lds_bytes(P);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&darcy_gen_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL(darcy_gen_kernel, dim3(B), dim3(DG_THREADS), lds, as_stream(stream), basis, z, q, K_in, P, d0, d1, bc_sign, int_w,
                     f_s, max_iter, rtol, K_out, p_out, res_mean, iters, relres);
  PIDM_CHECK_LAUNCH("darcy_gen_kernel");
  return 0;
}
