// Darcy training-data generation under periodic boundary conditions (bcs = 'periodic') at finite-difference order acc = 2, 4, 6:
// the solve of k_darcy_gen_acc.hip with every 1-D operator replaced by its central stencil on wrapped indices.
//
// Replaces (reference path): src/darcy_data_generation.py:129-163 with every FinDiff(axis, d, order, acc=acc) replaced by the
// central stencil of that order whose tap i + o reads point (i + o) mod P - the operators ResidualsDarcy(bcs='periodic') evaluates
// (the reference's generator itself has no periodic mode; main.py exposes bcs = 'periodic' for training only).  The system, the
// row order, the column scaling, the deflation by the integral row, the stopping rule and the launch protocol with its `state`
// layout are those of k_darcy_gen_acc.hip (read its header and that of k_darcy_gen.hip first); what changes is the 1-D operators:
//
//   every row i is central: acc+1 taps at columns wrap(i - mio + k), k <= acc, mio = acc / 2, for both derivatives; there are no
//   edge classes.  The four boundary row sets keep their meaning (as in the training residual): x-min = -(D0 p) on row 0, x-max =
//   +(D0 p) on row P-1, y-min = bc_sign (D1 p) on column 0, y-max = -bc_sign (D1 p) on column P-1, all with the wrapped operators.
//
// P >= 8 > acc + 1 makes the acc+1 wrapped taps of a row distinct points (at acc 6, P = 8 they are 7 of the 8) and lets one
// conditional add or subtract of P do the wrap.  One table of unit-spacing coefficients serves both axes and lives in LDS: entry
// k = (first-derivative weight, second-derivative weight) of tap k, entry acc+1 = (0, 0).  The transposed operators (column
// scales, adjoint) enumerate the rows that touch column m: exactly the acc+1 rows wrap(m - mio + c), c <= acc, row c holding tap
// acc - c at m.
#include <math.h>

#include "pidm_common.h"

namespace pidm {

constexpr int DGP_THREADS = 512;   // 8 waves: two per SIMD
constexpr int DGP_PTS = 8;         // points per lane at P = 64 (4096 / 512)
constexpr int DGP_RED = DGP_THREADS / 64;
constexpr size_t DGP_LDS_LIMIT = 160 * 1024;   // LDS of one gfx950 workgroup
// Between the points of a lane: the scheduler may not gather the LDS loads of a whole pass in front of their uses (the lane's
// eight points hold 128 registers for good; the 7 candidates x 4 values of one point at acc 6 fit next to them, those of all
// eight do not).
#define DGP_POINT_FENCE() __builtin_amdgcn_sched_barrier(0)

// k -> unit-spacing coefficients (first, second derivative) of central tap k (offset k - acc/2); the last pair is zero
template <int ACC>
struct DgpTable {
  static constexpr int NT = ACC + 1;
  double w[(NT + 1) * 2];
};
template <int ACC>
constexpr DgpTable<ACC> dgp_make_table() {
  constexpr int NT = ACC + 1;
  const double c1_2[7] = {-1.0 / 2, 0.0, 1.0 / 2, 0, 0, 0, 0};
  const double c1_4[7] = {1.0 / 12, -2.0 / 3, 0.0, 2.0 / 3, -1.0 / 12, 0, 0};
  const double c1_6[7] = {-1.0 / 60, 3.0 / 20, -3.0 / 4, 0.0, 3.0 / 4, -3.0 / 20, 1.0 / 60};
  const double c2_2[7] = {1.0, -2.0, 1.0, 0, 0, 0, 0};
  const double c2_4[7] = {-1.0 / 12, 4.0 / 3, -5.0 / 2, 4.0 / 3, -1.0 / 12, 0, 0};
  const double c2_6[7] = {1.0 / 90, -3.0 / 20, 3.0 / 2, -49.0 / 18, 3.0 / 2, -3.0 / 20, 1.0 / 90};
  const double* c1 = ACC == 2 ? c1_2 : (ACC == 4 ? c1_4 : c1_6);
  const double* c2 = ACC == 2 ? c2_2 : (ACC == 4 ? c2_4 : c2_6);
  DgpTable<ACC> t{};
  for (int k = 0; k < NT; ++k) {
    t.w[k * 2 + 0] = c1[k];
    t.w[k * 2 + 1] = c2[k];
  }
  return t;
}

// v in [-P, 2P) -> [0, P)
__device__ __forceinline__ int dgp_wrap(int v, int P) { return v < 0 ? v + P : (v >= P ? v - P : v); }

// table entry of D[e][m], the weight with which row e of a wrapped central operator reads column m (the zero entry acc+1 when it
// does not reach m)
template <int ACC>
__device__ __forceinline__ int dgp_entry(int e, int m, int P) {
  constexpr int MIO = ACC / 2;
  int o = m - e;                         // in (-P, P); the row's taps are the offsets -mio .. mio modulo P
  o = o > MIO ? o - P : (o < -MIO ? o + P : o);
  return o >= -MIO && o <= MIO ? o + MIO : ACC + 1;
}

__device__ __forceinline__ double dgp_block_sum(double v, double* red) {   // all DGP_THREADS lanes; result broadcast
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < DGP_RED; ++w) s += red[w];
  return s;
}

// doubles of one sample's state - the layout of k_darcy_gen_acc.hip (pidm_darcy_gen_acc_state_bytes sizes the buffer of both):
// iterate | search direction | row residuals (P^2 each) | boundary residuals (4P) | gamma | gamma0 | two int32 (iterations, done)
__host__ __device__ inline size_t dgp_state_doubles(int P) { return (size_t)3 * P * P + 4 * (size_t)P + 3; }

// LDS (doubles): F0 | F1 | F2 | Y (P^2 each) | RB (4P) | TAB ((acc + 2) * 2) | RED (8)
template <int ACC>
__global__ void __launch_bounds__(DGP_THREADS)
    darcy_gen_per_kernel(const double* __restrict__ basis, const double* __restrict__ z, int q, const double* __restrict__ K_in, int P,
                         double d0, double d1, double bc_sign, const double* __restrict__ int_w, const double* __restrict__ f_s,
                         int max_iter, double rtol, int iters_this_launch, int first_launch, double* __restrict__ state,
                         double* __restrict__ K_out, double* __restrict__ p_out, double* __restrict__ res_mean,
                         int32_t* __restrict__ iters_out, double* __restrict__ relres_out, int32_t* __restrict__ done_out) {
  constexpr int NT = ACC + 1, MIO = ACC / 2;
  HIP_DYNAMIC_SHARED(double, smem)
  const int b = blockIdx.x, tid = threadIdx.x, N = P * P, NB = 4 * P;
  double* st = state + (size_t)b * dgp_state_doubles(P);
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
  double* red = TAB + (NT + 1) * 2;
  const double i0 = 1.0 / d0, i00 = 1.0 / (d0 * d0), i1 = 1.0 / d1, i11 = 1.0 / (d1 * d1);

  // ---- prologue (every launch): coefficient table, K = exp(B z) (or K_in), K_0, K_1, column scales -------------------------
  if (tid == 0) {
    constexpr DgpTable<ACC> tab = dgp_make_table<ACC>();
#pragma unroll
    for (int e = 0; e < (NT + 1) * 2; ++e) TAB[e] = tab.w[e];
  }
  double K[DGP_PTS], K0[DGP_PTS], K1[DGP_PTS], sc[DGP_PTS];
#pragma unroll
  for (int u = 0; u < DGP_PTS; ++u) {
    const int n = tid + u * DGP_THREADS;
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
    v0 = v00 = v1 = v11 = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const double xa = F[dgp_wrap(i - MIO + k, P) * P + j], xb = F[i * P + dgp_wrap(j - MIO + k, P)];
      const double w1 = TAB[2 * k], w2 = TAB[2 * k + 1];
      v0 += w1 * xa;
      v00 += w2 * xa;
      v1 += w1 * xb;
      v11 += w2 * xb;
    }
  };
  // boundary row tq (< 4P) applied to the field F: x-min / x-max rows (0 | P-1, t) = -+ D0, y-min / y-max rows (t, 0 | P-1) =
  // +- bc_sign D1 (without the sign when `plain`)
  auto boundary_row = [&](const double* F, int tq, bool plain) -> double {
    const int side = tq / P, t = tq - side * P;
    const int e = side & 1 ? P - 1 : 0;
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int col = dgp_wrap(e - MIO + k, P);
      v += TAB[2 * k] * (side < 2 ? F[col * P + t] : F[t * P + col]);
    }
    v *= side < 2 ? i0 : i1;
    if (plain) return v;
    return side == 0 ? -v : (side == 1 ? v : (side == 2 ? bc_sign * v : -bc_sign * v));
  };

#pragma unroll
  for (int u = 0; u < DGP_PTS; ++u) {
    const int n = tid + u * DGP_THREADS;
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
    DGP_POINT_FENCE();
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < DGP_PTS; ++u) {
    const int n = tid + u * DGP_THREADS;
    if (n < N) { F1[n] = K0[u]; F2[n] = K1[u]; }
  }
  __syncthreads();
  // ||A_bc e_m||^2, m = (a, bb): the rows (i, bb) whose axis-0 stencil touches a (row (a, bb), candidate mio, also carries the axis-1
  // diagonal), the rows (a, j != bb) whose axis-1 stencil touches bb, and the four boundary rows that touch m
#pragma unroll
  for (int u = 0; u < DGP_PTS; ++u) {
    const int n = tid + u * DGP_THREADS;
    double s2 = 1.0;
    if (n < N) {
      const int a = n / P, bb = n - a * P;
      s2 = 0.0;
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        const double w1 = TAB[2 * (ACC - c)], w2 = TAB[2 * (ACC - c) + 1];
        {
          const int r = dgp_wrap(a - MIO + c, P) * P + bb;
          double v = -F0[r] * (w2 * i00) - F1[r] * (w1 * i0);
          if (c == MIO) v += -F0[r] * (w2 * i11) - F2[r] * (w1 * i1);
          s2 += v * v;
        }
        if (c != MIO) {
          const int r = a * P + dgp_wrap(bb - MIO + c, P);
          const double v = -F0[r] * (w2 * i11) - F2[r] * (w1 * i1);
          s2 += v * v;
        }
      }
      double w;
      w = TAB[2 * dgp_entry<ACC>(0, a, P)] * i0;          // x-min row (0, bb)
      s2 += w * w;
      w = TAB[2 * dgp_entry<ACC>(P - 1, a, P)] * i0;      // x-max row (P-1, bb)
      s2 += w * w;
      w = TAB[2 * dgp_entry<ACC>(0, bb, P)] * i1;         // y-min row (a, 0)
      s2 += w * w;
      w = TAB[2 * dgp_entry<ACC>(P - 1, bb, P)] * i1;     // y-max row (a, P-1)
      s2 += w * w;
    }
    sc[u] = 1.0 / sqrt(s2);
    DGP_POINT_FENCE();
  }

  // ---- CGLS on A_bc S ---------------------------------------------------------------------------------------------------
  double ph[DGP_PTS], s[DGP_PTS], r[DGP_PTS];
  double rb = 0.0;                               // boundary row tid (tid < 4P)

  // s = S A_bc^T r (reads F0..F2 / RB after its own barrier); returns the lane's partial ||s||^2
  auto adjoint = [&](int tq) -> double {
    PIDM_OPAQUE_I32(tq);   // (nor may the indices of the forward pass stay live for the transposed one)
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) {
      const int n = tq + u * DGP_THREADS;
      if (n < N) { F0[n] = K[u] * r[u]; F1[n] = K0[u] * r[u]; F2[n] = K1[u] * r[u]; }
    }
    if (tq < NB) RB[tq] = rb;
    __syncthreads();
    double part = 0.0;
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) {
      const int n = tq + u * DGP_THREADS;
      double v = 0.0;
      if (n < N) {
        const int a = n / P, bb = n - a * P;
        double s0 = 0.0, s00 = 0.0, s1 = 0.0, s11 = 0.0;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
          const double w1 = TAB[2 * (ACC - c)], w2 = TAB[2 * (ACC - c) + 1];
          const int ra = dgp_wrap(a - MIO + c, P) * P + bb, rr = a * P + dgp_wrap(bb - MIO + c, P);
          s00 += w2 * F0[ra];
          s0 += w1 * F1[ra];
          s11 += w2 * F0[rr];
          s1 += w1 * F2[rr];
        }
        v = -(s00 * i00 + s0 * i0 + s11 * i11 + s1 * i1);
        // boundary rows: x-min (0, bb) = -D0 row 0, x-max (P-1, bb) = +D0 row P-1, y-min (a, 0) = bc_sign D1 row 0, y-max -bc_sign
        v -= TAB[2 * dgp_entry<ACC>(0, a, P)] * i0 * RB[bb];
        v += TAB[2 * dgp_entry<ACC>(P - 1, a, P)] * i0 * RB[P + bb];
        v += bc_sign * (TAB[2 * dgp_entry<ACC>(0, bb, P)] * i1) * RB[2 * P + a];
        v -= bc_sign * (TAB[2 * dgp_entry<ACC>(P - 1, bb, P)] * i1) * RB[3 * P + a];
        v *= sc[u];
      }
      s[u] = v;
      part += v * v;
      DGP_POINT_FENCE();
    }
    return part;
  };

  double gamma, gamma0;
  int it;
  __syncthreads();                               // (every read of the column-scale pass is done before F0..F2 are rewritten)
  if (first_launch) {
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) {
      const int n = tid + u * DGP_THREADS;
      if (n < N) Y[n] = 0.0;
      r[u] = n < N ? f_s[n] : 0.0;
    }
    gamma = dgp_block_sum(adjoint(tid), red);
    gamma0 = gamma;
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) ph[u] = s[u];
    it = 0;
  } else {
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) {
      const int n = tid + u * DGP_THREADS;
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
    // index the compiler cannot see through keeps them inside: recomputing them is a few selects.
    int tq = tid;
    PIDM_OPAQUE_I32(tq);
    // q = A_bc S p_hat
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) {
      const int n = tq + u * DGP_THREADS;
      if (n < N) F0[n] = sc[u] * ph[u];
    }
    __syncthreads();
    double qb = 0.0, part = 0.0;
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) {
      const int n = tq + u * DGP_THREADS;
      double v = 0.0;
      if (n < N) {
        const int i = n / P, j = n - i * P;
        double v0, v00, v1, v11;
        stencils(F0, i, j, v0, v00, v1, v11);
        v = -K[u] * (v00 * i00) - K0[u] * (v0 * i0) - K[u] * (v11 * i11) - K1[u] * (v1 * i1);
      }
      if (n < N) F1[n] = v;   // (lane-private until the adjoint rewrites F1: the lane reads it back after the reduction)
      part += v * v;
      DGP_POINT_FENCE();
    }
    if (tq < NB) {
      qb = boundary_row(F0, tq, false);
      part += qb * qb;
    }
    const double delta = dgp_block_sum(part, red);   // (its barriers also retire every read of S p_hat)
    const double alpha = delta > 0.0 ? gamma / delta : 0.0;
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) {
      const int n = tq + u * DGP_THREADS;
      if (n < N) {
        Y[n] += alpha * ph[u];
        r[u] -= alpha * F1[n];
      }
    }
    rb -= alpha * qb;
    const double gnew = dgp_block_sum(adjoint(tq), red);
    const double beta = gnew / gamma;
    gamma = gnew;
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) ph[u] = s[u] + beta * ph[u];
  }

  if (it < max_iter && gamma > stop) {
    // ---- not finished: leave the state for the next launch --------------------------------------------------------------
#pragma unroll
    for (int u = 0; u < DGP_PTS; ++u) {
      const int n = tid + u * DGP_THREADS;
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
  for (int u = 0; u < DGP_PTS; ++u) {
    const int n = tid + u * DGP_THREADS;
    if (n < N) {
      const double x = Y[n] * sc[u];
      Y[n] = x;
      cx += int_w[n] * x;
      c1 += int_w[n];
    }
  }
  cx = dgp_block_sum(cx, red);
  c1 = dgp_block_sum(c1, red);
  const double shift = cx / c1;
  double cp = 0.0;
#pragma unroll
  for (int u = 0; u < DGP_PTS; ++u) {
    const int n = tid + u * DGP_THREADS;
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
  for (int u = 0; u < DGP_PTS; ++u) {
    const int n = tid + u * DGP_THREADS;
    if (n < N) {
      const int i = n / P, j = n - i * P;
      double v0, v00, v1, v11;
      stencils(F0, i, j, v0, v00, v1, v11);
      rabs += fabs(-K[u] * (v00 * i00) - K0[u] * (v0 * i0) - K[u] * (v11 * i11) - K1[u] * (v1 * i1) - f_s[n]);
    }
    DGP_POINT_FENCE();
  }
  if (tid < NB) rabs += fabs(boundary_row(F0, tid, true));   // |-+v| = |v|
  rabs = dgp_block_sum(rabs, red);
  cp = dgp_block_sum(cp, red);
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
static int dgp_launch(const double* basis, const double* z, int q, const double* K_in, int P, double d0, double d1, double bc_sign,
                      const double* int_w, const double* f_s, int max_iter, double rtol, int iters_this_launch, int first_launch,
                      double* state, double* K_out, double* p_out, double* res_mean, int32_t* iters, double* relres, int32_t* done,
                      int B, size_t lds, void* stream) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&darcy_gen_per_kernel<ACC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)DGP_LDS_LIMIT);
    attr = true;
  }
  hipLaunchKernelGGL(darcy_gen_per_kernel<ACC>, dim3(B), dim3(DGP_THREADS), lds, as_stream(stream), basis, z, q, K_in, P, d0, d1,
                     bc_sign, int_w, f_s, max_iter, rtol, iters_this_launch, first_launch, state, K_out, p_out, res_mean, iters, relres,
                     done);
  PIDM_CHECK_LAUNCH("darcy_gen_per_kernel");
  return 0;
}

}  // namespace pidm

using namespace pidm;

extern "C" size_t pidm_darcy_gen_periodic_lds_bytes(int P, int acc) {
  if (P < 1 || (acc != 2 && acc != 4 && acc != 6)) return 0;
  return ((size_t)4 * P * P + 4 * (size_t)P + ((size_t)acc + 2) * 2 + DGP_RED) * sizeof(double);
}

extern "C" int pidm_darcy_gen_periodic(const double* basis, const double* z, int q, const double* K_in, int P, int acc, double d0,
                                       double d1, double bc_sign, const double* int_w, const double* f_s, int max_iter, double rtol,
                                       int iters_this_launch, int first_launch, void* state, double* K_out, double* p_out,
                                       double* res_mean, int32_t* iters, double* relres, int32_t* done, int B, void* stream) {
  if (acc != 2 && acc != 4 && acc != 6) return fail("darcy_gen_periodic: acc=%d is not one of 2, 4, 6", acc);
  if (P < 8 || P > 64)
    return fail("darcy_gen_periodic: P=%d outside [8, 64] (the wrapped stencil of order 6 spans 7 points; four fp64 fields of P^2 "
                "must fit LDS)", P);
  if (B < 0) return fail("darcy_gen_periodic: B=%d must be >= 0", B);
  if (z) {
    if (!basis) return fail("darcy_gen_periodic: z given without a basis");
    if (q < 1 || q > P * P) return fail("darcy_gen_periodic: q=%d outside [1, P^2=%d]", q, P * P);
  } else if (!K_in) {
    return fail("darcy_gen_periodic: neither z (KLE synthesis) nor K_in given");
  }
  if (!int_w || !f_s || !p_out) return fail("darcy_gen_periodic: null buffer");
  if (!state) return fail("darcy_gen_periodic: null state buffer (pidm_darcy_gen_acc_state_bytes(P, B) bytes)");
  if (!done) return fail("darcy_gen_periodic: null done flags");
  if (iters_this_launch < 1) return fail("darcy_gen_periodic: iters_this_launch=%d must be >= 1", iters_this_launch);
  if (max_iter < 0 || !(rtol > 0.0)) return fail("darcy_gen_periodic: max_iter >= 0 and rtol > 0 required");
  if (!(d0 != 0.0) || !(d1 != 0.0)) return fail("darcy_gen_periodic: zero grid spacing");
  const size_t lds = pidm_darcy_gen_periodic_lds_bytes(P, acc);
  if (lds > DGP_LDS_LIMIT)
    return fail("darcy_gen_periodic: P=%d at acc=%d needs %zu bytes of LDS, a gfx950 workgroup has %zu", P, acc, lds, DGP_LDS_LIMIT);
  if (B == 0) return 0;
  double* st = static_cast<double*>(state);
  const int fl = first_launch != 0;
#define PIDM_DGP_ARGS basis, z, q, K_in, P, d0, d1, bc_sign, int_w, f_s, max_iter, rtol, iters_this_launch, fl, st, K_out, p_out, \
                      res_mean, iters, relres, done, B, lds, stream
  if (acc == 2) return dgp_launch<2>(PIDM_DGP_ARGS);
  if (acc == 4) return dgp_launch<4>(PIDM_DGP_ARGS);
  return dgp_launch<6>(PIDM_DGP_ARGS);
#undef PIDM_DGP_ARGS
}
