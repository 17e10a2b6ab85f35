// Darcy training-data generation at finite-difference order acc = 2, 4, 6: the solve of k_darcy_gen_cgls.h with findiff's classed
// operators of any of the three orders.
//
// Replaces (reference path): src/darcy_data_generation.py:129-163 with `acc` as the reference passes it to every
// FinDiff(..., acc=acc).  The solve itself - system, row order, column scaling, deflation, stopping rule, launch protocol - is
// darcy_gen_cgls_body of k_darcy_gen_cgls.h (read its header first); this file holds the 1-D operators, ClassedOps<ACC>:
//
//   rows i < mio use the forward stencil (taps i .. i+n-1), rows i > P-1-mio the backward one (taps i-n+1 .. i), all others the
//   central one (taps i-mio .. i+mio), mio = acc / 2 for both derivatives; central stencils have acc+1 taps, one-sided first
//   derivatives acc+1, one-sided second derivatives acc+2 (grad_utils.fd_offsets / fd_coefficients state the same rule).
//
// One table of unit-spacing coefficients serves both axes and lives in LDS: entry (class, k) = (first-derivative weight, second-
// derivative weight) of the tap at column base(i) + k, k < NT = acc+2, base = i (low class), i - mio (central), i - (acc+1) (high);
// taps a stencil does not have carry weight 0.  The transposed operators (column scales, adjoint) enumerate the rows that touch
// column m by class, each exactly once: the acc+1 central rows m-mio .. m+mio that ARE central rows, the mio low-edge rows and the
// mio high-edge rows - 2 acc + 1 candidates, whatever P.
#include <stdio.h>

#include "k_darcy_gen_cgls.h"

namespace pidm {

// (class, k, derivative) -> unit-spacing coefficient, classes 0 low / 1 central / 2 high; see the header
template <int ACC>
struct DgaTable {
  static constexpr int NT = ACC + 2;
  double w[(3 * NT + 1) * 2];   // (the last pair is zero)
};
template <int ACC>
constexpr DgaTable<ACC> dga_make_table() {
  constexpr int NT = ACC + 2;
  // forward first / second derivative (acc+1 / acc+2 taps); the backward stencils are the mirrored forward ones (first
  // derivative: negated)
  const double f1_2[8] = {-3.0 / 2, 2.0, -1.0 / 2, 0, 0, 0, 0, 0};
  const double f1_4[8] = {-25.0 / 12, 4.0, -3.0, 4.0 / 3, -1.0 / 4, 0, 0, 0};
  const double f1_6[8] = {-49.0 / 20, 6.0, -15.0 / 2, 20.0 / 3, -15.0 / 4, 6.0 / 5, -1.0 / 6, 0};
  const double f2_2[8] = {2.0, -5.0, 4.0, -1.0, 0, 0, 0, 0};
  const double f2_4[8] = {15.0 / 4, -77.0 / 6, 107.0 / 6, -13.0, 61.0 / 12, -5.0 / 6, 0, 0};
  const double f2_6[8] = {469.0 / 90, -223.0 / 10, 879.0 / 20, -949.0 / 18, 41.0, -201.0 / 10, 1019.0 / 180, -7.0 / 10};
  const double* f1 = ACC == 2 ? f1_2 : (ACC == 4 ? f1_4 : f1_6);
  const double* f2 = ACC == 2 ? f2_2 : (ACC == 4 ? f2_4 : f2_6);
  DgaTable<ACC> t{};
  for (int k = 0; k < NT; ++k) {
    const int j = ACC + 1 - k;   // high class: tap k sits at offset -j
    t.w[(0 * NT + k) * 2 + 0] = f1[k];
    t.w[(0 * NT + k) * 2 + 1] = f2[k];
    t.w[(1 * NT + k) * 2 + 0] = k <= ACC ? dgc_central(ACC, 1, k) : 0.0;
    t.w[(1 * NT + k) * 2 + 1] = k <= ACC ? dgc_central(ACC, 2, k) : 0.0;
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

// the operator set of darcy_gen_cgls_body (k_darcy_gen_cgls.h lists what each member is)
template <int ACC>
struct ClassedOps {
  static constexpr int NT = ACC + 2, NC = 2 * ACC + 1;
  static constexpr int TAB_DOUBLES = (3 * NT + 1) * 2;

  static __device__ __forceinline__ void fill(double* TAB) {
    constexpr DgaTable<ACC> tab = dga_make_table<ACC>();
#pragma unroll
    for (int e = 0; e < TAB_DOUBLES; ++e) TAB[e] = tab.w[e];
  }

  static __device__ __forceinline__ void taps(const double* TAB, int P, const double* F, int i, int j, double& v0, double& v00,
                                              double& v1, double& v11) {
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
      if (k % 4 == 3) DGC_POINT_FENCE();
    }
  }

  static __device__ __forceinline__ double boundary_sum(const double* TAB, int P, const double* F, int side, int e, int t) {
    int ce, be;
    dga_row<ACC>(e, P, ce, be);
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int col = dga_clamp(be + k, P);
      v += TAB[(ce * NT + k) * 2] * (side < 2 ? F[col * P + t] : F[t * P + col]);
    }
    return v;
  }

  // the rows (i, bb) whose axis-0 stencil touches a (row (a, bb) also carries the axis-1 diagonal) and the rows (a, j != bb) whose
  // axis-1 stencil touches bb
  static __device__ __forceinline__ double pde_colnorm2(const double* TAB, int P, const double* F0, const double* F1,
                                                        const double* F2, int a, int bb, double i0, double i00, double i1,
                                                        double i11) {
    int cb, bsb;
    dga_row<ACC>(bb, P, cb, bsb);
    const double dd1 = TAB[(cb * NT + (bb - bsb)) * 2], dd2 = TAB[(cb * NT + (bb - bsb)) * 2 + 1];
    double s2 = 0.0;
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
      if (c % 3 == 2) DGC_POINT_FENCE();
    }
    return s2;
  }

  static __device__ __forceinline__ double d1(const double* TAB, int P, bool last, int m) {
    int i, e;
    dga_cand<ACC>(last ? dga_cand_last<ACC>() : dga_cand_first<ACC>(), m, P, i, e);
    return TAB[2 * e];
  }

  static __device__ __forceinline__ void adjoint_sums(const double* TAB, int P, const double* F0, const double* F1, const double* F2,
                                                      int a, int bb, double& s0, double& s00, double& s1, double& s11) {
    s0 = s00 = s1 = s11 = 0.0;
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
      if (c % 3 == 2) DGC_POINT_FENCE();   // (the loads of at most three candidates in flight)
    }
  }
};

template <int ACC>
__global__ void __launch_bounds__(DGC_THREADS)
    darcy_gen_acc_kernel(const double* __restrict__ basis, const double* __restrict__ z, int q, const double* __restrict__ K_in, int P,
                         double d0, double d1, double bc_sign, const double* __restrict__ int_w, const double* __restrict__ f_s,
                         int max_iter, double rtol, int iters_this_launch, int first_launch, double* __restrict__ state,
                         double* __restrict__ K_out, double* __restrict__ p_out, double* __restrict__ res_mean,
                         int32_t* __restrict__ iters_out, double* __restrict__ relres_out, int32_t* __restrict__ done_out) {
  darcy_gen_cgls_body<ClassedOps<ACC>>(basis, z, q, K_in, P, d0, d1, bc_sign, int_w, f_s, max_iter, rtol, iters_this_launch,
                                       first_launch, state, K_out, p_out, res_mean, iters_out, relres_out, done_out);
}

}  // namespace pidm

using namespace pidm;

extern "C" size_t pidm_darcy_gen_acc_state_bytes(int P, int B) {
  if (P < 1 || B < 0) return 0;
  return (size_t)B * dgc_state_doubles(P) * sizeof(double);
}

extern "C" size_t pidm_darcy_gen_acc_lds_bytes(int P, int acc) {
  if (P < 1 || (acc != 2 && acc != 4 && acc != 6)) return 0;
  return dgc_lds_bytes(P, (3 * (size_t)(acc + 2) + 1) * 2);
}

extern "C" int pidm_darcy_gen_acc(const double* basis, const double* z, int q, const double* K_in, int P, int acc, double d0, double d1,
                                  double bc_sign, const double* int_w, const double* f_s, int max_iter, double rtol,
                                  int iters_this_launch, int first_launch, void* state, double* K_out, double* p_out,
                                  double* res_mean, int32_t* iters, double* relres, int32_t* done, int B, void* stream) {
  char p_note[160];
  snprintf(p_note, sizeof p_note, " at acc=%d (a one-sided second derivative of order %d spans %d points; four fp64 fields of P^2 "
           "must fit LDS)", acc, acc, acc + 2);
  return darcy_gen_entry<darcy_gen_acc_kernel<2>, darcy_gen_acc_kernel<4>, darcy_gen_acc_kernel<6>>(
      "darcy_gen_acc", "darcy_gen_acc_kernel", acc == 6 ? 10 : 8, p_note, pidm_darcy_gen_acc_lds_bytes(P, acc), basis, z, q, K_in, P,
      acc, d0, d1, bc_sign, int_w, f_s, max_iter, rtol, iters_this_launch, first_launch, state, K_out, p_out, res_mean, iters, relres,
      done, B, stream);
}
