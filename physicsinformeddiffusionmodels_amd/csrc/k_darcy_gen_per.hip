// Darcy training-data generation under periodic boundary conditions (bcs = 'periodic') at finite-difference order acc = 2, 4, 6:
// the solve of k_darcy_gen_acc.hip with every 1-D operator replaced by its central stencil on wrapped indices.
//
// Replaces (reference path): src/darcy_data_generation.py:129-163 with every FinDiff(axis, d, order, acc=acc) replaced by the
// central stencil of that order whose tap i + o reads point (i + o) mod P - the operators ResidualsDarcy(bcs='periodic') evaluates
// (the reference's generator itself has no periodic mode; main.py exposes bcs = 'periodic' for training only).  The solve itself -
// system, row order, column scaling, deflation, stopping rule, launch protocol with its `state` layout - is darcy_gen_cgls_body
// of k_darcy_gen_cgls.h, shared with k_darcy_gen_acc.hip (read its header first); this file holds the 1-D operators, WrappedOps<ACC>:
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
#include "k_darcy_gen_cgls.h"

namespace pidm {

// k -> unit-spacing coefficients (first, second derivative) of central tap k (offset k - acc/2); the last pair is zero
template <int ACC>
struct DgpTable {
  static constexpr int NT = ACC + 1;
  double w[(NT + 1) * 2];
};
template <int ACC>
constexpr DgpTable<ACC> dgp_make_table() {
  DgpTable<ACC> t{};
  for (int k = 0; k < ACC + 1; ++k) {
    t.w[k * 2 + 0] = dgc_central(ACC, 1, k);
    t.w[k * 2 + 1] = dgc_central(ACC, 2, k);
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

// the operator set of darcy_gen_cgls_body (k_darcy_gen_cgls.h lists what each member is)
template <int ACC>
struct WrappedOps {
  static constexpr int NT = ACC + 1, MIO = ACC / 2;
  static constexpr int TAB_DOUBLES = (NT + 1) * 2;

  static __device__ __forceinline__ void fill(double* TAB) {
    constexpr DgpTable<ACC> tab = dgp_make_table<ACC>();
#pragma unroll
    for (int e = 0; e < TAB_DOUBLES; ++e) TAB[e] = tab.w[e];
  }

  static __device__ __forceinline__ void taps(const double* TAB, int P, const double* F, int i, int j, double& v0, double& v00,
                                              double& v1, double& v11) {
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
  }

  static __device__ __forceinline__ double boundary_sum(const double* TAB, int P, const double* F, int side, int e, int t) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int col = dgp_wrap(e - MIO + k, P);
      v += TAB[2 * k] * (side < 2 ? F[col * P + t] : F[t * P + col]);
    }
    return v;
  }

  // the rows (i, bb) whose axis-0 stencil touches a (row (a, bb), candidate mio, also carries the axis-1 diagonal) and the rows
  // (a, j != bb) whose axis-1 stencil touches bb
  static __device__ __forceinline__ double pde_colnorm2(const double* TAB, int P, const double* F0, const double* F1,
                                                        const double* F2, int a, int bb, double i0, double i00, double i1,
                                                        double i11) {
    double s2 = 0.0;
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
    return s2;
  }

  static __device__ __forceinline__ double d1(const double* TAB, int P, bool last, int m) {
    return TAB[2 * dgp_entry<ACC>(last ? P - 1 : 0, m, P)];
  }

  static __device__ __forceinline__ void adjoint_sums(const double* TAB, int P, const double* F0, const double* F1, const double* F2,
                                                      int a, int bb, double& s0, double& s00, double& s1, double& s11) {
    s0 = s00 = s1 = s11 = 0.0;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      const double w1 = TAB[2 * (ACC - c)], w2 = TAB[2 * (ACC - c) + 1];
      const int ra = dgp_wrap(a - MIO + c, P) * P + bb, rr = a * P + dgp_wrap(bb - MIO + c, P);
      s00 += w2 * F0[ra];
      s0 += w1 * F1[ra];
      s11 += w2 * F0[rr];
      s1 += w1 * F2[rr];
    }
  }
};

template <int ACC>
__global__ void __launch_bounds__(DGC_THREADS)
    darcy_gen_per_kernel(const double* __restrict__ basis, const double* __restrict__ z, int q, const double* __restrict__ K_in, int P,
                         double d0, double d1, double bc_sign, const double* __restrict__ int_w, const double* __restrict__ f_s,
                         int max_iter, double rtol, int iters_this_launch, int first_launch, double* __restrict__ state,
                         double* __restrict__ K_out, double* __restrict__ p_out, double* __restrict__ res_mean,
                         int32_t* __restrict__ iters_out, double* __restrict__ relres_out, int32_t* __restrict__ done_out) {
  darcy_gen_cgls_body<WrappedOps<ACC>>(basis, z, q, K_in, P, d0, d1, bc_sign, int_w, f_s, max_iter, rtol, iters_this_launch,
                                       first_launch, state, K_out, p_out, res_mean, iters_out, relres_out, done_out);
}

}  // namespace pidm

using namespace pidm;

extern "C" size_t pidm_darcy_gen_periodic_lds_bytes(int P, int acc) {
  if (P < 1 || (acc != 2 && acc != 4 && acc != 6)) return 0;
  return dgc_lds_bytes(P, ((size_t)acc + 2) * 2);
}

extern "C" int pidm_darcy_gen_periodic(const double* basis, const double* z, int q, const double* K_in, int P, int acc, double d0,
                                       double d1, double bc_sign, const double* int_w, const double* f_s, int max_iter, double rtol,
                                       int iters_this_launch, int first_launch, void* state, double* K_out, double* p_out,
                                       double* res_mean, int32_t* iters, double* relres, int32_t* done, int B, void* stream) {
  return darcy_gen_entry<darcy_gen_per_kernel<2>, darcy_gen_per_kernel<4>, darcy_gen_per_kernel<6>>(
      "darcy_gen_periodic", "darcy_gen_per_kernel", 8,
      " (the wrapped stencil of order 6 spans 7 points; four fp64 fields of P^2 must fit LDS)",
      pidm_darcy_gen_periodic_lds_bytes(P, acc), basis, z, q, K_in, P, acc, d0, d1, bc_sign, int_w, f_s, max_iter, rtol,
      iters_this_launch, first_launch, state, K_out, p_out, res_mean, iters, relres, done, B, stream);
}
