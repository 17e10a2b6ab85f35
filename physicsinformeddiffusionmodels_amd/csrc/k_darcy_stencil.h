// Second-order finite-difference taps of the Darcy kernels, shared between k_darcy.hip (residual, adjoint, fused loss) and
// k_guidance.hip (posterior guidance): the per-axis coefficient tables, their host builder and the branch-free forward and
// transposed tap builders.  One definition, so "the same taps in the same order" holds between the two files by construction.
#pragma once
#include "pidm_common.h"

namespace pidm {

// acc-2 finite-difference coefficient tables along one axis, already divided by h^order (fp32, as the
// reference stores them in its conv kernels).  class 0 = low edge (taps at +0,+1,+2[,+3]),
// class 1 = centre (taps at -1,0,+1), class 2 = high edge (taps at -0,-1,-2[,-3]).
struct FdAxis {
  float c1[3][4];
  float c2[3][4];
};

static FdAxis make_axis(double inv_h) {
  // textbook 2nd-order-accurate coefficients (what findiff.FinDiff(axis,h,order,acc=2) produces)
  static const double c1[3][3] = {{-1.5, 2.0, -0.5}, {-0.5, 0.0, 0.5}, {1.5, -2.0, 0.5}};
  static const double c2[3][4] = {{2.0, -5.0, 4.0, -1.0}, {1.0, -2.0, 1.0, 0.0}, {2.0, -5.0, 4.0, -1.0}};
  FdAxis a;
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 4; ++k) {
      a.c1[c][k] = (k < 3) ? (float)(c1[c][k] * inv_h) : 0.f;
      a.c2[c][k] = (float)(c2[c][k] * inv_h * inv_h);
    }
  return a;
}

// Branch-free stencil taps.  Forward: (D a)[i] = sum_k w[k] a[idx[k]] with 4 (position, weight) pairs chosen by the class of i
// (low edge: rows 0..3, high edge: rows P-1..P-4 in that order, interior: i-1, i, i+1 and a zero-weight fourth tap) - the same
// taps in the same order as fd_apply (k_darcy.hip), without its three code paths.  Transposed: (D^T a)[m] = sum over the (at most 5)
// stencil rows that touch column m: the interior rows m-1, m, m+1 and the two edge rows 0 and P-1; rows that do not touch m get
// weight 0.  Indices of zero-weight taps are clamped into [lo, hi] (the band's window of LDS rows; 0, P-1 for a whole field).
struct FdTaps4 {
  int idx[4];
  float w1[4], w2[4];    // first / second derivative weights
};
__device__ __forceinline__ FdTaps4 fd_taps(const FdAxis& ax, int i, int P, int lo, int hi) {
  FdTaps4 t;
  const bool low = i == 0, high = i == P - 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int ix = high ? P - 1 - k : (low ? k : i - 1 + k);
    ix = ix < lo ? lo : (ix > hi ? hi : ix);
    t.idx[k] = ix;
    const float c1i = (k < 3) ? ax.c1[1][k] : 0.f, c2i = (k < 3) ? ax.c2[1][k] : 0.f;
    t.w1[k] = high ? ax.c1[2][k] : (low ? ax.c1[0][k] : c1i);
    t.w2[k] = high ? ax.c2[2][k] : (low ? ax.c2[0][k] : c2i);
  }
  return t;
}
struct FdTaps5 {
  int idx[5];
  float w1[5], w2[5];
};
__device__ __forceinline__ FdTaps5 fd_taps_T(const FdAxis& ax, int m, int P, int lo, int hi) {
  FdTaps5 t;
  // same order as fd_apply_T (k_darcy.hip): row 0, row P-1, then the interior rows m-1, m, m+1
  const int rows[5] = {0, P - 1, m - 1, m, m + 1};
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int i = rows[k];
    float a1 = 0.f, a2 = 0.f;
    if (k == 0) {
      const int q = m < 4 ? m : 3;
      a1 = (m < 3) ? ax.c1[0][q] : 0.f;
      a2 = (m < 4) ? ax.c2[0][q] : 0.f;
    } else if (k == 1) {
      const int d = P - 1 - m, q = d < 4 ? d : 3;
      a1 = (d < 3) ? ax.c1[2][q] : 0.f;
      a2 = (d < 4) ? ax.c2[2][q] : 0.f;
    } else {
      const bool ok = (i >= 1) & (i <= P - 2);
      const int q = m - (i - 1);          // 2, 1, 0 for k = 2, 3, 4
      a1 = ok ? ax.c1[1][q] : 0.f;
      a2 = ok ? ax.c2[1][q] : 0.f;
    }
    t.w1[k] = a1;
    t.w2[k] = a2;
    t.idx[k] = i < lo ? lo : (i > hi ? hi : i);
  }
  return t;
}

}  // namespace pidm
