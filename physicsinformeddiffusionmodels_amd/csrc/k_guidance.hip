// Posterior guidance of the Darcy sampler for gfx950: the arithmetic of one guided step around the UNet.
//
// Per sample, with x = the model's x0 estimate [2,P,P] (p, K), observations y and a 0/1 mask m:
//   L_obs = sum m (x - y)^2,  L_pde = sum r(x)^2 (the three residual channels of ResidualsDarcy),
//   Phi = zeta_obs sqrt(L_obs) + zeta_pde sqrt(L_pde),
//   v = dPhi/dx = zeta_obs m (x - y) / sqrt(L_obs) + zeta_pde J^T r / sqrt(L_pde)     (a term whose L is exactly 0 is omitted).
// v is the cotangent that the UNet's input-only backward pulls to x_t; pidm_psample_update_guided then takes the ancestral step
// minus that pulled gradient.  Flux readings add a third term zeta_flux sqrt(L_flux): see "flux observations" below.
//
// guidance_cotangent_kernel (second-order, non-periodic stencils): one workgroup per sample, everything between the first read of
// x and the store of v lives in LDS.  The adjoint is LINEAR in r, so the six transposed-stencil operands are built from the
// unscaled residual in the same pass that sums r^2, and 1 / sqrt(L_pde) multiplies the gathered result: the residual is never
// written out and never re-read.  LDS plan (floats, F = P*P): p | K | -K r | a0 | a1 | b0 | b1 | d  = 8 F (128 KiB at P = 64) +
// 2 x 4 doubles of the block sums.  Same taps, same order as darcy_kernel (k_darcy.hip): its adjoint figures carry over.
// The two sums are fp64: a thread adds its pixels in index order, then a fixed shuffle tree and four wave sums - no atomics, the
// same bits run to run and for any batch size (a sample never sees another one).
#include "pidm_common.h"

namespace pidm {

struct GdAxis {          // acc-2 coefficients / h^order: class 0 low edge, 1 centre, 2 high edge (as FdAxis of k_darcy.hip)
  float c1[3][4];
  float c2[3][4];
};
static GdAxis gd_axis(double inv_h) {
  static const double c1[3][3] = {{-1.5, 2.0, -0.5}, {-0.5, 0.0, 0.5}, {1.5, -2.0, 0.5}};
  static const double c2[3][4] = {{2.0, -5.0, 4.0, -1.0}, {1.0, -2.0, 1.0, 0.0}, {2.0, -5.0, 4.0, -1.0}};
  GdAxis a;
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 4; ++k) {
      a.c1[c][k] = (k < 3) ? (float)(c1[c][k] * inv_h) : 0.f;
      a.c2[c][k] = (float)(c2[c][k] * inv_h * inv_h);
    }
  return a;
}
// forward taps of line position i: 4 (index, weight) pairs; zero-weight taps keep an index inside [0, P)
struct GdTaps4 {
  int idx[4];
  float w1[4], w2[4];
};
__device__ __forceinline__ GdTaps4 gd_taps(const GdAxis& ax, int i, int P) {
  GdTaps4 t;
  const bool low = i == 0, high = i == P - 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int ix = high ? P - 1 - k : (low ? k : i - 1 + k);
    ix = ix < 0 ? 0 : (ix > P - 1 ? P - 1 : ix);
    t.idx[k] = ix;
    const float c1i = (k < 3) ? ax.c1[1][k] : 0.f, c2i = (k < 3) ? ax.c2[1][k] : 0.f;
    t.w1[k] = high ? ax.c1[2][k] : (low ? ax.c1[0][k] : c1i);
    t.w2[k] = high ? ax.c2[2][k] : (low ? ax.c2[0][k] : c2i);
  }
  return t;
}
// transposed taps of column m: rows 0, P-1, m-1, m, m+1 (rows that do not touch m get weight 0 and a clamped index)
struct GdTaps5 {
  int idx[5];
  float w1[5], w2[5];
};
__device__ __forceinline__ GdTaps5 gd_taps_T(const GdAxis& ax, int m, int P) {
  GdTaps5 t;
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
    t.idx[k] = i < 0 ? 0 : (i > P - 1 ? P - 1 : i);
  }
  return t;
}

// fixed-order block sum of two doubles (256 threads = 4 waves); every thread returns with both totals
__device__ __forceinline__ void gd_block_sum2(double& a, double& b, double (*red)[4], int tid) {
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off);
    b += __shfl_down(b, off);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = a;
    red[1][tid >> 6] = b;
  }
  __syncthreads();
  a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}
// zeta / sqrt(L), rounded once to fp32; exactly 0 when the term is absent
__device__ __forceinline__ float gd_scale(float zeta, double L) { return (L > 0.0 && zeta != 0.f) ? (float)((double)zeta / sqrt(L)) : 0.f; }

__global__ void __launch_bounds__(256) guidance_cotangent_kernel(const float* __restrict__ xh, const float* __restrict__ y,
                                                                 const float* __restrict__ msk,
                                                                 const float* __restrict__ f_s, float zeta_obs, float zeta_pde,
                                                                 float bc1_sign, GdAxis ax0, GdAxis ax1, float* __restrict__ v,
                                                                 float* __restrict__ sums, int P) {
  HIP_DYNAMIC_SHARED(float, smem)
  __shared__ double red[2][4];
  const int N = P * P, F = N;
  const int b = blockIdx.x, tid = threadIdx.x;
  float* sp = smem;
  float* sK = sp + F;
  float* skg = sp + 2 * F;    // -K r_eq
  float* sa0 = sp + 3 * F;    // coefficient on p0
  float* sa1 = sp + 4 * F;    // coefficient on p1
  float* sb0 = sp + 5 * F;    // coefficient on K0
  float* sb1 = sp + 6 * F;    // coefficient on K1
  float* sd = sp + 7 * F;     // direct dependence of eq on K at the same pixel
  const float* xb = xh + (size_t)b * 2 * N;
  const float* yb = y + (size_t)b * 2 * N;
  const float* mb = msk + (size_t)b * 2 * N;
  const int dj = 256 % P, di = 256 / P;

  double acc_obs = 0.0, acc_r2 = 0.0;
  for (int n = tid; n < N; n += 256) {
    const float vp = xb[n], vK = xb[N + n];
    sp[n] = vp;
    sK[n] = vK;
    const float d0 = vp - yb[n], d1 = vK - yb[N + n];
    acc_obs += (double)(mb[n] * (d0 * d0)) + (double)(mb[N + n] * (d1 * d1));
  }
  __syncthreads();
  {
    int i = tid / P, j = tid - (tid / P) * P;
    for (int n = tid; n < N; n += 256) {
      const GdTaps4 ti = gd_taps(ax0, i, P), tj = gd_taps(ax1, j, P);
      float p0 = 0.f, p00 = 0.f, K0 = 0.f, p1 = 0.f, p11 = 0.f, K1 = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float pa = sp[ti.idx[k] * P + j], pr = sp[i * P + tj.idx[k]];
        p0 = fmaf(ti.w1[k], pa, p0);
        p00 = fmaf(ti.w2[k], pa, p00);
        p1 = fmaf(tj.w1[k], pr, p1);
        p11 = fmaf(tj.w2[k], pr, p11);
        if (k < 3) {
          K0 = fmaf(ti.w1[k], sK[ti.idx[k] * P + j], K0);
          K1 = fmaf(tj.w1[k], sK[i * P + tj.idx[k]], K1);
        }
      }
      const float Kv = sK[n];
      const float vj00 = -Kv * p00 - K0 * p0;
      const float vj11 = -Kv * p11 - K1 * p1;
      const float eq = vj00 + vj11 - f_s[n];
      const float s0 = (i == 0) ? -1.f : ((i == P - 1) ? 1.f : 0.f);
      const float s1 = (j == 0) ? bc1_sign : ((j == P - 1) ? -bc1_sign : 0.f);
      const float bc0 = s0 * p0, bc1 = s1 * p1;
      acc_r2 += (double)(eq * eq) + (double)(bc0 * bc0) + (double)(bc1 * bc1);
      skg[n] = -Kv * eq;
      sa0[n] = -K0 * eq + s0 * bc0;
      sa1[n] = -K1 * eq + s1 * bc1;
      sb0[n] = -p0 * eq;
      sb1[n] = -p1 * eq;
      sd[n] = -(p00 + p11) * eq;
      j += dj;
      i += di;
      if (j >= P) {
        j -= P;
        ++i;
      }
    }
  }
  gd_block_sum2(acc_obs, acc_r2, red, tid);     // (its barrier also publishes the six operand fields)
  const float so = gd_scale(zeta_obs, acc_obs), sr = gd_scale(zeta_pde, acc_r2);
  if (tid == 0) {
    sums[2 * b] = (float)acc_obs;
    sums[2 * b + 1] = (float)acc_r2;
  }
  {
    int i = tid / P, j = tid - (tid / P) * P;
    float* vb = v + (size_t)b * 2 * N;
    for (int n = tid; n < N; n += 256) {
      const GdTaps5 ti = gd_taps_T(ax0, i, P), tj = gd_taps_T(ax1, j, P);
      float g00 = 0.f, g11 = 0.f, ga0 = 0.f, ga1 = 0.f, gb0 = 0.f, gb1 = 0.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int c0 = ti.idx[k] * P + j, c1 = i * P + tj.idx[k];
        g00 = fmaf(ti.w2[k], skg[c0], g00);
        ga0 = fmaf(ti.w1[k], sa0[c0], ga0);
        gb0 = fmaf(ti.w1[k], sb0[c0], gb0);
        g11 = fmaf(tj.w2[k], skg[c1], g11);
        ga1 = fmaf(tj.w1[k], sa1[c1], ga1);
        gb1 = fmaf(tj.w1[k], sb1[c1], gb1);
      }
      const float gp = ((g00 + g11) + ga0) + ga1;
      const float gK = (sd[n] + gb0) + gb1;
      const float op = so * (mb[n] * (sp[n] - yb[n])), oK = so * (mb[N + n] * (sK[n] - yb[N + n]));
      vb[n] = fmaf(sr, gp, op);
      vb[N + n] = fmaf(sr, gK, oK);
      j += dj;
      i += di;
      if (j >= P) {
        j -= P;
        ++i;
      }
    }
  }
}

// General stencil sets: between pidm_darcy_residual_general_fwd and _bwd.  One workgroup per sample, two passes over the sample
// (sums, then the scaled outputs); the second pass re-reads what the first just pulled through L2.  Same fp64 tree as above.
__global__ void __launch_bounds__(256) guidance_scale_general_kernel(const float* __restrict__ xh, const float* __restrict__ y,
                                                                     const float* __restrict__ msk,
                                                                     const float* __restrict__ res, float zeta_obs, float zeta_pde,
                                                                     float* __restrict__ gres, float* __restrict__ v_obs,
                                                                     float* __restrict__ sums, int N) {
  __shared__ double red[2][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* xb = xh + (size_t)b * 2 * N;
  const float* yb = y + (size_t)b * 2 * N;
  const float* mb = msk + (size_t)b * 2 * N;
  const float* rb = res + (size_t)b * 3 * N;
  double acc_obs = 0.0, acc_r2 = 0.0;
  for (int n = tid; n < N; n += 256) {
    const float d0 = xb[n] - yb[n], d1 = xb[N + n] - yb[N + n];
    acc_obs += (double)(mb[n] * (d0 * d0)) + (double)(mb[N + n] * (d1 * d1));
    const float r0 = rb[3 * n], r1 = rb[3 * n + 1], r2 = rb[3 * n + 2];
    acc_r2 += (double)(r0 * r0) + (double)(r1 * r1) + (double)(r2 * r2);
  }
  gd_block_sum2(acc_obs, acc_r2, red, tid);
  const float so = gd_scale(zeta_obs, acc_obs), sr = gd_scale(zeta_pde, acc_r2);
  if (tid == 0) {
    sums[2 * b] = (float)acc_obs;
    sums[2 * b + 1] = (float)acc_r2;
  }
  for (int n = tid; n < 2 * N; n += 256) v_obs[(size_t)b * 2 * N + n] = so * (mb[n] * (xb[n] - yb[n]));
  for (int n = tid; n < 3 * N; n += 256) gres[(size_t)b * 3 * N + n] = sr * rb[n];
}

// ---- flux observations --------------------------------------------------------------------------------------------------------
// Darcy flux q = (q0, q1) = (-K D0 p, -K D1 p) with the residual's own first-derivative operators; readings y_q under a 0/1 mask
// m_q: L_flux = sum m_q (q - y_q)^2, and Phi gains zeta_flux sqrt(L_flux).  With e_c = m_q,c (q_c - y_q,c), s_f = zeta_flux /
// sqrt(L_flux):  v_p += s_f sum_c D_c^T (-K e_c),  v_K += s_f (-sum_c e_c D_c p).
//
// guidance_cotangent_flux_kernel keeps the LDS plan of guidance_cotangent_kernel (8 F floats, so the same 5 <= P <= 71): three more
// operand fields would not fit at P = 64.  Instead the adjoint operands are stored ALREADY SCALED, which needs the sums first:
// pass 1 walks the stencils from the LDS-resident p and K and only sums; pass 2 walks them again (same taps, same order, so the
// same bits) and stores s_r (...) + s_f (-K e_c) into a0 / a1 and s_r (...) + s_f (-sum e_c p_c) into d; the gather is unchanged.
// y_q and m_q are read from global in both passes (the second read comes out of L2).
struct GdDerivs {
  float p0, p00, K0, p1, p11, K1;
};
__device__ __forceinline__ GdDerivs gd_derivs(const float* sp, const float* sK, const GdAxis& ax0, const GdAxis& ax1, int i, int j,
                                              int P) {
  const GdTaps4 ti = gd_taps(ax0, i, P), tj = gd_taps(ax1, j, P);
  GdDerivs d = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float pa = sp[ti.idx[k] * P + j], pr = sp[i * P + tj.idx[k]];
    d.p0 = fmaf(ti.w1[k], pa, d.p0);
    d.p00 = fmaf(ti.w2[k], pa, d.p00);
    d.p1 = fmaf(tj.w1[k], pr, d.p1);
    d.p11 = fmaf(tj.w2[k], pr, d.p11);
    if (k < 3) {
      d.K0 = fmaf(ti.w1[k], sK[ti.idx[k] * P + j], d.K0);
      d.K1 = fmaf(tj.w1[k], sK[i * P + tj.idx[k]], d.K1);
    }
  }
  return d;
}
__device__ __forceinline__ void gd_block_sum3(double& a, double& b, double& c, double (*red)[4], int tid) {
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off);
    b += __shfl_down(b, off);
    c += __shfl_down(c, off);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = a;
    red[1][tid >> 6] = b;
    red[2][tid >> 6] = c;
  }
  __syncthreads();
  a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  c = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
}

__global__ void __launch_bounds__(256) guidance_cotangent_flux_kernel(const float* __restrict__ xh, const float* __restrict__ y,
                                                                      const float* __restrict__ msk, const float* __restrict__ yq,
                                                                      const float* __restrict__ mq, const float* __restrict__ f_s,
                                                                      float zeta_obs, float zeta_pde, float zeta_flux, float bc1_sign,
                                                                      GdAxis ax0, GdAxis ax1, float* __restrict__ v,
                                                                      float* __restrict__ sums, int P) {
  HIP_DYNAMIC_SHARED(float, smem)
  __shared__ double red[3][4];
  const int N = P * P, F = N;
  const int b = blockIdx.x, tid = threadIdx.x;
  float* sp = smem;
  float* sK = sp + F;
  float* skg = sp + 2 * F;    // s_r (-K r_eq)
  float* sa0 = sp + 3 * F;    // coefficient on p0 (residual and flux parts)
  float* sa1 = sp + 4 * F;    // coefficient on p1
  float* sb0 = sp + 5 * F;    // coefficient on K0
  float* sb1 = sp + 6 * F;    // coefficient on K1
  float* sd = sp + 7 * F;     // direct dependence on K at the same pixel
  const float* xb = xh + (size_t)b * 2 * N;
  const float* yb = y + (size_t)b * 2 * N;
  const float* mb = msk + (size_t)b * 2 * N;
  const float* yqb = yq + (size_t)b * 2 * N;
  const float* mqb = mq + (size_t)b * 2 * N;
  const int dj = 256 % P, di = 256 / P;

  double acc_obs = 0.0, acc_r2 = 0.0, acc_fl = 0.0;
  for (int n = tid; n < N; n += 256) {
    const float vp = xb[n], vK = xb[N + n];
    sp[n] = vp;
    sK[n] = vK;
    const float d0 = vp - yb[n], d1 = vK - yb[N + n];
    acc_obs += (double)(mb[n] * (d0 * d0)) + (double)(mb[N + n] * (d1 * d1));
  }
  __syncthreads();
  {
    int i = tid / P, j = tid - (tid / P) * P;
    for (int n = tid; n < N; n += 256) {
      const GdDerivs d = gd_derivs(sp, sK, ax0, ax1, i, j, P);
      const float Kv = sK[n];
      const float vj00 = -Kv * d.p00 - d.K0 * d.p0;
      const float vj11 = -Kv * d.p11 - d.K1 * d.p1;
      const float eq = vj00 + vj11 - f_s[n];
      const float s0 = (i == 0) ? -1.f : ((i == P - 1) ? 1.f : 0.f);
      const float s1 = (j == 0) ? bc1_sign : ((j == P - 1) ? -bc1_sign : 0.f);
      const float bc0 = s0 * d.p0, bc1 = s1 * d.p1;
      acc_r2 += (double)(eq * eq) + (double)(bc0 * bc0) + (double)(bc1 * bc1);
      const float f0 = -Kv * d.p0 - yqb[n], f1 = -Kv * d.p1 - yqb[N + n];
      acc_fl += (double)(mqb[n] * (f0 * f0)) + (double)(mqb[N + n] * (f1 * f1));
      j += dj;
      i += di;
      if (j >= P) {
        j -= P;
        ++i;
      }
    }
  }
  gd_block_sum3(acc_obs, acc_r2, acc_fl, red, tid);
  const float so = gd_scale(zeta_obs, acc_obs), sr = gd_scale(zeta_pde, acc_r2), sf = gd_scale(zeta_flux, acc_fl);
  if (tid == 0) {
    sums[3 * b] = (float)acc_obs;
    sums[3 * b + 1] = (float)acc_r2;
    sums[3 * b + 2] = (float)acc_fl;
  }
  {
    int i = tid / P, j = tid - (tid / P) * P;
    for (int n = tid; n < N; n += 256) {
      const GdDerivs d = gd_derivs(sp, sK, ax0, ax1, i, j, P);
      const float Kv = sK[n];
      const float vj00 = -Kv * d.p00 - d.K0 * d.p0;
      const float vj11 = -Kv * d.p11 - d.K1 * d.p1;
      const float eq = sr * (vj00 + vj11 - f_s[n]);
      const float s0 = (i == 0) ? -1.f : ((i == P - 1) ? 1.f : 0.f);
      const float s1 = (j == 0) ? bc1_sign : ((j == P - 1) ? -bc1_sign : 0.f);
      const float bc0 = sr * (s0 * d.p0), bc1 = sr * (s1 * d.p1);
      const float e0 = sf * (mqb[n] * (-Kv * d.p0 - yqb[n])), e1 = sf * (mqb[N + n] * (-Kv * d.p1 - yqb[N + n]));
      skg[n] = -Kv * eq;
      sa0[n] = (-d.K0 * eq + s0 * bc0) - Kv * e0;
      sa1[n] = (-d.K1 * eq + s1 * bc1) - Kv * e1;
      sb0[n] = -d.p0 * eq;
      sb1[n] = -d.p1 * eq;
      sd[n] = -(d.p00 + d.p11) * eq - (e0 * d.p0 + e1 * d.p1);
      j += dj;
      i += di;
      if (j >= P) {
        j -= P;
        ++i;
      }
    }
  }
  __syncthreads();
  {
    int i = tid / P, j = tid - (tid / P) * P;
    float* vb = v + (size_t)b * 2 * N;
    for (int n = tid; n < N; n += 256) {
      const GdTaps5 ti = gd_taps_T(ax0, i, P), tj = gd_taps_T(ax1, j, P);
      float g00 = 0.f, g11 = 0.f, ga0 = 0.f, ga1 = 0.f, gb0 = 0.f, gb1 = 0.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int c0 = ti.idx[k] * P + j, c1 = i * P + tj.idx[k];
        g00 = fmaf(ti.w2[k], skg[c0], g00);
        ga0 = fmaf(ti.w1[k], sa0[c0], ga0);
        gb0 = fmaf(ti.w1[k], sb0[c0], gb0);
        g11 = fmaf(tj.w2[k], skg[c1], g11);
        ga1 = fmaf(tj.w1[k], sa1[c1], ga1);
        gb1 = fmaf(tj.w1[k], sb1[c1], gb1);
      }
      const float gp = ((g00 + g11) + ga0) + ga1;
      const float gK = (sd[n] + gb0) + gb1;
      const float op = so * (mb[n] * (sp[n] - yb[n])), oK = so * (mb[N + n] * (sK[n] - yb[N + n]));
      vb[n] = gp + op;
      vb[N + n] = gK + oK;
      j += dj;
      i += di;
      if (j >= P) {
        j -= P;
        ++i;
      }
    }
  }
}

// Any stencil set, any P: the flux term on top of the composition around guidance_scale_general_kernel.  dp0 / dp1 [B][N] are
// D0 p and D1 p (the first two fields the general residual leaves in its workspace, or one two-operator stencil launch on p).
// One workgroup per sample, two passes (sum, then write).  Writes sums3 [B,3] = (sums2[b], L_flux) (sums2 NULL: only the flux
// slot), w [B,2,N] = s_f (-K e_c) - the cotangents of the stencil adjoint that finishes the p channel - and the K channel
// v_out = v_in + s_f (-sum_c e_c D_c p) (v_out may be v_in: each element is read and written by one thread).
__global__ void __launch_bounds__(256) guidance_flux_general_kernel(const float* __restrict__ xh, const float* __restrict__ dp0,
                                                                    const float* __restrict__ dp1, const float* __restrict__ yq,
                                                                    const float* __restrict__ mq, float zeta_flux,
                                                                    const float* __restrict__ sums2, float* __restrict__ sums3,
                                                                    float* __restrict__ w, const float* v_in, float* v_out, int N) {
  __shared__ double red[3][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* Kb = xh + (size_t)b * 2 * N + N;
  const float* d0b = dp0 + (size_t)b * N;
  const float* d1b = dp1 + (size_t)b * N;
  const float* yqb = yq + (size_t)b * 2 * N;
  const float* mqb = mq + (size_t)b * 2 * N;
  double acc_fl = 0.0, z0 = 0.0, z1 = 0.0;
  for (int n = tid; n < N; n += 256) {
    const float Kv = Kb[n];
    const float f0 = -Kv * d0b[n] - yqb[n], f1 = -Kv * d1b[n] - yqb[N + n];
    acc_fl += (double)(mqb[n] * (f0 * f0)) + (double)(mqb[N + n] * (f1 * f1));
  }
  gd_block_sum3(acc_fl, z0, z1, red, tid);
  const float sf = gd_scale(zeta_flux, acc_fl);
  if (tid == 0) {
    if (sums2) {
      sums3[3 * b] = sums2[2 * b];
      sums3[3 * b + 1] = sums2[2 * b + 1];
    }
    sums3[3 * b + 2] = (float)acc_fl;
  }
  float* wb = w + (size_t)b * 2 * N;
  const float* vi = v_in + (size_t)b * 2 * N + N;
  float* vo = v_out + (size_t)b * 2 * N + N;
  for (int n = tid; n < N; n += 256) {
    const float Kv = Kb[n], p0 = d0b[n], p1 = d1b[n];
    const float e0 = sf * (mqb[n] * (-Kv * p0 - yqb[n])), e1 = sf * (mqb[N + n] * (-Kv * p1 - yqb[N + n]));
    wb[n] = -Kv * e0;
    wb[N + n] = -Kv * e1;
    vo[n] = vi[n] - (e0 * p0 + e1 * p1);
  }
}

// flux [B,2,N] = (-K D0 p, -K D1 p) from the two derivative fields dp0 / dp1 [B][N]
__global__ void __launch_bounds__(256) darcy_flux_kernel(const float* __restrict__ xh, const float* __restrict__ dp0,
                                                         const float* __restrict__ dp1, float* __restrict__ flux, size_t total, int N) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t b = idx / N, n = idx - b * N;
  const float Kv = xh[b * 2 * N + N + n];
  flux[b * 2 * N + n] = -Kv * dp0[idx];
  flux[b * 2 * N + N + n] = -Kv * dp1[idx];
}

__global__ void __launch_bounds__(256) guidance_add_kernel(float* __restrict__ v, const float* __restrict__ adj, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] += adj[i];
}

// out [B,C,HW] (NCHW) = c1 x0_pred + c2 x_t + sigma z - g, g [B,HW,C] read transposed.  A 64-pixel x C tile of g goes through LDS so
// that both the NHWC read and the NCHW accesses are contiguous; C <= 16.
__global__ void __launch_bounds__(256) psample_update_guided_kernel(const float* __restrict__ x0p, const float* __restrict__ xt,
                                                                    const float* __restrict__ z, const float* __restrict__ g, float c1,
                                                                    float c2, float sigma, float* __restrict__ out, int C, int HW) {
  __shared__ float tile[64 * 17];
  const int b = blockIdx.y, n0 = blockIdx.x * 64, tid = threadIdx.x;
  const int np = (HW - n0 < 64) ? HW - n0 : 64;
  const float* gb = g + ((size_t)b * HW + n0) * C;
  for (int e = tid; e < np * C; e += 256) {
    const int pix = e / C, c = e - pix * C;
    tile[pix * 17 + c] = gb[e];
  }
  __syncthreads();
  for (int e = tid; e < np * C; e += 256) {
    const int c = e / np, pix = e - c * np;
    const size_t o = ((size_t)b * C + c) * HW + n0 + pix;
    out[o] = fmaf(sigma, z[o], fmaf(c2, xt[o], c1 * x0p[o])) - tile[pix * 17 + c];
  }
}

static const size_t kGuidanceLdsMax = 160 * 1024 - 256;

}  // namespace pidm

using namespace pidm;

extern "C" int pidm_darcy_guidance_cotangent(const float* x0_pred, const float* obs, const float* mask, const float* f_s,
                                             float inv_h0, float inv_h1, float zeta_obs, float zeta_pde, float* v, float* sums, int B,
                                             int P, void* stream) {
  if (!x0_pred || !obs || !mask || !f_s || !v || !sums) return fail("darcy_guidance_cotangent: null buffer");
  if (B <= 0 || P < 5) return fail("darcy_guidance_cotangent: need B>0 and P>=5 (got B=%d P=%d)", B, P);
  const size_t lds = (size_t)8 * P * P * sizeof(float);
  if (lds > kGuidanceLdsMax) return fail("darcy_guidance_cotangent: P=%d does not fit the 160 KiB LDS (one sample per workgroup: P <= 71)", P);
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&guidance_cotangent_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kGuidanceLdsMax);
    attr_done = true;
  }
  hipLaunchKernelGGL(guidance_cotangent_kernel, dim3((unsigned)B), dim3(256), lds, as_stream(stream), x0_pred, obs, mask, f_s, zeta_obs, zeta_pde, (inv_h1 < 0.f) ? 1.f : -1.f, gd_axis(inv_h0),
                     gd_axis(inv_h1), v, sums, P);
  PIDM_CHECK_LAUNCH("guidance_cotangent_kernel");
  return 0;
}

extern "C" int pidm_darcy_guidance_cotangent_flux(const float* x0_pred, const float* obs, const float* mask, const float* flux_obs,
                                                  const float* flux_mask, const float* f_s, float inv_h0, float inv_h1, float zeta_obs,
                                                  float zeta_pde, float zeta_flux, float* v, float* sums, int B, int P, void* stream) {
  if (!x0_pred || !obs || !mask || !flux_obs || !flux_mask || !f_s || !v || !sums)
    return fail("darcy_guidance_cotangent_flux: null buffer");
  if (B <= 0 || P < 5) return fail("darcy_guidance_cotangent_flux: need B>0 and P>=5 (got B=%d P=%d)", B, P);
  const size_t lds = (size_t)8 * P * P * sizeof(float);
  if (lds > kGuidanceLdsMax)
    return fail("darcy_guidance_cotangent_flux: P=%d does not fit the 160 KiB LDS (one sample per workgroup: P <= 71)", P);
  static bool attr_done = false;
  if (!attr_done) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&guidance_cotangent_flux_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kGuidanceLdsMax);
    attr_done = true;
  }
  hipLaunchKernelGGL(guidance_cotangent_flux_kernel, dim3((unsigned)B), dim3(256), lds, as_stream(stream), x0_pred, obs, mask, flux_obs,
                     flux_mask, f_s, zeta_obs, zeta_pde, zeta_flux, (inv_h1 < 0.f) ? 1.f : -1.f, gd_axis(inv_h0), gd_axis(inv_h1), v,
                     sums, P);
  PIDM_CHECK_LAUNCH("guidance_cotangent_flux_kernel");
  return 0;
}

static int flux_range_check(const char* what, int B, int P) {
  if (B <= 0 || P < 2 || (long long)B * P * P > 0x7fffffffLL / 4) return fail("%s: need B>0, P>=2 and B*P*P < 2^29 (got B=%d P=%d)", what, B, P);
  return 0;
}

extern "C" int pidm_guidance_flux_general(const float* x0_pred, const float* dp0, const float* dp1, const float* flux_obs,
                                          const float* flux_mask, float zeta_flux, const float* sums2, float* sums3, float* w,
                                          const float* v_in, float* v_out, int B, int P, void* stream) {
  if (!x0_pred || !dp0 || !dp1 || !flux_obs || !flux_mask || !sums3 || !w || !v_in || !v_out) return fail("guidance_flux_general: null buffer");
  if (int rc = flux_range_check("guidance_flux_general", B, P)) return rc;
  hipLaunchKernelGGL(guidance_flux_general_kernel, dim3((unsigned)B), dim3(256), 0, as_stream(stream), x0_pred, dp0, dp1, flux_obs,
                     flux_mask, zeta_flux, sums2, sums3, w, v_in, v_out, P * P);
  PIDM_CHECK_LAUNCH("guidance_flux_general_kernel");
  return 0;
}

extern "C" size_t pidm_darcy_flux_ws(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  return (size_t)2 * B * P * P * sizeof(float);
}

extern "C" int pidm_darcy_flux(const float* x0, const pidm_stencil_op* ops2_host, int periodic, float* flux, void* workspace, int B,
                               int P, void* stream) {
  if (!x0 || !ops2_host || !flux || !workspace) return fail("darcy_flux: null buffer");
  if (int rc = flux_range_check("darcy_flux", B, P)) return rc;
  const long long N = (long long)P * P, total = (long long)B * N;
  float* d = reinterpret_cast<float*>(workspace);
  float* outs[2] = {d, d + total};
  if (int rc = pidm_stencil_apply(x0, 2 * N, ops2_host, outs, 2, N, B, P, P, periodic, stream)) return rc;
  hipLaunchKernelGGL(darcy_flux_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x0, d, d + total, flux,
                     (size_t)total, (int)N);
  PIDM_CHECK_LAUNCH("darcy_flux_kernel");
  return 0;
}

extern "C" int pidm_guidance_scale_general(const float* x0_pred, const float* obs, const float* mask, const float* residual,
                                           float zeta_obs, float zeta_pde, float* grad_res, float* v_obs, float* sums, int B, int P,
                                           void* stream) {
  if (!x0_pred || !obs || !mask || !residual || !grad_res || !v_obs || !sums) return fail("guidance_scale_general: null buffer");
  if (B <= 0 || P <= 0 || P > 16384) return fail("guidance_scale_general: need B>0 and 0<P<=16384 (got B=%d P=%d)", B, P);
  hipLaunchKernelGGL(guidance_scale_general_kernel, dim3((unsigned)B), dim3(256), 0, as_stream(stream), x0_pred, obs, mask, residual, zeta_obs, zeta_pde, grad_res, v_obs, sums, P * P);
  PIDM_CHECK_LAUNCH("guidance_scale_general_kernel");
  return 0;
}

extern "C" int pidm_guidance_add(float* v, const float* adjoint, size_t n, void* stream) {
  if (!v || !adjoint) return fail("guidance_add: null buffer");
  if (n == 0 || n > ((size_t)1 << 40)) return fail("guidance_add: bad element count %zu", n);
  hipLaunchKernelGGL(guidance_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), v, adjoint, n);
  PIDM_CHECK_LAUNCH("guidance_add_kernel");
  return 0;
}

extern "C" int pidm_psample_update_guided(const float* x0_pred, const float* x_t, const float* z, const float* g_nhwc, float c1, float c2,
                                          float sigma, float* x_prev, int B, int C, int HW, void* stream) {
  if (!x0_pred || !x_t || !z || !g_nhwc || !x_prev) return fail("psample_update_guided: null buffer");
  if (B <= 0 || B > 65535 || HW <= 0) return fail("psample_update_guided: need 0<B<=65535 and HW>0 (got B=%d HW=%d)", B, HW);
  if (C <= 0 || C > 16) return fail("psample_update_guided: C=%d, need 1..16", C);
  hipLaunchKernelGGL(psample_update_guided_kernel, dim3((unsigned)((HW + 63) / 64), (unsigned)B), dim3(256), 0, as_stream(stream),
                     x0_pred, x_t, z, g_nhwc, c1, c2, sigma, x_prev, C, HW);
  PIDM_CHECK_LAUNCH("psample_update_guided_kernel");
  return 0;
}
