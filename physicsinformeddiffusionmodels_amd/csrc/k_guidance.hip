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
// 2 x 4 doubles of the block sums.  The taps are darcy_kernel's own (k_darcy_stencil.h, window 0 .. P-1), taken in its order: its
// adjoint figures carry over.
// The sums are fp64: a thread adds its pixels in index order, then block_sum_f64 (pidm_common.h) - no atomics, the same bits run
// to run and for any batch size (a sample never sees another one).
#include "k_darcy_stencil.h"
#include "pidm_common.h"

namespace pidm {

// ---- pieces shared by the two LDS-resident kernels (guidance_cotangent_kernel, guidance_cotangent_flux_kernel) -----------------
struct GdFields {      // the 8 F floats of dynamic LDS
  float* p;
  float* K;
  float* kg;           // -K r_eq
  float* a0;           // coefficient on p0 (flux kernel: residual and flux parts)
  float* a1;           // coefficient on p1
  float* b0;           // coefficient on K0
  float* b1;           // coefficient on K1
  float* d;            // direct dependence of eq (and of the flux) on K at the same pixel
};
__device__ __forceinline__ GdFields gd_fields(float* smem, int F) {
  return GdFields{smem, smem + F, smem + 2 * F, smem + 3 * F, smem + 4 * F, smem + 5 * F, smem + 6 * F, smem + 7 * F};
}
// pixel (i, j) of n = tid, tid + 256, ... without a division per pixel
struct GdWalk {
  int i, j, di, dj;
  __device__ __forceinline__ GdWalk(int tid, int P) : i(tid / P), j(tid - (tid / P) * P), di(256 / P), dj(256 % P) {}
  __device__ __forceinline__ void step(int P) {
    j += dj;
    i += di;
    if (j >= P) {
      j -= P;
      ++i;
    }
  }
};
// x -> LDS (p | K); returns this thread's part of L_obs.  The caller's barrier publishes the two fields.
__device__ __forceinline__ double gd_stage(const float* __restrict__ xb, const float* __restrict__ yb, const float* __restrict__ mb,
                                           const GdFields& s, int N, int tid) {
  double acc_obs = 0.0;
  for (int n = tid; n < N; n += 256) {
    const float vp = xb[n], vK = xb[N + n];
    s.p[n] = vp;
    s.K[n] = vK;
    const float d0 = vp - yb[n], d1 = vK - yb[N + n];
    acc_obs += (double)(mb[n] * (d0 * d0)) + (double)(mb[N + n] * (d1 * d1));
  }
  return acc_obs;
}
// the forward stencil walk: the six derivatives at pixel (i, j)
struct GdDerivs {
  float p0, p00, K0, p1, p11, K1;
};
__device__ __forceinline__ GdDerivs gd_derivs(const float* sp, const float* sK, const FdAxis& ax0, const FdAxis& ax1, int i, int j,
                                              int P) {
  const FdTaps4 ti = fd_taps(ax0, i, P, 0, P - 1), tj = fd_taps(ax1, j, P, 0, P - 1);
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
// the residual terms from the derivatives: eq BEFORE f_s is subtracted, the boundary signs and the two boundary channels
struct GdResid {
  float eq, s0, s1, bc0, bc1;
};
__device__ __forceinline__ GdResid gd_resid(const GdDerivs& d, float Kv, float bc1_sign, int i, int j, int P) {
  GdResid r;
  const float vj00 = -Kv * d.p00 - d.K0 * d.p0;
  const float vj11 = -Kv * d.p11 - d.K1 * d.p1;
  r.eq = vj00 + vj11;
  r.s0 = (i == 0) ? -1.f : ((i == P - 1) ? 1.f : 0.f);
  r.s1 = (j == 0) ? bc1_sign : ((j == P - 1) ? -bc1_sign : 0.f);
  r.bc0 = r.s0 * d.p0;
  r.bc1 = r.s1 * d.p1;
  return r;
}
// the transposed gather at pixel n = (i, j) from the six operand fields: (J^T .) on the p and on the K channel
struct GdGrad {
  float gp, gK;
};
__device__ __forceinline__ GdGrad gd_gather(const GdFields& s, const FdAxis& ax0, const FdAxis& ax1, int i, int j, int n, int P) {
  const FdTaps5 ti = fd_taps_T(ax0, i, P, 0, P - 1), tj = fd_taps_T(ax1, j, P, 0, P - 1);
  float g00 = 0.f, g11 = 0.f, ga0 = 0.f, ga1 = 0.f, gb0 = 0.f, gb1 = 0.f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int c0 = ti.idx[k] * P + j, c1 = i * P + tj.idx[k];
    g00 = fmaf(ti.w2[k], s.kg[c0], g00);
    ga0 = fmaf(ti.w1[k], s.a0[c0], ga0);
    gb0 = fmaf(ti.w1[k], s.b0[c0], gb0);
    g11 = fmaf(tj.w2[k], s.kg[c1], g11);
    ga1 = fmaf(tj.w1[k], s.a1[c1], ga1);
    gb1 = fmaf(tj.w1[k], s.b1[c1], gb1);
  }
  return GdGrad{((g00 + g11) + ga0) + ga1, (s.d[n] + gb0) + gb1};
}

__global__ void __launch_bounds__(256) guidance_cotangent_kernel(const float* __restrict__ xh, const float* __restrict__ y,
                                                                 const float* __restrict__ msk,
                                                                 const float* __restrict__ f_s, float zeta_obs, float zeta_pde,
                                                                 float bc1_sign, FdAxis ax0, FdAxis ax1, float* __restrict__ v,
                                                                 float* __restrict__ sums, int P) {
  HIP_DYNAMIC_SHARED(float, smem)
  __shared__ double red[2][4];
  const int N = P * P;
  const int b = blockIdx.x, tid = threadIdx.x;
  const GdFields s = gd_fields(smem, N);
  const float* xb = xh + (size_t)b * 2 * N;
  const float* yb = y + (size_t)b * 2 * N;
  const float* mb = msk + (size_t)b * 2 * N;

  double L[2] = {gd_stage(xb, yb, mb, s, N, tid), 0.0};     // L_obs, L_pde
  __syncthreads();
  {
    GdWalk q(tid, P);
    for (int n = tid; n < N; n += 256, q.step(P)) {
      const GdDerivs d = gd_derivs(s.p, s.K, ax0, ax1, q.i, q.j, P);
      const float Kv = s.K[n];
      const GdResid r = gd_resid(d, Kv, bc1_sign, q.i, q.j, P);
      const float eq = r.eq - f_s[n];
      L[1] += (double)(eq * eq) + (double)(r.bc0 * r.bc0) + (double)(r.bc1 * r.bc1);
      s.kg[n] = -Kv * eq;
      s.a0[n] = -d.K0 * eq + r.s0 * r.bc0;
      s.a1[n] = -d.K1 * eq + r.s1 * r.bc1;
      s.b0[n] = -d.p0 * eq;
      s.b1[n] = -d.p1 * eq;
      s.d[n] = -(d.p00 + d.p11) * eq;
    }
  }
  block_sum_f64<2>(L, red, tid);     // (its barrier also publishes the six operand fields)
  const float so = guidance_scale(zeta_obs, L[0]), sr = guidance_scale(zeta_pde, L[1]);
  if (tid == 0) {
    sums[2 * b] = (float)L[0];
    sums[2 * b + 1] = (float)L[1];
  }
  {
    GdWalk q(tid, P);
    float* vb = v + (size_t)b * 2 * N;
    for (int n = tid; n < N; n += 256, q.step(P)) {
      const GdGrad g = gd_gather(s, ax0, ax1, q.i, q.j, n, P);
      const float op = so * (mb[n] * (s.p[n] - yb[n])), oK = so * (mb[N + n] * (s.K[n] - yb[N + n]));
      vb[n] = fmaf(sr, g.gp, op);
      vb[N + n] = fmaf(sr, g.gK, oK);
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
  double L[2] = {0.0, 0.0};     // L_obs, L_pde
  for (int n = tid; n < N; n += 256) {
    const float d0 = xb[n] - yb[n], d1 = xb[N + n] - yb[N + n];
    L[0] += (double)(mb[n] * (d0 * d0)) + (double)(mb[N + n] * (d1 * d1));
    const float r0 = rb[3 * n], r1 = rb[3 * n + 1], r2 = rb[3 * n + 2];
    L[1] += (double)(r0 * r0) + (double)(r1 * r1) + (double)(r2 * r2);
  }
  block_sum_f64<2>(L, red, tid);
  const float so = guidance_scale(zeta_obs, L[0]), sr = guidance_scale(zeta_pde, L[1]);
  if (tid == 0) {
    sums[2 * b] = (float)L[0];
    sums[2 * b + 1] = (float)L[1];
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
__global__ void __launch_bounds__(256) guidance_cotangent_flux_kernel(const float* __restrict__ xh, const float* __restrict__ y,
                                                                      const float* __restrict__ msk, const float* __restrict__ yq,
                                                                      const float* __restrict__ mq, const float* __restrict__ f_s,
                                                                      float zeta_obs, float zeta_pde, float zeta_flux, float bc1_sign,
                                                                      FdAxis ax0, FdAxis ax1, float* __restrict__ v,
                                                                      float* __restrict__ sums, int P) {
  HIP_DYNAMIC_SHARED(float, smem)
  __shared__ double red[3][4];
  const int N = P * P;
  const int b = blockIdx.x, tid = threadIdx.x;
  const GdFields s = gd_fields(smem, N);
  const float* xb = xh + (size_t)b * 2 * N;
  const float* yb = y + (size_t)b * 2 * N;
  const float* mb = msk + (size_t)b * 2 * N;
  const float* yqb = yq + (size_t)b * 2 * N;
  const float* mqb = mq + (size_t)b * 2 * N;

  double L[3] = {gd_stage(xb, yb, mb, s, N, tid), 0.0, 0.0};     // L_obs, L_pde, L_flux
  __syncthreads();
  {
    GdWalk q(tid, P);
    for (int n = tid; n < N; n += 256, q.step(P)) {
      const GdDerivs d = gd_derivs(s.p, s.K, ax0, ax1, q.i, q.j, P);
      const float Kv = s.K[n];
      const GdResid r = gd_resid(d, Kv, bc1_sign, q.i, q.j, P);
      const float eq = r.eq - f_s[n];
      L[1] += (double)(eq * eq) + (double)(r.bc0 * r.bc0) + (double)(r.bc1 * r.bc1);
      const float f0 = -Kv * d.p0 - yqb[n], f1 = -Kv * d.p1 - yqb[N + n];
      L[2] += (double)(mqb[n] * (f0 * f0)) + (double)(mqb[N + n] * (f1 * f1));
    }
  }
  block_sum_f64<3>(L, red, tid);
  const float so = guidance_scale(zeta_obs, L[0]), sr = guidance_scale(zeta_pde, L[1]), sf = guidance_scale(zeta_flux, L[2]);
  if (tid == 0) {
    sums[3 * b] = (float)L[0];
    sums[3 * b + 1] = (float)L[1];
    sums[3 * b + 2] = (float)L[2];
  }
  {
    GdWalk q(tid, P);
    for (int n = tid; n < N; n += 256, q.step(P)) {
      const GdDerivs d = gd_derivs(s.p, s.K, ax0, ax1, q.i, q.j, P);
      const float Kv = s.K[n];
      const GdResid r = gd_resid(d, Kv, bc1_sign, q.i, q.j, P);
      const float eq = sr * (r.eq - f_s[n]);
      const float bc0 = sr * r.bc0, bc1 = sr * r.bc1;
      const float e0 = sf * (mqb[n] * (-Kv * d.p0 - yqb[n])), e1 = sf * (mqb[N + n] * (-Kv * d.p1 - yqb[N + n]));
      s.kg[n] = -Kv * eq;
      s.a0[n] = (-d.K0 * eq + r.s0 * bc0) - Kv * e0;
      s.a1[n] = (-d.K1 * eq + r.s1 * bc1) - Kv * e1;
      s.b0[n] = -d.p0 * eq;
      s.b1[n] = -d.p1 * eq;
      s.d[n] = -(d.p00 + d.p11) * eq - (e0 * d.p0 + e1 * d.p1);
    }
  }
  __syncthreads();
  {
    GdWalk q(tid, P);
    float* vb = v + (size_t)b * 2 * N;
    for (int n = tid; n < N; n += 256, q.step(P)) {
      const GdGrad g = gd_gather(s, ax0, ax1, q.i, q.j, n, P);
      const float op = so * (mb[n] * (s.p[n] - yb[n])), oK = so * (mb[N + n] * (s.K[n] - yb[N + n]));
      vb[n] = g.gp + op;
      vb[N + n] = g.gK + oK;
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
  __shared__ double red[1][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* Kb = xh + (size_t)b * 2 * N + N;
  const float* d0b = dp0 + (size_t)b * N;
  const float* d1b = dp1 + (size_t)b * N;
  const float* yqb = yq + (size_t)b * 2 * N;
  const float* mqb = mq + (size_t)b * 2 * N;
  double L[1] = {0.0};     // L_flux
  for (int n = tid; n < N; n += 256) {
    const float Kv = Kb[n];
    const float f0 = -Kv * d0b[n] - yqb[n], f1 = -Kv * d1b[n] - yqb[N + n];
    L[0] += (double)(mqb[n] * (f0 * f0)) + (double)(mqb[N + n] * (f1 * f1));
  }
  block_sum_f64<1>(L, red, tid);
  const float sf = guidance_scale(zeta_flux, L[0]);
  if (tid == 0) {
    if (sums2) {
      sums3[3 * b] = sums2[2 * b];
      sums3[3 * b + 1] = sums2[2 * b + 1];
    }
    sums3[3 * b + 2] = (float)L[0];
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

// host side of the two LDS-resident kernels: the B / P check, the dynamic LDS of one launch (8 F floats) and, once per kernel, the
// opt-in to more than 64 KiB of it
static const size_t kGuidanceLdsMax = 160 * 1024 - 256;
static int gd_lds_plan(const char* what, const void* kernel, bool* attr_done, int B, int P, size_t* lds) {
  if (B <= 0 || P < 5) return fail("%s: need B>0 and P>=5 (got B=%d P=%d)", what, B, P);
  *lds = (size_t)8 * P * P * sizeof(float);
  if (*lds > kGuidanceLdsMax) return fail("%s: P=%d does not fit the 160 KiB LDS (one sample per workgroup: P <= 71)", what, P);
  if (!*attr_done) {
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGuidanceLdsMax);
    *attr_done = true;
  }
  return 0;
}

}  // namespace pidm

using namespace pidm;

extern "C" int pidm_darcy_guidance_cotangent(const float* x0_pred, const float* obs, const float* mask, const float* f_s,
                                             float inv_h0, float inv_h1, float zeta_obs, float zeta_pde, float* v, float* sums, int B,
                                             int P, void* stream) {
  if (!x0_pred || !obs || !mask || !f_s || !v || !sums) return fail("darcy_guidance_cotangent: null buffer");
  static bool attr_done = false;
  size_t lds;
  if (int rc = gd_lds_plan("darcy_guidance_cotangent", reinterpret_cast<const void*>(&guidance_cotangent_kernel), &attr_done, B, P, &lds))
    return rc;
  hipLaunchKernelGGL(guidance_cotangent_kernel, dim3((unsigned)B), dim3(256), lds, as_stream(stream), x0_pred, obs, mask, f_s, zeta_obs, zeta_pde, (inv_h1 < 0.f) ? 1.f : -1.f, make_axis(inv_h0),
                     make_axis(inv_h1), v, sums, P);
  PIDM_CHECK_LAUNCH("guidance_cotangent_kernel");
  return 0;
}

extern "C" int pidm_darcy_guidance_cotangent_flux(const float* x0_pred, const float* obs, const float* mask, const float* flux_obs,
                                                  const float* flux_mask, const float* f_s, float inv_h0, float inv_h1, float zeta_obs,
                                                  float zeta_pde, float zeta_flux, float* v, float* sums, int B, int P, void* stream) {
  if (!x0_pred || !obs || !mask || !flux_obs || !flux_mask || !f_s || !v || !sums)
    return fail("darcy_guidance_cotangent_flux: null buffer");
  static bool attr_done = false;
  size_t lds;
  if (int rc = gd_lds_plan("darcy_guidance_cotangent_flux", reinterpret_cast<const void*>(&guidance_cotangent_flux_kernel), &attr_done, B,
                           P, &lds))
    return rc;
  hipLaunchKernelGGL(guidance_cotangent_flux_kernel, dim3((unsigned)B), dim3(256), lds, as_stream(stream), x0_pred, obs, mask, flux_obs,
                     flux_mask, f_s, zeta_obs, zeta_pde, zeta_flux, (inv_h1 < 0.f) ? 1.f : -1.f, make_axis(inv_h0), make_axis(inv_h1), v,
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
