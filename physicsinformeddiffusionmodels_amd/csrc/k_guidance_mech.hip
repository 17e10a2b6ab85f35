// Posterior guidance of the mechanics (topology optimisation) sampler for gfx950: the arithmetic of one guided step around the UNet.
//
// Per sample, with the quantities of mech_kernel (k_mech.hip) for the model's x0 estimate x [3,nel,nel] = (u_x, u_y, rho):
//   model_out = (U = bilinear(u, nn), rho zero-padded) [3,nn,nn],  r = K_closed(rho) U - f (row-replaced),  shift = mean(rho) - vf,
//   L_obs = sum m (model_out - y)^2 (channel 2 over rows / columns < nel only: the padding is no part of the state),
//   L_pde = sum r^2,  L_vol = shift^2,
//   Phi = zeta_obs sqrt(L_obs) + zeta_pde sqrt(L_pde) + zeta_vol sqrt(L_vol),   v = dPhi/dx   (a term whose L is exactly 0 is omitted).
// v is the cotangent that the UNet's input-only backward pulls to the network input; pidm_psample_update_guided_resized then takes
// the ancestral step on the nn x nn state minus that gradient carried back through the nn -> nel resize of the network input.
//
// mech_guidance_kernel is a sibling of mech_loss_kernel: one workgroup per sample, LDS U[ndof] | rho[E] | Z[ndof] | GU[ndof]
// ((3 ndof + E) floats: 117 784 B at nel = 64, one workgroup per CU).  Unlike the training loss the scale factors 1 / sqrt(L) need
// the sums BEFORE the adjoint: phase 2 leaves the unscaled residual in Z while it sums, one fixed-order block reduction follows,
// then every thread rescales the entries it wrote itself and fills GU; phases 3 and 4 are mech_kernel<true>'s gather adjoints.
// The three sums are fp64: a thread adds its entries in index order, then block_sum_f64 (pidm_common.h, shared with k_guidance.hip)
// - no atomics, the same bits run to run and for any batch size (a sample never sees another one).
//
// Compliance term (FORM != kCompNone; pidm_mech_guidance_cotangent_compliance): C = U . K_closed(rho) U = sum_i U_i Kbc_i, the
// `compliance` of mech_kernel<false> (fp32 products, fp64 sums), is a fourth sum and enters Phi linearly and signed, zeta_comp C.
//   kCompEnergy       d/d(U, rho) of zeta_comp C - mech_kernel<true>'s g_compliance terms: the cotangent on Kbc_i gains zeta_comp U_i
//                     (it rides the phase-3 gathers when i is free and is the transposed identity row when i is clamped) and the
//                     direct gU_i gains zeta_comp Kbc_i;
//   kCompSensitivity  d/d rho of -zeta_comp sg(U) . K_closed(rho) sg(U), the adjoint sensitivity of f^T K^-1 f at the predicted U:
//                     v_rho_e gains -zeta_comp sum_{a : D_e[a] free} U_{D_e[a]} (k_e u_e)_a, the displacement channels nothing.
// Kbc_i waits in GU (idle until the rescale) for the thread that wrote it; the sensitivity form reads the clamp flags of an
// element's eight dofs from bcs again.  No LDS beyond the plan above, no atomics, no further pass over global memory.
#include "k_mech_common.h"

namespace pidm {

enum { kCompNone = -1, kCompEnergy = 0, kCompSensitivity = 1 };

template <int FORM>
__global__ void __launch_bounds__(256) mech_guidance_kernel(MechMesh ms, const float* __restrict__ x0,   // [B,3,nel,nel] x0 estimate
                                                            const float* __restrict__ bcs,               // [B,4,nn,nn]
                                                            const float* __restrict__ vf,                // [B]
                                                            const float* __restrict__ obs,               // [B,3,nn,nn]
                                                            const float* __restrict__ msk,               // [B,3,nn,nn]
                                                            float zeta_obs, float zeta_pde, float zeta_vol, float zeta_comp,
                                                            float* __restrict__ v,                       // [B,3,nel,nel]
                                                            float* __restrict__ model_out,               // [B,3,nn,nn]
                                                            float* __restrict__ sums) {                  // [B,3] or [B,4]
  constexpr bool COMP = FORM != kCompNone;
  constexpr int NS = COMP ? 4 : 3;
  HIP_DYNAMIC_SHARED(float, smem)
  __shared__ double red[NS][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nel = ms.nel, nn = ms.nn, E = ms.E, ndof = ms.ndof;
  float* sU = smem;
  float* sR = smem + ndof;
  float* sZ = sR + E;
  float* sG = sZ + ndof;
  const float* xb = x0 + (size_t)b * 3 * nel * nel;
  const float* bb = bcs + (size_t)b * 4 * nn * nn;
  const float* yb = obs + (size_t)b * 3 * nn * nn;
  const float* mb = msk + (size_t)b * 3 * nn * nn;
  float* mo = model_out + (size_t)b * 3 * nn * nn;
  // ---- phase 1: U = bilinear(u, nn), rho -> LDS; model_out; the observation misfit ----
  double a_obs = 0.0;
  for (int node = tid; node < nn * nn; node += 256) {
    const int r = node / nn, c = node - r * nn;
    int y0, y1, x0i, x1i;
    float ly, lx;
    bil_src(r, nel, nn, &y0, &y1, &ly);
    bil_src(c, nel, nn, &x0i, &x1i, &lx);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const float* p = xb + (size_t)d * nel * nel;
      const float top = p[y0 * nel + x0i] * (1.f - lx) + p[y0 * nel + x1i] * lx;
      const float bot = p[y1 * nel + x0i] * (1.f - lx) + p[y1 * nel + x1i] * lx;
      const float u = top * (1.f - ly) + bot * ly;
      sU[2 * node + d] = u;
      mo[(size_t)d * nn * nn + node] = u;
      const float diff = u - yb[(size_t)d * nn * nn + node];
      a_obs += (double)(mb[(size_t)d * nn * nn + node] * (diff * diff));
    }
    const bool inside = r < nel && c < nel;
    const float rho_pad = inside ? xb[(size_t)2 * nel * nel + r * nel + c] : 0.f;
    mo[(size_t)2 * nn * nn + node] = rho_pad;
    if (inside) {
      const float d2 = rho_pad - yb[(size_t)2 * nn * nn + node];
      a_obs += (double)(mb[(size_t)2 * nn * nn + node] * (d2 * d2));
    }
  }
  double rsum = 0.0;
  for (int e = tid; e < E; e += 256) {
    const float rv = xb[(size_t)2 * nel * nel + e];
    sR[e] = rv;
    rsum += rv;
  }
  __syncthreads();
  // ---- phase 2: per dof: (K_closed U)_i and the residual, left UNSCALED in Z; sum r^2 ----
  double a_r2 = 0.0, a_comp = 0.0;
  for (int i = tid; i < ndof; i += 256) {
    float ku = 0.f;
    for (int s = 0; s < 4; ++s) {
      const int e = ms.dof_elems[(i * 4 + s) * 2], a = ms.dof_elems[(i * 4 + s) * 2 + 1];
      if (e < 0) continue;
      const float* k = ms.kloc + (size_t)e * ms.kloc_stride + a * 8;
      const int* D = ms.elem_dofs + (size_t)e * 8;
      float acc = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) acc = fmaf(k[q], sU[D[q]], acc);
      ku = fmaf(sR[e], acc, ku);
    }
    const int node = i >> 1, d = i & 1;
    const bool masked = bb[(size_t)d * nn * nn + node] != 0.f;
    const float f = masked ? 0.f : bb[(size_t)(2 + d) * nn * nn + node];
    const float kbc = masked ? sU[i] : ku;
    const float res = kbc - f;
    a_r2 += (double)(res * res);
    sZ[i] = res;
    if constexpr (COMP) {
      a_comp += (double)(sU[i] * kbc);
      if constexpr (FORM == kCompEnergy) sG[i] = kbc;            // read back below by this thread only
    }
  }
  double S[NS];                          // L_obs, L_pde, sum of rho (, C)
  S[0] = a_obs;
  S[1] = a_r2;
  S[2] = rsum;
  if constexpr (COMP) S[3] = a_comp;
  block_sum_f64<NS>(S, red, tid);
  const float shift = (float)(S[2] / E) - vf[b];
  const double l_vol = (double)shift * (double)shift;
  const float so = guidance_scale(zeta_obs, S[0]), sr = guidance_scale(zeta_pde, S[1]), sv = guidance_scale(zeta_vol, l_vol);
  if (tid == 0) {
    sums[NS * b] = (float)S[0];
    sums[NS * b + 1] = (float)S[1];
    sums[NS * b + 2] = (float)l_vol;
    if constexpr (COMP) sums[NS * b + 3] = (float)S[3];
  }
  // every thread rescales the entries of Z it wrote itself: d Phi / d (K U)_i and the direct d Phi / d U_i
  for (int i = tid; i < ndof; i += 256) {
    const int node = i >> 1, d = i & 1;
    const bool masked = bb[(size_t)d * nn * nn + node] != 0.f;
    float w = sr * sZ[i];                                        // d Phi / d Kbc_i
    if constexpr (FORM == kCompEnergy) w += zeta_comp * sU[i];
    sZ[i] = masked ? 0.f : w;
    const float eo = so * (mb[(size_t)d * nn * nn + node] * (sU[i] - yb[(size_t)d * nn * nn + node]));
    float gu = (masked ? w : 0.f) + eo;
    if constexpr (FORM == kCompEnergy) gu += zeta_comp * sG[i];  // zeta_comp Kbc_i
    sG[i] = gu;
  }
  __syncthreads();
  // ---- phase 3: gU += K^T z (gather); g_rho_e = z_e^T kloc u_e + volume term + observation term ----
  for (int i = tid; i < ndof; i += 256) {
    float acc = 0.f;
    for (int s = 0; s < 4; ++s) {
      const int e = ms.dof_elems[(i * 4 + s) * 2], bq = ms.dof_elems[(i * 4 + s) * 2 + 1];
      if (e < 0) continue;
      const float* k = ms.kloc + (size_t)e * ms.kloc_stride;
      const int* D = ms.elem_dofs + (size_t)e * 8;
      float t = 0.f;
#pragma unroll
      for (int a = 0; a < 8; ++a) t = fmaf(k[a * 8 + bq], sZ[D[a]], t);   // column bq of kloc
      acc = fmaf(sR[e], t, acc);
    }
    sG[i] += acc;
  }
  const float gs = sv * shift / (float)E;                        // d Phi / d rho_e via the shift
  float* gx = v + (size_t)b * 3 * nel * nel;
  for (int e = tid; e < E; e += 256) {
    const float* k = ms.kloc + (size_t)e * ms.kloc_stride;
    const int* D = ms.elem_dofs + (size_t)e * 8;
    float acc = 0.f, se = 0.f;                                   // se = sum over the element's free dofs of U_a (k_e u_e)_a
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) t = fmaf(k[a * 8 + q], sU[D[q]], t);
      acc = fmaf(sZ[D[a]], t, acc);
      if constexpr (FORM == kCompSensitivity) {
        const int i = D[a];
        const bool masked = bb[(size_t)(i & 1) * nn * nn + (i >> 1)] != 0.f;
        se = fmaf(masked ? 0.f : sU[i], t, se);
      }
    }
    const int r = e / nel, c = e - r * nel;
    const size_t on = (size_t)2 * nn * nn + r * nn + c;
    float gr = (acc + gs) + so * (mb[on] * (sR[e] - yb[on]));
    if constexpr (FORM == kCompSensitivity) gr -= zeta_comp * se;
    gx[(size_t)2 * nel * nel + e] = gr;
  }
  __syncthreads();
  // ---- phase 4: adjoint of the bilinear up-sampling: each nel x nel pixel gathers the <= 3x3 nodes that read it ----
  for (int pix = tid; pix < nel * nel; pix += 256) {
    const int y = pix / nel, x = pix - y * nel;
    float g0 = 0.f, g1 = 0.f;
    for (int r = y - 1; r <= y + 2; ++r) {
      if (r < 0 || r >= nn) continue;
      int y0, y1;
      float ly;
      bil_src(r, nel, nn, &y0, &y1, &ly);
      const float wy = (y0 == y ? 1.f - ly : 0.f) + (y1 == y ? ly : 0.f);
      if (wy == 0.f) continue;
      for (int c = x - 1; c <= x + 2; ++c) {
        if (c < 0 || c >= nn) continue;
        int x0i, x1i;
        float lx;
        bil_src(c, nel, nn, &x0i, &x1i, &lx);
        const float wx = (x0i == x ? 1.f - lx : 0.f) + (x1i == x ? lx : 0.f);
        if (wx == 0.f) continue;
        const int node = r * nn + c;
        g0 = fmaf(wy * wx, sG[2 * node], g0);
        g1 = fmaf(wy * wx, sG[2 * node + 1], g1);
      }
    }
    gx[pix] = g0;
    gx[(size_t)nel * nel + pix] = g1;
  }
}

// candidate window [lo, hi] of Hi-grid positions whose two taps (bil_src(i, Ho, Hi)) can touch Ho-grid position y: the source
// coordinate (i + 0.5) Ho / Hi - 0.5 lies in (y - 1, y + 1), widened by one for the fp32 rounding; positions whose source is
// clamped to 0 all read y = 0.  Every candidate is confirmed with bil_src itself.
__device__ __forceinline__ void radj_window(int y, int Hi, int Ho, int* lo, int* hi) {
  const float inv_s = (float)Hi / (float)Ho;
  int l = (y == 0) ? 0 : (int)floorf(((float)y - 0.5f) * inv_s - 0.5f) - 1;
  int h = (int)ceilf(((float)y + 1.5f) * inv_s - 0.5f) + 1;
  *lo = l < 0 ? 0 : l;
  *hi = h > Hi - 1 ? Hi - 1 : h;
}

// x_prev [B,C,Ho,Ho] = c1 x0 + c2 x_t + sigma z - R^T g,  g [B,Hi*Hi,Cg] (channels 0..C-1), R = bilinear resize Ho -> Hi.
// One thread per (sample, Ho-grid pixel): it gathers, rows then columns ascending, the Hi-grid pixels that read it.
__global__ void __launch_bounds__(256) psample_update_guided_resized_kernel(const float* __restrict__ x0p, const float* __restrict__ xt,
                                                                            const float* __restrict__ z, const float* __restrict__ g,
                                                                            float c1, float c2, float sigma, float* __restrict__ out,
                                                                            int C, int Cg, int Hi, int Ho) {
  const int pix = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (pix >= Ho * Ho) return;
  const int y = pix / Ho, x = pix - y * Ho;
  int ylo, yhi, xlo, xhi;
  radj_window(y, Hi, Ho, &ylo, &yhi);
  radj_window(x, Hi, Ho, &xlo, &xhi);
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
  const float* gb = g + (size_t)b * Hi * Hi * Cg;
  for (int iy = ylo; iy <= yhi; ++iy) {
    int y0, y1;
    float ly;
    bil_src(iy, Ho, Hi, &y0, &y1, &ly);
    const float wy = (y0 == y ? 1.f - ly : 0.f) + (y1 == y ? ly : 0.f);
    if (wy == 0.f) continue;
    for (int ix = xlo; ix <= xhi; ++ix) {
      int x0i, x1i;
      float lx;
      bil_src(ix, Ho, Hi, &x0i, &x1i, &lx);
      const float wx = (x0i == x ? 1.f - lx : 0.f) + (x1i == x ? lx : 0.f);
      if (wx == 0.f) continue;
      const float* gp = gb + ((size_t)iy * Hi + ix) * Cg;
      const float w = wy * wx;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c < C) acc[c] = fmaf(w, gp[c], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (c < C) {
      const size_t o = ((size_t)b * C + c) * Ho * Ho + pix;
      out[o] = fmaf(sigma, z[o], fmaf(c2, xt[o], c1 * x0p[o])) - acc[c];
    }
}

}  // namespace pidm

using namespace pidm;

// the guards shared by the two entries (nothing is read or launched when one of them fires), then the launch of one instantiation
template <int FORM>
static int mech_guidance_launch(const char* who, const float* x0_pred, const float* bcs, const float* vf, const float* obs,
                                const float* mask, float zeta_obs, float zeta_pde, float zeta_vol, float zeta_comp, const float* kloc,
                                int kloc_stride, const int32_t* elem_dofs, const int32_t* dof_elems, int nel, float* v,
                                float* model_out, float* sums, int B, void* stream) {
  const int E = nel * nel, nn = nel + 1, ndof = 2 * nn * nn;
  if (mech_args(nel, E, ndof, kloc, elem_dofs, dof_elems)) return -1;
  if (!x0_pred || !bcs || !vf || !obs || !mask || !v || !model_out || !sums) return fail("%s: null buffer", who);
  if (B <= 0) return fail("%s: B must be positive", who);
  if (nel < 1 || (kloc_stride != 0 && kloc_stride != 64))
    return fail("%s: need nel >= 1 and kloc_stride 0 or 64 (got nel=%d kloc_stride=%d)", who, nel, kloc_stride);
  MechMesh ms{elem_dofs, dof_elems, kloc, kloc_stride, E, ndof, nel, nn};
  const size_t lds = ((size_t)3 * ndof + (size_t)E) * sizeof(float);
  if (lds > 150 * 1024) return fail("%s: mesh does not fit LDS (nel=%d needs %zu bytes of 153600)", who, nel, lds);
  static bool attr = false;               // (one per instantiation)
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mech_guidance_kernel<FORM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              150 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL(mech_guidance_kernel<FORM>, dim3((unsigned)B), dim3(256), lds, as_stream(stream), ms, x0_pred, bcs, vf, obs, mask,
                     zeta_obs, zeta_pde, zeta_vol, zeta_comp, v, model_out, sums);
  PIDM_CHECK_LAUNCH("mech_guidance_kernel");
  return 0;
}

extern "C" int pidm_mech_guidance_cotangent(const float* x0_pred, const float* bcs, const float* vf, const float* obs, const float* mask,
                                            float zeta_obs, float zeta_pde, float zeta_vol, const float* kloc, int kloc_stride,
                                            const int32_t* elem_dofs, const int32_t* dof_elems, int nel, float* v, float* model_out,
                                            float* sums, int B, void* stream) {
  return mech_guidance_launch<kCompNone>("mech_guidance_cotangent", x0_pred, bcs, vf, obs, mask, zeta_obs, zeta_pde, zeta_vol, 0.f, kloc,
                                         kloc_stride, elem_dofs, dof_elems, nel, v, model_out, sums, B, stream);
}

extern "C" int pidm_mech_guidance_cotangent_compliance(const float* x0_pred, const float* bcs, const float* vf, const float* obs,
                                                       const float* mask, float zeta_obs, float zeta_pde, float zeta_vol,
                                                       float zeta_comp, int comp_form, const float* kloc, int kloc_stride,
                                                       const int32_t* elem_dofs, const int32_t* dof_elems, int nel, float* v,
                                                       float* model_out, float* sums, int B, void* stream) {
  const char* who = "mech_guidance_cotangent_compliance";
  if (comp_form == kCompEnergy)
    return mech_guidance_launch<kCompEnergy>(who, x0_pred, bcs, vf, obs, mask, zeta_obs, zeta_pde, zeta_vol, zeta_comp, kloc, kloc_stride,
                                             elem_dofs, dof_elems, nel, v, model_out, sums, B, stream);
  if (comp_form == kCompSensitivity)
    return mech_guidance_launch<kCompSensitivity>(who, x0_pred, bcs, vf, obs, mask, zeta_obs, zeta_pde, zeta_vol, zeta_comp, kloc,
                                                  kloc_stride, elem_dofs, dof_elems, nel, v, model_out, sums, B, stream);
  return fail("%s: comp_form must be 0 (energy) or 1 (sensitivity), got %d", who, comp_form);
}

extern "C" int pidm_psample_update_guided_resized(const float* x0, const float* x_t, const float* z, const float* g_nhwc, float c1,
                                                  float c2, float sigma, float* x_prev, int B, int C, int Cg, int Hi, int Ho,
                                                  void* stream) {
  if (!x0 || !x_t || !z || !g_nhwc || !x_prev) return fail("psample_update_guided_resized: null buffer");
  if (B <= 0 || B > 65535) return fail("psample_update_guided_resized: need 0<B<=65535 (got B=%d)", B);
  if (Hi < 1 || Ho < 1 || Hi > 16384 || Ho > 16384)
    return fail("psample_update_guided_resized: need 1<=Hi,Ho<=16384 (got Hi=%d Ho=%d)", Hi, Ho);
  if (Cg <= 0 || Cg > 16) return fail("psample_update_guided_resized: Cg=%d, need 1..16", Cg);
  if (C <= 0 || C > Cg) return fail("psample_update_guided_resized: C=%d, need 1..Cg (Cg=%d)", C, Cg);
  hipLaunchKernelGGL(psample_update_guided_resized_kernel, dim3((unsigned)((Ho * Ho + 255) / 256), (unsigned)B), dim3(256), 0,
                     as_stream(stream), x0, x_t, z, g_nhwc, c1, c2, sigma, x_prev, C, Cg, Hi, Ho);
  PIDM_CHECK_LAUNCH("psample_update_guided_resized_kernel");
  return 0;
}
