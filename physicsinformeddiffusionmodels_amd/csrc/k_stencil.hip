// Classed stencil operators for gfx950: forward, adjoint, and the Darcy residual for any stencil set.
//
// Replaces (reference paths): StencilGradientComputation.forward src/grad_utils.py:64-146 (nine depthwise convolutions, nine slice
// scatters and two pads PER OPERATOR), StencilGradients.forward :161-175 (five of those for mode='all'), their autograd backward,
// and - for fd_acc != 2 or bcs='periodic' - the stencil part of ResidualsDarcy.compute_residual src/residuals_darcy.py:137-183.
//
// One workgroup per (image, tile of rows x columns).  The tile of the input plus a halo of h = largest offset of any operator of the
// launch is staged ONCE in LDS (zeros outside the image, wrapped indices when periodic), the tap lists of all operators of the launch
// sit next to it as (LDS offset, coefficient) pairs, and every thread owns four consecutive pixels of a row: where the four share a
// position class - everywhere but at most two quads per row - one walk over the class's tap list serves all four (the tap reads are
// LDS broadcasts: interior waves run the ('C','C') list without a per-lane branch).  K operators = one read of x and K writes.
// The adjoint is a GATHER: an input pixel collects, per class, from the output pixels p - d that HAVE that class (a range check per
// tap near the border, none in the interior where only ('C','C') reaches); cotangents are staged one operator at a time through the
// same LDS tile, the sum over k, classes and taps runs in table order - no atomics, bit-identical run to run.
#include "pidm_common.h"

namespace pidm {

enum { kStMaxOps = PIDM_STENCIL_MAX_OPS, kStMaxHalo = 32, kStThreads = 256, kStQuadsPerThread = 4 };

struct StOp {
  const int* table;
  float* ptr;        // forward: this operator's output; adjoint: its cotangent
  int mio, reach;    // reach = max(mio, max_offset): how far a tap of ANY class goes
  int ntaps;
  int lds;           // first word of this operator's block in the LDS table area: 18 words of (first tap, taps) per class, 3 per tap
};
struct StArgs {
  StOp op[kStMaxOps];
  int K;
};
struct StTile {
  int H, W, TR, TC, ntr, ntc, h, periodic;
};

__device__ __forceinline__ int st_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int st_wrap(int v, int n) {
  v %= n;
  return v < 0 ? v + n : v;
}
// 0 (low edge), 1 (centre), 2 (high edge)
__device__ __forceinline__ int st_class(int i, int n, int mio) { return i < mio ? 0 : (i >= n - mio ? 2 : 1); }

// tap lists of the launch -> LDS; whatever the table holds is clamped to what the launcher sized LDS and the halo for
__device__ __forceinline__ void st_stage_tables(const StArgs& a, int* tab, int LW, int h, int sign, int tid) {
  for (int k = 0; k < a.K; ++k) {
    const StOp& op = a.op[k];
    int* dst = tab + op.lds;
    if (tid < 18) {
      const int c = tid >> 1;
      const int start = st_clamp(op.table[2 * c], 0, op.ntaps);
      const int cnt = st_clamp(op.table[2 * c + 1], 0, op.ntaps - start);
      dst[tid] = (tid & 1) ? cnt : start;
    }
    for (int t = tid; t < op.ntaps; t += kStThreads) {
      const int di = st_clamp(op.table[24 + 3 * t], -h, h), dj = st_clamp(op.table[24 + 3 * t + 1], -h, h);
      dst[18 + 3 * t] = sign * (di * LW + dj);
      dst[18 + 3 * t + 1] = op.table[24 + 3 * t + 2];
      dst[18 + 3 * t + 2] = ((di + 64) << 8) | (dj + 64);
    }
  }
}

// rows [r0 - h, r0 + TR + h) x columns [c0 - h, c0 + TC + h) of image `src` -> LDS
__device__ __forceinline__ void st_stage_tile(const float* __restrict__ src, float* smem, const StTile& g, int r0, int c0, int tid) {
  const int LW = g.TC + 2 * g.h, LH = g.TR + 2 * g.h;
  int li = tid / LW, lj = tid - li * LW;
  const int dli = kStThreads / LW, dlj = kStThreads - dli * LW;
  for (int idx = tid; idx < LH * LW; idx += kStThreads) {
    int gi = r0 - g.h + li, gj = c0 - g.h + lj;
    float v = 0.f;
    if (g.periodic) {
      gi = st_wrap(gi, g.H);
      gj = st_wrap(gj, g.W);
      v = src[(size_t)gi * g.W + gj];
    } else if (gi >= 0 && gi < g.H && gj >= 0 && gj < g.W) {
      v = src[(size_t)gi * g.W + gj];
    }
    smem[idx] = v;
    li += dli;
    lj += dlj;
    if (lj >= LW) {
      lj -= LW;
      ++li;
    }
  }
}

__device__ __forceinline__ void st_store4(float* dst, const float (&v)[4], int npx) {
  if (npx == 4 && (reinterpret_cast<size_t>(dst) & 15) == 0) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    for (int m = 0; m < npx; ++m) dst[m] = v[m];
  }
}

__global__ void __launch_bounds__(kStThreads) stencil_fwd_kernel(const float* __restrict__ x, long long x_stride, StArgs a,
                                                                   long long out_stride, StTile g) {
  HIP_DYNAMIC_SHARED(float, smem)
  const int LW = g.TC + 2 * g.h, LH = g.TR + 2 * g.h;
  int* tab = reinterpret_cast<int*>(smem + LH * LW);
  const int tid = threadIdx.x;
  const int tiles = g.ntr * g.ntc;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int tr = t / g.ntc, tc = t - tr * g.ntc;
  const int r0 = tr * g.TR, c0 = tc * g.TC;
  const int r1 = (r0 + g.TR < g.H) ? r0 + g.TR : g.H, c1 = (c0 + g.TC < g.W) ? c0 + g.TC : g.W;
  st_stage_tables(a, tab, LW, g.h, 1, tid);
  st_stage_tile(x + (size_t)n * x_stride, smem, g, r0, c0, tid);
  __syncthreads();

  const int QC = (g.TC + 3) >> 2;
  for (int q = tid; q < QC * g.TR; q += kStThreads) {
    const int li = q / QC, i = r0 + li, j0 = c0 + ((q - li * QC) << 2);
    if (i >= r1 || j0 >= c1) continue;
    const int npx = (c1 - j0 < 4) ? c1 - j0 : 4;
    const int pb = (li + g.h) * LW + (j0 - c0 + g.h);
    for (int k = 0; k < a.K; ++k) {
      const StOp& op = a.op[k];
      const int* ot = tab + op.lds;
      const int rc = g.periodic ? 1 : st_class(i, g.H, op.mio);
      const int ca = g.periodic ? 1 : st_class(j0, g.W, op.mio), cb = g.periodic ? 1 : st_class(j0 + npx - 1, g.W, op.mio);
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      if (npx == 4 && ca == cb) {     // column classes are monotone along a row: equal ends = one class for the quad
        const int cls = 3 * rc + ca;
        const int* tp = ot + 18 + 3 * ot[2 * cls];
        for (int cnt = ot[2 * cls + 1]; cnt > 0; --cnt, tp += 3) {
          const float w = __uint_as_float((unsigned)tp[1]);
          const float* s = smem + pb + tp[0];
#pragma unroll
          for (int m = 0; m < 4; ++m) acc[m] = fmaf(w, s[m], acc[m]);
        }
      } else {
        for (int m = 0; m < npx; ++m) {
          const int cls = 3 * rc + (g.periodic ? 1 : st_class(j0 + m, g.W, op.mio));
          const int* tp = ot + 18 + 3 * ot[2 * cls];
          float r = 0.f;
          for (int cnt = ot[2 * cls + 1]; cnt > 0; --cnt, tp += 3) r = fmaf(__uint_as_float((unsigned)tp[1]), smem[pb + m + tp[0]], r);
          acc[m] = r;
        }
      }
      st_store4(op.ptr + (size_t)n * out_stride + (size_t)i * g.W + j0, acc, npx);
    }
  }
}

__global__ void __launch_bounds__(kStThreads) stencil_adj_kernel(StArgs a, long long g_stride, const float* __restrict__ add,
                                                                   long long add_stride, float* __restrict__ gx, long long gx_stride,
                                                                   StTile g) {
  HIP_DYNAMIC_SHARED(float, smem)
  const int LW = g.TC + 2 * g.h, LH = g.TR + 2 * g.h;
  int* tab = reinterpret_cast<int*>(smem + LH * LW);
  const int tid = threadIdx.x;
  const int tiles = g.ntr * g.ntc;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int tr = t / g.ntc, tc = t - tr * g.ntc;
  const int r0 = tr * g.TR, c0 = tc * g.TC;
  const int r1 = (r0 + g.TR < g.H) ? r0 + g.TR : g.H, c1 = (c0 + g.TC < g.W) ? c0 + g.TC : g.W;
  st_stage_tables(a, tab, LW, g.h, -1, tid);      // x[p + d] feeds y[p]  <=>  gx[p] collects from g[p - d]

  const int QC = (g.TC + 3) >> 2;
  float acc[kStQuadsPerThread][4];
#pragma unroll
  for (int s = 0; s < kStQuadsPerThread; ++s)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[s][m] = 0.f;

  for (int k = 0; k < a.K; ++k) {
    const StOp& op = a.op[k];
    if (k) __syncthreads();
    st_stage_tile(op.ptr + (size_t)n * g_stride, smem, g, r0, c0, tid);
    __syncthreads();
    const int* ot = tab + op.lds;
    // rows / columns below `inner` from either end see taps of the edge classes, or centre taps whose output pixel is an edge pixel
    const int inner = (2 * op.mio > op.mio + op.reach) ? 2 * op.mio : op.mio + op.reach;
#pragma unroll
    for (int s = 0; s < kStQuadsPerThread; ++s) {
      const int q = tid + s * kStThreads;
      if (q >= QC * g.TR) continue;
      const int li = q / QC, i = r0 + li, j0 = c0 + ((q - li * QC) << 2);
      if (i >= r1 || j0 >= c1) continue;
      const int npx = (c1 - j0 < 4) ? c1 - j0 : 4;
      const int pb = (li + g.h) * LW + (j0 - c0 + g.h);
      const bool pure = g.periodic || (i >= inner && i < g.H - inner && j0 >= inner && j0 + 3 < g.W - inner);
      if (npx == 4 && pure) {
        const int* tp = ot + 18 + 3 * ot[2 * 4];
        for (int cnt = ot[2 * 4 + 1]; cnt > 0; --cnt, tp += 3) {
          const float w = __uint_as_float((unsigned)tp[1]);
          const float* sp = smem + pb + tp[0];
#pragma unroll
          for (int m = 0; m < 4; ++m) acc[s][m] = fmaf(w, sp[m], acc[s][m]);
        }
        continue;
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (m >= npx) continue;
        const int j = j0 + m;
        float r = acc[s][m];
        if (g.periodic) {
          const int* tp = ot + 18 + 3 * ot[2 * 4];
          for (int cnt = ot[2 * 4 + 1]; cnt > 0; --cnt, tp += 3) r = fmaf(__uint_as_float((unsigned)tp[1]), smem[pb + m + tp[0]], r);
        } else {
          for (int rc = 0; rc < 3; ++rc) {
            // output rows of class rc: [rlo, rhi); they reach input rows within `reach` of them
            const int rlo = rc == 0 ? 0 : (rc == 1 ? op.mio : g.H - op.mio), rhi = rc == 0 ? op.mio : (rc == 1 ? g.H - op.mio : g.H);
            if (i < rlo - op.reach || i >= rhi + op.reach) continue;
            for (int cc = 0; cc < 3; ++cc) {
              const int clo = cc == 0 ? 0 : (cc == 1 ? op.mio : g.W - op.mio), chi = cc == 0 ? op.mio : (cc == 1 ? g.W - op.mio : g.W);
              if (j < clo - op.reach || j >= chi + op.reach) continue;
              const int cls = 3 * rc + cc;
              const int* tp = ot + 18 + 3 * ot[2 * cls];
              for (int cnt = ot[2 * cls + 1]; cnt > 0; --cnt, tp += 3) {
                const int di = (tp[2] >> 8) - 64, dj = (tp[2] & 255) - 64;
                const int qi = i - di, qj = j - dj;
                if ((unsigned)(qi - rlo) < (unsigned)(rhi - rlo) && (unsigned)(qj - clo) < (unsigned)(chi - clo))
                  r = fmaf(__uint_as_float((unsigned)tp[1]), smem[pb + m + tp[0]], r);
              }
            }
          }
        }
        acc[s][m] = r;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kStQuadsPerThread; ++s) {
    const int q = tid + s * kStThreads;
    if (q >= QC * g.TR) continue;
    const int li = q / QC, i = r0 + li, j0 = c0 + ((q - li * QC) << 2);
    if (i >= r1 || j0 >= c1) continue;
    const int npx = (c1 - j0 < 4) ? c1 - j0 : 4;
    float v[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) v[m] = acc[s][m];
    if (add) {
      const float* ap = add + (size_t)n * add_stride + (size_t)i * g.W + j0;
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (m < npx) v[m] = ap[m] + v[m];
    }
    st_store4(gx + (size_t)n * gx_stride + (size_t)i * g.W + j0, v, npx);
  }
}

// ---- launch planning ---------------------------------------------------------------------------------------------------------
static int st_plan(const pidm_stencil_op* ops, int K, int N, int H, int W, int periodic, StArgs* a, StTile* g, size_t* lds,
                   const char* what) {
  if (!ops) return fail("%s: null operator array", what);
  if (K < 1 || K > kStMaxOps) return fail("%s: 1..%d operators per launch (got %d)", what, (int)kStMaxOps, K);
  if (N <= 0 || H <= 0 || W <= 0) return fail("%s: need N, H, W > 0 (got %d, %d, %d)", what, N, H, W);
  int h = 0, words = 0;
  a->K = K;
  for (int k = 0; k < K; ++k) {
    const pidm_stencil_op& o = ops[k];
    if (!o.table) return fail("%s: operator %d has no table", what, k);
    if (o.mio < 0 || o.max_offset < 0 || o.ntaps < 0 || o.ntaps > 9 * PIDM_STENCIL_MAX_TAPS)
      return fail("%s: operator %d: mio=%d max_offset=%d ntaps=%d out of range", what, k, o.mio, o.max_offset, o.ntaps);
    const int reach = periodic ? o.mio : (o.mio > o.max_offset ? o.mio : o.max_offset);
    if (reach > kStMaxHalo) return fail("%s: operator %d reaches %d pixels (limit %d)", what, k, reach, (int)kStMaxHalo);
    const int need = periodic ? 2 * o.mio + 1 : (2 * o.mio > o.mio + o.max_offset ? 2 * o.mio : o.mio + o.max_offset);
    if (H < need || W < need)
      return fail("%s: a %d x %d image is too small for operator %d (mio=%d, max_offset=%d, periodic=%d: needs %d per axis)", what, H,
                  W, k, o.mio, o.max_offset, periodic, need);
    a->op[k].table = o.table;
    a->op[k].ptr = nullptr;
    a->op[k].mio = o.mio;
    a->op[k].reach = reach;
    a->op[k].ntaps = o.ntaps;
    a->op[k].lds = words;
    words += 18 + 3 * o.ntaps;
    if (reach > h) h = reach;
  }
  const int TC = (W <= 128) ? W : 64, QC = (TC + 3) / 4, LW = TC + 2 * h;
  const int ntc = (W + TC - 1) / TC;
  int cap = (kStThreads * kStQuadsPerThread) / QC;                 // quads a workgroup owns
  const int cap_lds = (64 * 1024 / 4) / LW - 2 * h;               // 64 KB of tile
  if (cap_lds < cap) cap = cap_lds;
  if (cap < 1) return fail("%s: no tile of a %d-wide image with a halo of %d fits LDS", what, W, h);
  // enough workgroups to fill the chip where the batch alone does not provide them, but bands no thinner than the halo they re-read
  const long long wgs = (long long)N * ntc;
  int want = (int)((1024 + wgs - 1) / wgs);
  int TR = (H + want - 1) / want;
  const int thin = (h > 8) ? h : 8;
  if (TR < thin) TR = thin;
  if (TR > cap) TR = cap;
  if (TR > H) TR = H;
  const int ntr = (H + TR - 1) / TR;
  if ((long long)N * ntr * ntc > 0x7fffffffLL) return fail("%s: %d images x %d tiles exceed the grid", what, N, ntr * ntc);
  g->H = H; g->W = W; g->TR = TR; g->TC = TC; g->ntr = ntr; g->ntc = ntc; g->h = h; g->periodic = periodic ? 1 : 0;
  *lds = ((size_t)(TR + 2 * h) * LW + (size_t)words) * 4;
  return 0;
}

static int launch_stencil_fwd(const float* x, long long x_stride, const pidm_stencil_op* ops, float* const* outs, int K,
                              long long out_stride, int N, int H, int W, int periodic, hipStream_t st) {
  StArgs a;
  StTile g;
  size_t lds;
  if (int rc = st_plan(ops, K, N, H, W, periodic, &a, &g, &lds, "stencil_apply")) return rc;
  if (!x || !outs) return fail("stencil_apply: null buffer");
  for (int k = 0; k < K; ++k) {
    if (!outs[k]) return fail("stencil_apply: output %d is null", k);
    a.op[k].ptr = outs[k];
  }
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stencil_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
    attr = true;
  }
  hipLaunchKernelGGL(stencil_fwd_kernel, dim3((unsigned)N * g.ntr * g.ntc), dim3(kStThreads), lds, st, x, x_stride, a, out_stride, g);
  PIDM_CHECK_LAUNCH("stencil_fwd_kernel");
  return 0;
}

static int launch_stencil_adj(const float* const* gs, long long g_stride, const pidm_stencil_op* ops, int K, const float* add,
                              long long add_stride, float* gx, long long gx_stride, int N, int H, int W, int periodic, hipStream_t st) {
  StArgs a;
  StTile g;
  size_t lds;
  if (int rc = st_plan(ops, K, N, H, W, periodic, &a, &g, &lds, "stencil_apply_adjoint")) return rc;
  if (!gs || !gx) return fail("stencil_apply_adjoint: null buffer");
  for (int k = 0; k < K; ++k) {
    if (!gs[k]) return fail("stencil_apply_adjoint: cotangent %d is null", k);
    a.op[k].ptr = const_cast<float*>(gs[k]);
  }
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stencil_adj_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
    attr = true;
  }
  hipLaunchKernelGGL(stencil_adj_kernel, dim3((unsigned)N * g.ntr * g.ntc), dim3(kStThreads), lds, st, a, g_stride, add, add_stride, gx,
                     gx_stride, g);
  PIDM_CHECK_LAUNCH("stencil_adj_kernel");
  return 0;
}

// ---- Darcy residual on top of the operators: the pointwise part (src/residuals_darcy.py:146-183) -------------------------------
// d: six fields [B][P*P]: p_0, p_1, p_00, p_11, K_0, K_1
__global__ void __launch_bounds__(256) darcy_general_assemble_kernel(const float* __restrict__ x0, const float* __restrict__ f_s,
                                                                      const float* __restrict__ d, float bc1_sign,
                                                                      float* __restrict__ residual, int B, int P) {
  const size_t N = (size_t)P * P, total = (size_t)B * N;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t b = idx / N;
  const int n = (int)(idx - b * N), i = n / P, j = n - i * P;
  const float Kv = x0[b * 2 * N + N + n];
  const float p0 = d[idx], p1 = d[total + idx], p00 = d[2 * total + idx], p11 = d[3 * total + idx], K0 = d[4 * total + idx],
              K1 = d[5 * total + idx];
  // reference op order: vj00 = -K*p00 - K0*p0 ; vj11 = -K*p11 - K1*p1 ; eq = vj00 + vj11 - f_s
  const float vj00 = -Kv * p00 - K0 * p0;
  const float vj11 = -Kv * p11 - K1 * p1;
  const float s0 = (i == 0) ? -1.f : ((i == P - 1) ? 1.f : 0.f);
  const float s1 = (j == 0) ? bc1_sign : ((j == P - 1) ? -bc1_sign : 0.f);
  float* r = residual + idx * 3;
  r[0] = vj00 + vj11 - f_s[n];
  r[1] = s0 * p0;
  r[2] = s1 * p1;
}

// c: six cotangent fields [B][P*P]: on p_0, p_1, p_00 (= p_11: both carry -K g), on K_0, K_1, and the direct term on K
__global__ void __launch_bounds__(256) darcy_general_adjoint_kernel(const float* __restrict__ x0, const float* __restrict__ grad_res,
                                                                     const float* __restrict__ d, float bc1_sign, float* __restrict__ c,
                                                                     int B, int P) {
  const size_t N = (size_t)P * P, total = (size_t)B * N;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t b = idx / N;
  const int n = (int)(idx - b * N), i = n / P, j = n - i * P;
  const float Kv = x0[b * 2 * N + N + n];
  const float p0 = d[idx], p1 = d[total + idx], p00 = d[2 * total + idx], p11 = d[3 * total + idx], K0 = d[4 * total + idx],
              K1 = d[5 * total + idx];
  const float* gr = grad_res + idx * 3;
  const float gq = gr[0], gb0 = gr[1], gb1 = gr[2];
  const float s0 = (i == 0) ? -1.f : ((i == P - 1) ? 1.f : 0.f);
  const float s1 = (j == 0) ? bc1_sign : ((j == P - 1) ? -bc1_sign : 0.f);
  c[idx] = -K0 * gq + s0 * gb0;
  c[total + idx] = -K1 * gq + s1 * gb1;
  c[2 * total + idx] = -Kv * gq;
  c[3 * total + idx] = -p0 * gq;
  c[4 * total + idx] = -p1 * gq;
  c[5 * total + idx] = -(p00 + p11) * gq;
}

static int darcy_general_derivs(const float* x0, const pidm_stencil_op* ops4, int periodic, float* d, int B, int P, hipStream_t st) {
  const long long N = (long long)P * P, total = (long long)B * N;
  float* outs_p[4] = {d, d + total, d + 2 * total, d + 3 * total};
  float* outs_k[2] = {d + 4 * total, d + 5 * total};
  if (int rc = launch_stencil_fwd(x0, 2 * N, ops4, outs_p, 4, N, B, P, P, periodic, st)) return rc;
  return launch_stencil_fwd(x0 + N, 2 * N, ops4, outs_k, 2, N, B, P, P, periodic, st);
}

static int darcy_general_check(const void* a, const void* b, const void* c, const void* ws, int B, int P) {
  if (!a || !b || !c || !ws) return fail("darcy_residual_general: null buffer");
  if (B <= 0 || P < 2 || (long long)B * P * P > 0x7fffffffLL / 4) return fail("darcy_residual_general: B=%d P=%d out of range", B, P);
  return 0;
}

}  // namespace pidm

using namespace pidm;

extern "C" int pidm_stencil_apply(const float* x, long long x_stride, const pidm_stencil_op* ops_host, float* const* outs_host, int K,
                                  long long out_stride, int N, int H, int W, int periodic, void* stream) {
  return launch_stencil_fwd(x, x_stride, ops_host, outs_host, K, out_stride, N, H, W, periodic, as_stream(stream));
}

extern "C" int pidm_stencil_apply_adjoint(const float* const* gs_host, long long g_stride, const pidm_stencil_op* ops_host, int K,
                                          const float* add, long long add_stride, float* gx, long long gx_stride, int N, int H, int W,
                                          int periodic, void* stream) {
  return launch_stencil_adj(gs_host, g_stride, ops_host, K, add, add_stride, gx, gx_stride, N, H, W, periodic, as_stream(stream));
}

extern "C" int pidm_stencil_plan(const pidm_stencil_op* ops_host, int K, int N, int H, int W, int periodic, int* out6) {
  StArgs a;
  StTile g;
  size_t lds;
  if (int rc = st_plan(ops_host, K, N, H, W, periodic, &a, &g, &lds, "stencil_plan")) return rc;
  if (!out6) return fail("stencil_plan: null buffer");
  out6[0] = g.TR; out6[1] = g.TC; out6[2] = g.ntr; out6[3] = g.ntc; out6[4] = g.h; out6[5] = (int)lds;
  return 0;
}

extern "C" size_t pidm_darcy_general_ws(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  return (size_t)12 * B * P * P * sizeof(float);
}

extern "C" int pidm_darcy_residual_general_fwd(const float* x0, const float* f_s, const pidm_stencil_op* ops4_host, int periodic,
                                               float bc1_sign, float* residual, void* workspace, int B, int P, void* stream) {
  if (int rc = darcy_general_check(x0, f_s, residual, workspace, B, P)) return rc;
  hipStream_t st = as_stream(stream);
  float* d = reinterpret_cast<float*>(workspace);
  if (int rc = darcy_general_derivs(x0, ops4_host, periodic, d, B, P, st)) return rc;
  const size_t total = (size_t)B * P * P;
  hipLaunchKernelGGL(darcy_general_assemble_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x0, f_s, d, bc1_sign,
                     residual, B, P);
  PIDM_CHECK_LAUNCH("darcy_general_assemble_kernel");
  return 0;
}

extern "C" int pidm_darcy_residual_general_bwd(const float* x0, const float* grad_res, const pidm_stencil_op* ops4_host, int periodic,
                                               float bc1_sign, float* grad_x0, void* workspace, int B, int P, void* stream) {
  if (int rc = darcy_general_check(x0, grad_res, grad_x0, workspace, B, P)) return rc;
  hipStream_t st = as_stream(stream);
  const long long N = (long long)P * P, total = (long long)B * N;
  float* d = reinterpret_cast<float*>(workspace);
  float* c = d + 6 * total;
  if (int rc = darcy_general_derivs(x0, ops4_host, periodic, d, B, P, st)) return rc;
  hipLaunchKernelGGL(darcy_general_adjoint_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x0, grad_res, d, bc1_sign, c,
                     B, P);
  PIDM_CHECK_LAUNCH("darcy_general_adjoint_kernel");
  // grad wrt p: D0^T c0 + D1^T c1 + D00^T (-K g) + D11^T (-K g);  grad wrt K: direct + D0^T c3 + D1^T c4
  const float* gs_p[4] = {c, c + total, c + 2 * total, c + 2 * total};
  const float* gs_k[2] = {c + 3 * total, c + 4 * total};
  if (int rc = launch_stencil_adj(gs_p, N, ops4_host, 4, nullptr, 0, grad_x0, 2 * N, B, P, P, periodic, st)) return rc;
  return launch_stencil_adj(gs_k, N, ops4_host, 2, c + 5 * total, N, grad_x0 + N, 2 * N, B, P, P, periodic, st);
}
