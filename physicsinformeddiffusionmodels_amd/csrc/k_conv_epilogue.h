// Epilogue helpers shared by the fp32 (k_conv_fp32.hip) and the split-form (k_conv.hip) convolution kernels: GroupNorm statistics and
// GroupNorm-backward sums of a wave's 32-pixel x 32-channel output tile, computed while the tile is still in registers.
#pragma once
#include "pidm_common.h"

namespace pidm {
// GroupNorm partial statistics of a wave's 32-pixel x 32-channel output tile (ConvGeom::gn_part): each lane holds the sums over
// its 16 rows of one channel; butterfly over the gn_cpg lanes of a group and the two lane halves, one lane per group writes.
#define PIDM_GN_PARTIAL(s1_, s2_, b_, pix_in_img_, c_)                                                              \
  {                                                                                                                 \
    float a1__ = (s1_), a2__ = (s2_);                                                                               \
    for (int off__ = 1; off__ < g.gn_cpg; off__ <<= 1) {                                                            \
      a1__ += __shfl_xor(a1__, off__);                                                                              \
      a2__ += __shfl_xor(a2__, off__);                                                                              \
    }                                                                                                               \
    a1__ += pidm_other_half(a1__);                                                                                   \
    a2__ += pidm_other_half(a2__);                                                                                   \
    if (half == 0 && (l31 & (g.gn_cpg - 1)) == 0) {                                                                 \
      double* o__ = g.gn_part + (((size_t)(b_) * g.gn_nchunk + ((pix_in_img_) >> 5)) * g.gn_G + (c_) / g.gn_cpg) * 2; \
      o__[0] = (double)a1__;                                                                                        \
      o__[1] = (double)a2__;                                                                                        \
    }                                                                                                               \
  }
// GroupNorm-backward partial sums from a dgrad epilogue (ConvGeom::bn_part).  acc_ = the lane's 16 rows of dy for channel c_
// (rows (r&3) + 8(r>>2) + 4half of the wave's 32 pixels), xrow_ = &x[first pixel of the wave][c_], xstep_ = floats between
// consecutive pixels of the wave in x.  Same arithmetic as gn_recompute (k_norm.hip).
// res_on_ (wave-uniform, from kernel arguments): the epilogue adds a residual; rrow_ is evaluated only then.  The optional loads
// (FiLM rows, residual rows) sit behind SCALAR conditions as batches: with a per-lane `ptr ? ptr[..] : 0` hipcc gave each of the 16
// residual rows a branch, a reload of its spilled offset and s_waitcnt vmcnt(0) - 16 memory round trips in the epilogue of every
// input-gradient launch that leaves these sums (ISA of conv3x3_split_ws_kernel, round 6).
#define PIDM_BN_PARTIAL(acc_, bv_, b_, pix_in_img_, c_, xrow_, xstep_, res_on_, rrow_, rstep_)                      \
  {                                                                                                                 \
    const int gI__ = (c_) / g.bn_cpg;                                                                               \
    const float mean__ = g.bn_stats[((size_t)(b_) * g.bn_G + gI__) * 2], rstd__ = g.bn_stats[((size_t)(b_) * g.bn_G + gI__) * 2 + 1]; \
    const float gm__ = g.bn_gamma[(c_)], bt__ = g.bn_beta[(c_)];                                                    \
    float sc__ = 1.f, sh__ = 0.f;                                                                                   \
    if (g.bn_ss) {                                                                                                  \
      sc__ = 1.f + (g.bn_ss[(size_t)(b_) * g.bn_ldss + (c_)] + g.bn_ssb[(c_)]);                                     \
      sh__ = g.bn_ss[(size_t)(b_) * g.bn_ldss + g.Cout + (c_)] + g.bn_ssb[g.Cout + (c_)];                           \
    }                                                                                                               \
    float xv__[16], rv__[16];                                                                                       \
    _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                                  \
        xv__[r] = (xrow_)[(unsigned)((r & 3) + 8 * (r >> 2) + 4 * half) * (unsigned)(xstep_)];   /* 32-bit row offsets */ \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) rv__[r] = 0.f;                                                   \
    if (res_on_) {                                                                                                  \
      const float* rr__ = (rrow_);                                                                                  \
      _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                                \
          rv__[r] = rr__[(unsigned)((r & 3) + 8 * (r >> 2) + 4 * half) * (unsigned)(rstep_)];                       \
    }                                                                                                               \
    float a1__ = 0.f, a2__ = 0.f;                                                                                   \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                                \
      const float xh__ = (xv__[r] - mean__) * rstd__;                                                               \
      const float v__ = (xh__ * gm__ + bt__) * sc__ + sh__;                                                         \
      const float sg__ = pidm_sigmoid(v__);                                                                         \
      const float dv__ = (((acc_)[r] + (bv_)) + rv__[r]) * (sg__ * (1.f + v__ * (1.f - sg__)));                     \
      a1__ += dv__;                                                                                                 \
      a2__ += dv__ * xh__;                                                                                          \
    }                                                                                                               \
    a1__ += pidm_other_half(a1__);                                                                                   \
    a2__ += pidm_other_half(a2__);                                                                                   \
    if (half == 0) {                                                                                                \
      double* o__ = g.bn_part + (((size_t)(b_) * g.bn_nchunk + ((pix_in_img_) >> 5)) * g.Cout + (c_)) * 2;          \
      o__[0] = (double)a1__;                                                                                        \
      o__[1] = (double)a2__;                                                                                        \
    }                                                                                                               \
  }

// ---------------------------------------------------------------------------------------------------------------------------
// GroupNorm finished inside the workgroup (ConvGeom::gf_out / bf_dx; split-form 3x3 kernels whose tile holds whole images).
// A wave's sums go to the LDS rows below in front of the stage barrier; behind it every wave totals the rows of ITS image and
// normalises the 32 x 32 tile it still holds in registers.  Row = the wave's 32-pixel sub-tile st of the workgroup tile (an image
// = gn_nchunk consecutive sub-tiles), 32 lanes x (s1, s2) doubles per row: forward, the first lane of a group carries the group's
// sums; backward, every lane its channel's.  The additions repeat those of gn_finalize_stats / gn_bwd_apply_kernel (k_norm.hip)
// term by term - float sums per wave, doubles across waves, nl interleaved runs added in order - so that a build without FMA
// contraction (the host emulator's) gives the bits of the separate kernels.
// ---------------------------------------------------------------------------------------------------------------------------
static constexpr int kFzRow = 32 * 2;     // doubles per sub-tile row
// The separate kernels are built with -ffp-contract=fast, and which multiply-add pairs hipcc fuses there decides their last bits
// (ISA of gn_apply_kernel, gn_bwd_apply_kernel and of PIDM_BN_PARTIAL inside the split kernels).  The functions below switch
// contraction off and spell those fused operations out, so that the gfx950 build gives the bits of the separate launches too;
// the host emulator's build contracts nothing anywhere, there a fused operation is a product and a sum.
#if defined(__HIP_DEVICE_COMPILE__)
#define PIDM_FZ_FMAF(a_, b_, c_) __builtin_fmaf((a_), (b_), (c_))
#define PIDM_FZ_FMA(a_, b_, c_) __builtin_fma((a_), (b_), (c_))
#else
#define PIDM_FZ_FMAF(a_, b_, c_) ((a_) * (b_) + (c_))
#define PIDM_FZ_FMA(a_, b_, c_) ((a_) * (b_) + (c_))
#endif
// bytes of those rows for a tile of nw sub-tiles (the launchers add them to the kernel's dynamic LDS)
static inline size_t fz_lds_bytes(int nw) { return (size_t)nw * kFzRow * sizeof(double); }

// S = sum over the n rows from p (stride kFzRow): run ln takes rows ln, ln + nl, ...; the runs are added in order
__device__ __forceinline__ void pidm_fz_sum_rows(const double* p, int n, int nl, double& S1, double& S2) {
#pragma clang fp contract(off)
  S1 = 0.0;
  S2 = 0.0;
  for (int ln = 0; ln < nl && ln < n; ++ln) {
    double s = 0.0, t = 0.0;
    for (int k = ln; k < n; k += nl) {
      s += p[(size_t)k * kFzRow];
      t += p[(size_t)k * kFzRow + 1];
    }
    S1 += s;
    S2 += t;
  }
}

// a lane's 16 values (rows (r & 3) + 8 (r >> 2) + 4 half of the wave's 32 pixels, channel l31) as 16-byte stores of four
// channels per pixel (4x4 register transposes inside lane quads, as in the convolution epilogues); res != null: added, laid out
// like dst and fetched as one batch
__device__ __forceinline__ void pidm_fz_store_tile(const float (&v)[16], float* __restrict__ dst, const float* __restrict__ res,
                                                   size_t opix, size_t sox, int half, int l31) {
#pragma clang fp contract(off)
  // (the per-lane row offsets are formed here, once per tile: as loop invariants of the stage loop hipcc kept them in registers
  //  across the MFMA stages and spilled them)
  PIDM_OPAQUE_I32(half);
  PIDM_OPAQUE_I32(l31);
  const bool odd1 = (l31 & 1) != 0, odd2 = (l31 & 2) != 0;
  f32x4 rres[4];
  if (res) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) rres[q4] = *reinterpret_cast<const f32x4*>(res + opix + (size_t)(8 * q4 + 4 * half + (l31 & 3)) * sox);
  }
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    float x0 = v[4 * q4], x1 = v[4 * q4 + 1], x2 = v[4 * q4 + 2], x3 = v[4 * q4 + 3];
    const float r01 = pidm_quad_xor1(odd1 ? x0 : x1), r23 = pidm_quad_xor1(odd1 ? x2 : x3);
    x0 = odd1 ? r01 : x0; x1 = odd1 ? x1 : r01;
    x2 = odd1 ? r23 : x2; x3 = odd1 ? x3 : r23;
    const float r02 = pidm_quad_xor2(odd2 ? x0 : x2), r13 = pidm_quad_xor2(odd2 ? x1 : x3);
    x0 = odd2 ? r02 : x0; x2 = odd2 ? x2 : r02;
    x1 = odd2 ? r13 : x1; x3 = odd2 ? x3 : r13;
    f32x4 o = {x0, x1, x2, x3};
    if (res) o += rres[q4];
    *reinterpret_cast<f32x4*>(dst + opix + (size_t)(8 * q4 + 4 * half + (l31 & 3)) * sox) = o;
  }
}

// forward, in front of the barrier: the wave's group sums (PIDM_GN_PARTIAL's additions) to its LDS row
__device__ __forceinline__ void pidm_fz_fwd_put(const ConvGeom& g, double* __restrict__ rows, int st, float s1, float s2, int half, int l31) {
#pragma clang fp contract(off)
  float a1 = s1, a2 = s2;
  for (int off = 1; off < g.gn_cpg; off <<= 1) {
    a1 += __shfl_xor(a1, off);
    a2 += __shfl_xor(a2, off);
  }
  a1 += pidm_other_half(a1);
  a2 += pidm_other_half(a2);
  if (half == 0 && (l31 & (g.gn_cpg - 1)) == 0) {
    double* o = rows + ((size_t)st * 32 + l31) * 2;
    o[0] = (double)a1;
    o[1] = (double)a2;
  }
}
// forward, behind the barrier: statistics of the image as gn_finalize_stats forms them, then gn_apply_kernel's arithmetic on the
// wave's tile v (the convolution output incl. bias).  b / pin / n0: image, first pixel inside it and first channel of the tile.
__device__ __forceinline__ void pidm_fz_fwd_finish(const ConvGeom& g, const double* __restrict__ rows, int st, int b, int pin, int n0,
                                                   const float (&v)[16], int half, int l31) {
#pragma clang fp contract(off)
  const int c = n0 + l31;
  // per-channel constants as one batch of loads without branches (gn_load_consts, k_norm.hip): without FiLM the four slots read gamma
  const float* const sp = g.gf_ss ? g.gf_ss + (size_t)b * g.gf_ldss : g.gf_gamma;
  const float* const bp = g.gf_ss ? g.gf_ssb : g.gf_gamma;
  const int oC = g.gf_ss ? g.Cout : 0;
  const float gm = g.gf_gamma[c], bt = g.gf_beta[c], s0 = sp[c], b0 = bp[c], s1 = sp[oC + c], b1 = bp[oC + c];
  const int cpi = g.gn_nchunk, st0 = st & ~(cpi - 1), l0 = l31 & ~(g.gn_cpg - 1);
  double S1, S2;
  pidm_fz_sum_rows(rows + ((size_t)st0 * 32 + l0) * 2, cpi, g.gf_nl, S1, S2);
  const double count = (double)(32 * cpi) * (double)g.gn_cpg;
  const double mean = S1 / count;
  double var = PIDM_FZ_FMA(-mean, mean, S2 / count);
  if (var < 0.0) var = 0.0;
  const float mf = (float)mean, rf = (float)(1.0 / sqrt(var + (double)1e-5f));
  if (st == st0 && half == 0 && l31 == l0) {
    float* so = g.gf_stats + ((size_t)b * g.gn_G + (c >> __builtin_ctz(g.gn_cpg))) * 2;
    so[0] = mf;
    so[1] = rf;
  }
  const float a = rf * gm;
  const float sc1 = g.gf_ss ? 1.f + (s0 + b0) : 1.f, sh = g.gf_ss ? s1 + b1 : 0.f;
  // the residual joins the SiLU's product in ONE fused operation there: it is fetched in the accumulator layout (one channel per
  // lane, 16 rows), as one batch behind a scalar condition
  float y[16], rr[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) rr[r] = 0.f;
  if (g.gf_res) {
    int hr = half;
    PIDM_OPAQUE_I32(hr);
    const float* rrow = g.gf_res + ((size_t)b * (32 * cpi) + pin) * g.Cout + c;
#pragma unroll
    for (int r = 0; r < 16; ++r) rr[r] = rrow[(unsigned)((r & 3) + 8 * (r >> 2) + 4 * hr) * (unsigned)g.Cout];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float t = PIDM_FZ_FMAF(sc1, PIDM_FZ_FMAF(a, v[r] - mf, bt), sh);
    y[r] = PIDM_FZ_FMAF(t, pidm_sigmoid(t), rr[r]);
  }
  const size_t opix = ((size_t)b * (32 * cpi) + pin) * g.Cout + n0 + 4 * (l31 >> 2);
  pidm_fz_store_tile(y, g.gf_out, nullptr, opix, (size_t)g.Cout, half, l31);
}

// backward: what a lane keeps of its tile across the barrier
struct FzBwdKeep {
  float dv[16], xh[16];
  float rstd, gm, bt, sc1, ps0, psb0;
};
// backward, in front of the barrier: dv = dy SiLU'(v) and xhat per value (PIDM_BN_PARTIAL's arithmetic, no residual), the wave's
// per-channel sums to its LDS row.  acc_ + bv = the lane's 16 rows of dy, xrow = &x[first pixel of the wave][c], pixels Cout apart.
template <typename ACC>
__device__ __forceinline__ void pidm_fz_bwd_put(const ConvGeom& g, double* __restrict__ rows, int st, const ACC& acc, float bv, int b, int c,
                                                const float* __restrict__ xrow, int half, int l31, FzBwdKeep& k) {
#pragma clang fp contract(off)
  PIDM_OPAQUE_I32(half);               // (row offsets formed per tile, not kept across the stage loop: pidm_fz_store_tile)
  const int gI = c >> __builtin_ctz(g.bn_cpg);
  const float mean = g.bn_stats[((size_t)b * g.bn_G + gI) * 2];
  k.rstd = g.bn_stats[((size_t)b * g.bn_G + gI) * 2 + 1];
  const float* const sp = g.bn_ss ? g.bn_ss + (size_t)b * g.bn_ldss : g.bn_gamma;
  const float* const bp = g.bn_ss ? g.bn_ssb : g.bn_gamma;
  const int oC = g.bn_ss ? g.Cout : 0;
  k.gm = g.bn_gamma[c];
  k.bt = g.bn_beta[c];
  k.ps0 = sp[c];
  k.psb0 = bp[c];
  const float s1 = sp[oC + c], b1 = bp[oC + c];
  float xv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) xv[r] = xrow[(unsigned)((r & 3) + 8 * (r >> 2) + 4 * half) * (unsigned)g.Cout];
  k.sc1 = g.bn_ss ? 1.f + (k.ps0 + k.psb0) : 1.f;
  const float sh = g.bn_ss ? s1 + b1 : 0.f;
  float a1 = 0.f, a2 = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float xh = (xv[r] - mean) * k.rstd;
    const float v = PIDM_FZ_FMAF(k.sc1, PIDM_FZ_FMAF(k.gm, xh, k.bt), sh);
    const float sg = pidm_sigmoid(v);
    const float d = sg * PIDM_FZ_FMAF(v, 1.f - sg, 1.f);
    const float dy = (acc[r] + bv) + 0.f;
    const float dv = dy * d;
    k.xh[r] = xh;
    k.dv[r] = dv;
    a1 = PIDM_FZ_FMAF(dy, d, a1);
    a2 = PIDM_FZ_FMAF(xh, dv, a2);
  }
  a1 += pidm_other_half(a1);
  a2 += pidm_other_half(a2);
  if (half == 0) {
    double* o = rows + ((size_t)st * 32 + l31) * 2;
    o[0] = (double)a1;
    o[1] = (double)a2;
  }
}
// backward, behind the barrier: gn_bwd_apply_kernel's coefficient pass for the lane's channel (chunk sums, the per-image
// dgamma / dbeta and FiLM rows, group means over the gn_cpg lanes of the group in channel order) and its dx for the wave's tile
__device__ __forceinline__ void pidm_fz_bwd_finish(const ConvGeom& g, const double* __restrict__ rows, int st, int b, int pin, int n0,
                                                   const FzBwdKeep& k, int half, int l31) {
#pragma clang fp contract(off)
  const int c = n0 + l31, C = g.Cout;
  const int cpi = g.bn_nchunk, st0 = st & ~(cpi - 1);
  double S1, S2;
  pidm_fz_sum_rows(rows + ((size_t)st0 * 32 + l31) * 2, cpi, g.bf_nl, S1, S2);
  const double gm = k.gm, bt = k.bt;
  const double sc1 = g.bn_ss ? 1.0 + ((double)k.ps0 + (double)k.psb0) : 1.0;
  if (st == st0 && half == 0) {
    if (g.bn_ss) {
      g.bf_dss[(size_t)b * g.bn_ldss + c] = (float)PIDM_FZ_FMA(bt, S1, gm * S2);      // d scale
      g.bf_dss[(size_t)b * g.bn_ldss + C + c] = (float)S1;                    // d shift
    }
    g.bf_dgb[((size_t)b * 2 + 0) * C + c] = (float)(sc1 * S2);
    g.bf_dgb[((size_t)b * 2 + 1) * C + c] = (float)(sc1 * S1);
  }
  const double ga = gm * sc1 * S1, gb = gm * sc1 * S2;
  const int lane0 = (half << 5) + (l31 & ~(g.bn_cpg - 1));
  double a = 0.0, d = 0.0;
  for (int j = 0; j < g.bn_cpg; ++j) {
    a += __shfl(ga, lane0 + j);
    d += __shfl(gb, lane0 + j);
  }
  const double n = (double)g.bn_cpg * (double)(32 * cpi);
  const float k1 = (float)(a / n), k2 = (float)(d / n);
  float o[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = k.rstd * PIDM_FZ_FMAF(-k.xh[r], k2, PIDM_FZ_FMAF(k.dv[r] * k.sc1, k.gm, -k1));
  const size_t opix = ((size_t)b * (32 * cpi) + pin) * C + n0 + 4 * (l31 >> 2);
  pidm_fz_store_tile(o, g.bf_dx, nullptr, opix, (size_t)C, half, l31);
}
}  // namespace pidm
