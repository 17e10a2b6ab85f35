/* pidm.h - C ABI of libpidm_hip.so, the MI355X (gfx950) engine behind the reference's Python API.
 *
 * The reference (jhbastek/PhysicsInformedDiffusionModels) is pure Python/PyTorch and has no FFI of its
 * own; the "binding a maintainer would add" is a ctypes stub.  Each entry point below
 * names the reference code it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  All pointers are DEVICE pointers unless
 *     the name ends in _host.  The library never allocates or frees caller memory, never synchronises
 *     the device, and enqueues every kernel on the caller-supplied stream (a hipStream_t passed as
 *     void*; NULL = the null stream).
 *   - return 0 on success, negative on error; message via pidm_last_error() (thread-local).
 *   - fp32 everywhere; image tensors are channels-last (NHWC, i.e. the reference's own [B, P*P, C]
 *     "b_xy_c" interchange layout) unless stated.
 */
#ifndef PIDM_H
#define PIDM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIDM_ABI_VERSION 1

int pidm_version(void);
const char* pidm_last_error(void);
/* "hip" for the product library, "hipemu" for the host-emulated test build (tests/hipemu). */
const char* pidm_backend(void);

/* bench-only: per-launch timing of the dominant kernels with HIP events recorded on the launch stream.
 * class 0 = conv forward/dgrad on the fp32 MFMA (work = algorithmic FLOPs), class 1 = conv wgrad on the fp32 MFMA,
 * class 2 / 3 = the same two in split form on the bf16 pipe (each launch is in exactly one class). */
int pidm_prof_enable(int on);
int pidm_prof_collect(double* ms4, long long* launches4, double* work4);
/* bench-only, per KERNEL: between _begin and _collect every launch of the library records one event on `stream` (graph replay and
 * the side-stream overlap are off meanwhile, so launches are back to back on that stream); a launch's time is the interval since
 * the previous launch's event.  _collect writes one line per kernel name, largest total first:
 *   name \t launches \t total_ms \t work \t class \n   (work: FLOPs the launcher declared, 0 = none; class as above, -1 = none)
 * and returns the bytes the table needs incl. the terminating 0 (the text is truncated to `cap`), or -1.
 * Single-threaded by contract: between _begin and _collect only ONE host thread may call into the library. */
int pidm_prof_kernels_begin(void* stream);
long long pidm_prof_kernels_collect(char* buf, size_t cap);

/* ---------------------------------------------------------------------------------------------
 * Darcy PDE residual                    replaces ResidualsDarcy.compute_residual's stencil part
 *   src/residuals_darcy.py:137-183 + StencilGradientComputation.forward src/grad_utils.py:64-146
 * x0      [B,2,P,P] NCHW (ch0 = pressure, ch1 = permeability) - the layout the reference UNet returns
 * residual[B,P*P,3]  (eq, bc0, bc1)
 * inv_h0 = 1/d0, inv_h1 = 1/d1 (d1 negative when reverse_d1).  f_s [P*P] source field.
 * A null buffer, B <= 0, P < 5 or a P whose row bands do not fit LDS is refused before anything is launched (Darcy loss included).
 * ------------------------------------------------------------------------------------------- */
int pidm_darcy_residual_fwd(const float* x0, const float* f_s, float inv_h0, float inv_h1,
                            float* residual, int B, int P, void* stream);
/* adjoint: grad_x0[B,2,P,P] = (d residual / d x0)^T grad_res[B,P*P,3] */
int pidm_darcy_residual_bwd(const float* x0, const float* grad_res, float inv_h0, float inv_h1,
                            float* grad_x0, int B, int P, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused PIDM loss (Darcy, mean estimation)          replaces DenoisingDiffusion.model_estimation_loss
 *   src/denoising_utils.py:666-692  (data term with min-SNR weight + residual virtual likelihood)
 * x0, x0_pred [B,2,P,P] NCHW; p2w[B] = p2_loss_weight[t_b]; inv_var[B] = 1/posterior_variance_clipped[t_b]
 * out_scalars[4] = {loss, c_data*data_loss, mean|r|, 0};  grad_x0_pred [B,2,P,P] = d loss / d x0_pred.
 * residual [B,P*P,3] is written as a by-product (the API returns it).  workspace: >= pidm_darcy_loss_ws(B,P) bytes.
 * ------------------------------------------------------------------------------------------- */
size_t pidm_darcy_loss_ws(int B, int P);
int pidm_darcy_loss_fwd_bwd(const float* x0, const float* x0_pred, const float* f_s, const float* p2w,
                            const float* inv_var, float c_data, float c_residual, float inv_h0, float inv_h1,
                            float* residual, float* grad_x0_pred, float* out_scalars, void* workspace,
                            int B, int P, void* stream);
/* The same with the per-sample weights looked up inside the kernel: t int64 [B] (the step's time levels), p2w_table =
 * diff_dict['p2_loss_weight'], var_table = diff_dict['posterior_variance_clipped'] (its reciprocal is taken in the kernel) -
 * replaces the two extract() gathers + the reciprocal of src/denoising_utils.py:677,689-692 as well. */
int pidm_darcy_loss_fwd_bwd_t(const float* x0, const float* x0_pred, const float* f_s, const int64_t* t,
                              const float* p2w_table, const float* var_table, float c_data, float c_residual,
                              float inv_h0, float inv_h1, float* residual, float* grad_x0_pred, float* out_scalars,
                              void* workspace, int B, int P, void* stream);

/* CoCoGen residual correction: max over all entries of d residual / d p per sample
 *   replaces the dense vmap(jacfwd) Jacobian of src/residuals_darcy.py:217-231 (400 MB per 64x64 sample) by the
 *   analytic stencil rows.  x0: [B,2,P,P] (p, K); max_dr_dp: [B]. */
int pidm_darcy_jacobian_max(const float* x0, float inv_h0, float inv_h1, float* max_dr_dp, int B, int P, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Classed stencil operators (k_stencil.hip)     replaces StencilGradientComputation src/grad_utils.py:27-146
 *   (nine depthwise convolutions + nine slice scatters per operator) and StencilGradients.forward :161-175.
 * An operator is what the reference's constructor builds from a findiff stencil dictionary: `mio` = largest |offset| of the
 * ('C','C') stencil, `max_offset` = largest over the other eight classes, and a tap list per position class.  Pixel (i, j) of an
 * H x W image has row class L (0) if i < mio, H (2) if i >= H - mio, else C (1); columns alike with W; its value is the sum, in
 * table order, of coefficient * x[i + di, j + dj] over the taps of class 3 * row class + column class.  periodic != 0: only class
 * 4 (C, C), indices wrapped (F.pad(mode='circular'), :76-81).
 * table (device, int32 words): [2c], [2c+1] = first tap and number of taps of class c (c = 0..8); [18] mio, [19] max_offset,
 * [20] taps in total, [21..23] reserved; from word 24 on three words per tap: di, dj, fp32 bits of the coefficient.
 * Up to PIDM_STENCIL_MAX_TAPS taps per class.  mio / max_offset / ntaps of the descriptor are the launcher's copy of words 18-20 (the
 * launcher never reads device memory); the kernels clamp what they read from the table to them.
 * Non-periodic needs H, W >= max(2 mio, mio + max_offset), periodic H, W >= 2 mio + 1 (an error otherwise: the reference
 * differentiates its zero padding there).
 * ------------------------------------------------------------------------------------------- */
#define PIDM_STENCIL_MAX_OPS 5
#define PIDM_STENCIL_MAX_TAPS 49
typedef struct pidm_stencil_op {
  const int32_t* table;
  int mio, max_offset, ntaps;
} pidm_stencil_op;
/* K operators (1..5) on N images x[n * x_stride + i * W + j] in ONE launch, one read of x:
 * outs_host[k][n * out_stride + i * W + j] = (S_k x_n)[i, j].  ops_host and outs_host are HOST arrays read during the call (each
 * output has its own base pointer, all share the image stride: a [.., K, H, W] stack is written directly).  Strides in floats. */
int pidm_stencil_apply(const float* x, long long x_stride, const pidm_stencil_op* ops_host, float* const* outs_host, int K,
                       long long out_stride, int N, int H, int W, int periodic, void* stream);
/* adjoint: gx[n * gx_stride + ..] = (add ? add[n * add_stride + ..] : 0) + sum_k S_k^T g_k, as a gather in a fixed order (k, then
 * class, then tap): no atomics, bit-identical run to run.  gs_host: HOST array of the K cotangent base pointers (image stride
 * g_stride).  Replaces the autograd backward of the convolutions / scatters above. */
int pidm_stencil_apply_adjoint(const float* const* gs_host, long long g_stride, const pidm_stencil_op* ops_host, int K,
                               const float* add, long long add_stride, float* gx, long long gx_stride, int N, int H, int W,
                               int periodic, void* stream);
/* The launch plan both entries above give K operators on N images of H x W, without a launch (host only): out6 = rows and columns
 * of a tile (TR, TC), tiles along the rows and the columns (ntr, ntc), the halo h and the dynamic LDS bytes of a workgroup.  The
 * same refusals as the launches (operator count, sizes, reach, image too small). */
int pidm_stencil_plan(const pidm_stencil_op* ops_host, int K, int N, int H, int W, int periodic, int* out6);
/* Darcy residual for ANY stencil set      replaces src/residuals_darcy.py:137-183 with fd_acc / bcs as constructor arguments.
 * Same tensors as pidm_darcy_residual_fwd / _bwd; ops4_host = the operators d/d0, d/d1, d2/d0^2, d2/d1^2; bc1_sign = +1 when
 * reverse_d1 (:175-180); the boundary rows keep their meaning under periodic.  A composition that stays on the device: two
 * stencil launches + one pointwise kernel forward, the same + the pointwise adjoint + two adjoint launches backward.
 * workspace: >= pidm_darcy_general_ws(B, P) bytes. */
size_t pidm_darcy_general_ws(int B, int P);
int pidm_darcy_residual_general_fwd(const float* x0, const float* f_s, const pidm_stencil_op* ops4_host, int periodic, float bc1_sign,
                                    float* residual, void* workspace, int B, int P, void* stream);
int pidm_darcy_residual_general_bwd(const float* x0, const float* grad_res, const pidm_stencil_op* ops4_host, int periodic,
                                    float bc1_sign, float* grad_x0, void* workspace, int B, int P, void* stream);

/* q-sample  x_t = a[t_b] x0 + am1[t_b] eps          replaces src/denoising_utils.py:633-638
 * writes x_t in channels-last [B,P*P,C] (what the UNet consumes) from NCHW x0/eps. */
int pidm_qsample_nhwc(const float* x0, const float* eps, const float* a_t, const float* am1_t, float* xt_nhwc,
                      int B, int C, int HW, void* stream);
/* the same with the extract() gathers folded in: t int64 [B], a_table = diff_dict['alphas_bar_sqrt'],
 * am1_table = diff_dict['one_minus_alphas_bar_sqrt']  (src/denoising_utils.py:302-306,633-638) */
int pidm_qsample_nhwc_t(const float* x0, const float* eps, const int64_t* t, const float* a_table, const float* am1_table,
                        float* xt_nhwc, int B, int C, int HW, void* stream);
/* ancestral update x_{t-1} = c1 x0_pred + c2 x_t + sigma z   replaces src/denoising_utils.py:441-455 */
int pidm_psample_update(const float* x0_pred, const float* x_t, const float* z, float c1, float c2, float sigma,
                        float* x_prev, size_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Posterior guidance of the Darcy sampler (csrc/k_guidance.hip; no counterpart in the reference: an extension).
 * Per sample, with x = the x0 estimate, y = observations, m = 0/1 mask (all [B,2,P,P], channel 0 = p, 1 = K):
 *   L_obs = sum m (x - y)^2,  L_pde = sum r(x)^2 over the three residual channels,
 *   Phi = zeta_obs sqrt(L_obs) + zeta_pde sqrt(L_pde),  v = dPhi/dx (a term whose L is exactly 0 is omitted: no NaN, no epsilon).
 * sums [B,2] = (L_obs, L_pde), fp32 roundings of fp64 fixed-tree sums: bit-identical run to run and across batch sizes.
 *
 * pidm_darcy_guidance_cotangent: second-order, non-periodic stencils (the kernel of pidm_darcy_residual_fwd / _bwd), v and sums in
 * ONE launch, one workgroup per sample with the sample and its adjoint operands resident in LDS: 5 <= P <= 71 (8 P^2 floats of
 * LDS); anything else fails with a message. */
int pidm_darcy_guidance_cotangent(const float* x0_pred, const float* obs, const float* mask, const float* f_s, float inv_h0,
                                  float inv_h1, float zeta_obs, float zeta_pde, float* v, float* sums, int B, int P, void* stream);
/* Any stencil set: sits between pidm_darcy_residual_general_fwd (-> residual [B,P*P,3]) and _bwd.  Writes sums, grad_res =
 * zeta_pde r / sqrt(L_pde) (the input of the general adjoint) and v_obs = the observation part of v; pidm_guidance_add then adds
 * the adjoint's result: v[i] += adjoint[i], n elements. */
int pidm_guidance_scale_general(const float* x0_pred, const float* obs, const float* mask, const float* residual, float zeta_obs,
                                float zeta_pde, float* grad_res, float* v_obs, float* sums, int B, int P, void* stream);
int pidm_guidance_add(float* v, const float* adjoint, size_t n, void* stream);
/* Flux observations.  The Darcy flux of a sample is q = (q0, q1) = (-K D0 p, -K D1 p) [B,2,P,P] with D0 / D1 the residual's own
 * first-derivative operators (order fd_acc, classed or periodic, spacing d0 / d1).  With readings y_q under a 0/1 mask m_q
 * (both [B,2,P,P]): L_flux = sum m_q (q - y_q)^2 and Phi gains zeta_flux sqrt(L_flux); with e_c = m_q,c (q_c - y_q,c) and
 * s_f = zeta_flux / sqrt(L_flux) the new part of v is  v_p += s_f sum_c D_c^T (-K e_c),  v_K += s_f (-sum_c e_c D_c p)
 * (omitted, like the other terms, when L_flux is exactly 0).
 *
 * pidm_darcy_flux: q of x0 for any stencil set.  ops2_host = the operators d/d0, d/d1.  One two-operator stencil launch on p and
 * one pointwise kernel.  workspace: >= pidm_darcy_flux_ws(B, P) bytes; on return it holds D0 p [B,P*P] followed by D1 p [B,P*P]. */
size_t pidm_darcy_flux_ws(int B, int P);
int pidm_darcy_flux(const float* x0, const pidm_stencil_op* ops2_host, int periodic, float* flux, void* workspace, int B, int P,
                    void* stream);
/* pidm_darcy_guidance_cotangent with the flux term: second-order, non-periodic stencils, v and sums [B,3] = (L_obs, L_pde, L_flux)
 * in ONE launch.  Same LDS plan (8 P^2 floats), so the same 5 <= P <= 71: the sums are taken in a first pass that stores nothing,
 * a second pass rebuilds the stencil values from the resident sample and stores the adjoint operands already scaled, flux part
 * included; anything else fails with a message. */
int pidm_darcy_guidance_cotangent_flux(const float* x0_pred, const float* obs, const float* mask, const float* flux_obs,
                                       const float* flux_mask, const float* f_s, float inv_h0, float inv_h1, float zeta_obs,
                                       float zeta_pde, float zeta_flux, float* v, float* sums, int B, int P, void* stream);
/* Any stencil set, any P: the flux term on top of the composition above, after pidm_guidance_add.  dp0 / dp1 [B,P*P] = D0 p, D1 p
 * (the first two fields pidm_darcy_residual_general_fwd / _bwd leave in their workspace, or the workspace of pidm_darcy_flux / one
 * pidm_stencil_apply on p).  Writes sums3 [B,3] = (sums2[b,0], sums2[b,1], L_flux) (sums2 [B,2] may be NULL: only the flux slot is
 * written), w [B,2,P,P] = s_f (-K e_c), and the K channel v_out = v_in + s_f (-sum_c e_c D_c p) (v_out == v_in is allowed).  The
 * p channel is then ONE pidm_stencil_apply_adjoint of (d/d0, d/d1) over w with add = the p channel of v_in, gx = that of v_out
 * (distinct buffers). */
int pidm_guidance_flux_general(const float* x0_pred, const float* dp0, const float* dp1, const float* flux_obs, const float* flux_mask,
                               float zeta_flux, const float* sums2, float* sums3, float* w, const float* v_in, float* v_out, int B,
                               int P, void* stream);
/* guided ancestral update x_{t-1} = c1 x0_pred + c2 x_t + sigma z - g; g [B,HW,C] is the UNet's input-gradient layout
 * (pidm_unet_backward_input), read transposed; everything else [B,C,HW].  C <= 16. */
int pidm_psample_update_guided(const float* x0_pred, const float* x_t, const float* z, const float* g_nhwc, float c1, float c2,
                               float sigma, float* x_prev, int B, int C, int HW, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused global-norm clip + Adam over flat fp32 buffers    replaces main.py:165-166
 *   torch.nn.utils.clip_grad_norm_(model.parameters(), 1.) ; optimizer.step()   (torch.optim.Adam, no weight decay/amsgrad)
 * param/grad/exp_avg/exp_avg_sq: n floats each, 16-byte aligned; `step` is the 1-based update count (bias correction);
 * max_norm <= 0 disables clipping; total_norm_out (device float, may be NULL) receives the pre-clip global L2 norm.
 * workspace: pidm_clip_adam_ws_bytes() bytes.  Deterministic (fixed-order sums). */
size_t pidm_clip_adam_ws_bytes(void);
int pidm_clip_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                        double beta2, double eps, long long step, double max_norm, float* total_norm_out, void* workspace,
                        void* stream);

/* The same step with the parameter EMA of main.py:178-179 folded in (EMA.update, src/denoising_utils.py:174-177):
 *   shadow = (1 - mu) * p_new + mu * shadow   with the reference's fp32 roundings (two products, one sum; no fma),
 * so the shadow is bit-identical to the reference's per-tensor update applied to the same p_new.  ema_shadow: n floats.
 * pidm_ema_update is the stand-alone form (one read of p and shadow, one write of shadow) for steps taken by another
 * optimizer. */
int pidm_clip_adam_ema_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema_shadow, size_t n,
                            double lr, double beta1, double beta2, double eps, long long step, double max_norm, double ema_mu,
                            float* total_norm_out, void* workspace, void* stream);
int pidm_ema_update(float* ema_shadow, const float* param, size_t n, double ema_mu, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mechanics residual r = K(rho) u - f, matrix-free      replaces ResidualsMechanics.compute_residual
 *   src/residuals_mechanics_K.py:198-274 (dense 8450x8450 index_put assembly + einsum) and resize_image :10-21
 * x0_pred [B,3,nel,nel] NCHW (u1,u2,rho); bcs [B,4,nel+1,nel+1] (bc_x, bc_y, load_x, load_y); vf [B]
 * mesh: kloc [E,8,8] (kloc_stride 64) or one 8x8 (stride 0); elem_dofs int32 [E,8]; dof_elems int32 [ndof,4,2]
 * outputs: residual [B,ndof]; model_out [B,3,nel+1,nel+1] (u bilinearly resized, rho zero padded);
 * comp_shift [B,2] = (compliance u^T K u, mean(rho) - vf).  The adjoint takes gradients of all four.
 * ------------------------------------------------------------------------------------------- */
int pidm_bilinear_resize(const float* in, float* out, int BC, int Hi, int Ho, void* stream);
int pidm_mech_residual_fwd(const float* x0_pred, const float* bcs, const float* vf, const float* kloc, int kloc_stride,
                           const int32_t* elem_dofs, const int32_t* dof_elems, int nel, float* residual, float* model_out,
                           float* comp_shift, int B, void* stream);
int pidm_mech_residual_bwd(const float* x0_pred, const float* bcs, const float* kloc, int kloc_stride,
                           const int32_t* elem_dofs, const int32_t* dof_elems, int nel, const float* g_residual,
                           const float* g_model_out, const float* g_comp_shift, float* g_x0_pred, int B, void* stream);

/* Fused mechanics training loss + its gradient wrt the network output     replaces src/denoising_utils.py:666-708 (loss
 * algebra on top of compute_residual) for gov_eqs == 'mechanics': data term on model_out = (u resized to nn x nn, rho zero padded)
 * against target x_0 [B,3,nn,nn], residual term, the [B,B]-broadcast inequality term (:697, only when c_ineq > 0) and the
 * compliance term, all with injected per-sample p2_loss_weight[t_b] and 1/posterior_variance_clipped[t_b].
 * inv_var_sum (device float, may be NULL): value to use for sum_i inv_var_i in the inequality term instead of the local sum -
 * under data parallelism the caller passes the all-rank sum divided by the number of ranks (it depends on t only), which makes
 * the rank-averaged loss and gradient equal to the single-process global-batch ones.
 * out_scalars[8]: loss, data loss, mean |r|, mean shift (0 unless c_ineq > 0), mean compliance, 0, 0, 0.
 * grad_x0_pred [B,3,nel,nel] = d loss / d x0_pred.  workspace: pidm_mech_loss_ws(B) bytes. */
size_t pidm_mech_loss_ws(int B);
int pidm_mech_loss_fwd_bwd(const float* x0_pred, const float* target, const float* bcs, const float* vf, const float* p2w,
                           const float* inv_var, const float* inv_var_sum, float c_data, float c_residual, float c_ineq,
                           float lambda_opt, const float* kloc, int kloc_stride, const int32_t* elem_dofs, const int32_t* dof_elems,
                           int nel, float* grad_x0_pred, float* out_scalars, void* workspace, int B, void* stream);

/* Topology-optimisation evaluation block      replaces src/residuals_mechanics_K.py:276-347,369-380
 *   pidm_mech_apply:  residual = K_closed(rho) u - f and comp_uf = u.f for nodal displacement images u [B,2,nn,nn]
 *                     (the "residual of opt_disp should be zero" check and compliance_data, :293-296)
 *   pidm_mech_solve:  u = K_closed(rho')^-1 f per sample (reference: torch.linalg.solve on the dense 8450^2 matrix, :321-323)
 *                     by Jacobi-preconditioned CG on the matrix-free operator in fp64; rho' = rho if bin_threshold < 0,
 *                     else (rho > bin_threshold ? bin_hi : bin_lo)  (:299-301).  compliance[b] = f.u, rho_mean[b] = mean(rho').
 *                     Stops at ||r|| <= rtol ||f|| or max_iter; iters / relres (may be NULL) report what happened.
 *   pidm_floating_material: number of 8-connected components of {rho > threshold} per sample (cv2.connectedComponents, :369-380)
 * rho: [B, nel*nel]; bcs: [B,4,nn,nn]; workspace: pidm_mech_solve_ws_bytes(nel, B). */
int pidm_mech_apply(const float* rho, const float* u_img, const float* bcs, const float* kloc, int kloc_stride,
                    const int32_t* elem_dofs, const int32_t* dof_elems, int nel, float* residual, float* comp_uf, int B,
                    void* stream);
size_t pidm_mech_solve_ws_bytes(int nel, int B);
int pidm_mech_solve(const float* rho, const float* bcs, const float* kloc, int kloc_stride, const int32_t* elem_dofs,
                    const int32_t* dof_elems, int nel, float bin_threshold, float bin_hi, float bin_lo, int max_iter,
                    double rtol, float* u_dofs, float* compliance, float* rho_mean, int32_t* iters, float* relres,
                    void* workspace, int B, void* stream);
int pidm_floating_material(const float* rho, float threshold, int nel, int32_t* n_components, int B, void* stream);

/* Posterior guidance of the mechanics sampler (csrc/k_guidance_mech.hip; no counterpart in the reference: an extension).
 * With the quantities of pidm_mech_residual_fwd for an x0 estimate x0_pred [B,3,nel,nel] (nn = nel + 1): model_out [B,3,nn,nn] =
 * (u bilinearly resized, rho zero padded), r = the row-replaced residual, shift = mean(rho) - vf; observations obs and a 0/1 mask
 * (both [B,3,nn,nn]).  Per sample
 *   L_obs = sum mask (model_out - obs)^2  (channel 2 over rows and columns < nel only: the zero padding is no part of the state,
 *           whatever the mask says there),   L_pde = sum r^2,   L_vol = shift^2,
 *   Phi = zeta_obs sqrt(L_obs) + zeta_pde sqrt(L_pde) + zeta_vol sqrt(L_vol)   (a term whose L is exactly 0 is omitted).
 * ONE launch, one workgroup per sample on the LDS plan of the fused loss ((3 ndof + E) floats, so the same mesh limit): writes
 * v [B,3,nel,nel] = dPhi/dx0_pred, model_out, and sums [B,3] = (L_obs, L_pde, L_vol) whatever the weights are; the sums are fp32
 * roundings of fp64 fixed-tree sums (bit-identical run to run and across batch sizes). */
int pidm_mech_guidance_cotangent(const float* x0_pred, const float* bcs, const float* vf, const float* obs, const float* mask,
                                 float zeta_obs, float zeta_pde, float zeta_vol, const float* kloc, int kloc_stride,
                                 const int32_t* elem_dofs, const int32_t* dof_elems, int nel, float* v, float* model_out, float* sums,
                                 int B, void* stream);
/* The same launch with a compliance term.  C = U . A(rho) U = sum_i U_i (A U)_i with A the closed stiffness ((A U)_i = U_i on a
 * clamped dof, sum_e rho_e (k_e u_e)_i on a free one): the `compliance` of pidm_mech_residual_fwd, SIGNED, entering Phi linearly
 * (never clamped, square-rooted or omitted).  comp_form selects what v gains:
 *   0 'energy'       Phi += zeta_comp C, differentiated through U and rho (the functional of the training loss's lambda_opt term);
 *   1 'sensitivity'  the adjoint (SIMP) sensitivity of the true compliance f^T K(rho)^-1 f evaluated at the predicted displacement:
 *                    the gradient of -zeta_comp sg(U) . A(rho) sg(U) (sg = stop-gradient), i.e. the density channel of v gains
 *                    -zeta_comp sum_{a : dof D_e[a] free} U_{D_e[a]} (k_e u_e)_a and the displacement channels gain nothing.  The
 *                    sampler steps AGAINST v, so a positive weight adds material where the strain energy is.
 * sums [B,4] = (L_obs, L_pde, L_vol, C) whatever the weights and the form are.  zeta_comp = 0 gives the v, model_out and first
 * three sums of pidm_mech_guidance_cotangent.  Same LDS plan, mesh limit, fixed-order fp64 sums and guards; comp_form outside
 * {0, 1} is refused.  The weights are user parameters; the defaults of the Python layer are placeholders: no trained
 * checkpoint was available and no sample quality is claimed. */
int pidm_mech_guidance_cotangent_compliance(const float* x0_pred, const float* bcs, const float* vf, const float* obs,
                                            const float* mask, float zeta_obs, float zeta_pde, float zeta_vol, float zeta_comp,
                                            int comp_form, const float* kloc, int kloc_stride, const int32_t* elem_dofs,
                                            const int32_t* dof_elems, int nel, float* v, float* model_out, float* sums, int B,
                                            void* stream);
/* guided ancestral update on a state that the network sees resized: x_prev = c1 x0 + c2 x_t + sigma z - R^T g, everything
 * [B,C,Ho,Ho] except g [B,Hi*Hi,Cg] (the UNet's input-gradient layout, channels 0..C-1 used).  R = pidm_bilinear_resize Ho -> Hi.
 * Gather form, fixed order.  Any Hi, Ho >= 1; 1 <= C <= Cg <= 16; B <= 65535. */
int pidm_psample_update_guided_resized(const float* x0, const float* x_t, const float* z, const float* g_nhwc, float c1, float c2,
                                       float sigma, float* x_prev, int B, int C, int Cg, int Hi, int Ho, void* stream);

/* Darcy training-data generation      replaces src/darcy_data_generation.py:118-163 (generate_sample: findiff assembly + dense lstsq)
 *   pidm_darcy_gen_acc: per sample b, K = exp(basis^T z_b) (basis [q, P*P] row-major, sqrt(eigenvalue)-scaled KLE modes; z [B, q],
 *                   1 <= q <= P^2) or, when z is NULL, K = K_in[b] ([B, P*P]); then p = the least-squares solution of the
 *                   reference's (P^2+4P+1) x P^2 system: A p = -K p_00 - K_0 p_0 - K p_11 - K_1 p_1 = f_s (spacings d0 / d1;
 *                   d1 < 0 for reverse_dy), boundary rows -D0 p (x-min), +D0 p (x-max), bc_sign D1 p (y-min), -bc_sign D1 p
 *                   (y-max) = 0, integral row int_w . p = 0 (f_s, int_w [P*P]).  The 1-D operators are findiff's classed ones of
 *                   order acc in {2, 4, 6} (src/darcy_data_generation.py:129-142, every FinDiff(..., acc=acc)): rows i < acc/2
 *                   forward, rows i > P-1-acc/2 backward, the others central; central and one-sided first-derivative stencils
 *                   have acc+1 taps, one-sided second-derivative stencils acc+2.  K_0 and K_1 come from the same operators.
 *                   Matrix-free column-scaled CGLS in fp64 on the system without the integral row, then the constant-mode shift;
 *                   stops at ||S A^T r|| <= rtol ||S A^T b|| or max_iter.  Every vector of the iteration stays on chip (four
 *                   fp64 fields of P^2 live in LDS).  This entry and pidm_darcy_gen_periodic run one solver,
 *                   csrc/k_darcy_gen_cgls.h, with the 1-D operators of csrc/k_darcy_gen_acc.hip / csrc/k_darcy_gen_per.hip.
 *                   Outputs: K_out [B, P*P] (may be NULL), p_out [B, P*P], res_mean [B] = mean |row residual| over all
 *                   P^2+4P+1 rows, iters [B], relres [B] = ||S A^T r|| / ||S A^T b|| (each of the last three may be NULL).  All
 *                   arrays fp64 on the device (iters int32); basis may be NULL when z is, K_in when z is given.
 *                   Launch protocol - one call runs at most iters_this_launch (>= 1) CGLS iterations per sample that is not done
 *                   and returns; the caller repeats the call (first_launch = 0, every other argument unchanged) until done[b] != 0
 *                   for every b.  first_launch != 0 initialises `state` (whatever it held).  A sample is finished when it
 *                   converges (||S A^T r|| <= rtol ||S A^T b||) or reaches max_iter iterations in total; the launch that
 *                   finishes it runs the deflation and the residual pass and writes p_out[b], res_mean[b], iters[b], relres[b]
 *                   and done[b] = 1, once; later launches leave a finished sample untouched.  An unfinished sample gets
 *                   done[b] = 0.  K_out is written by the first launch.  A solve cut into launches of any size returns bit-identical
 *                   results to the same solve in one launch.
 *                   state (device, pidm_darcy_gen_acc_state_bytes(P, B) bytes, 8-byte aligned), per sample 3 P^2 + 4P + 3 doubles:
 *                   iterate | search direction | row residuals (P^2 each) | boundary residuals (4P) | gamma | gamma0 | two int32
 *                   (iterations done, done flag).  K, K_0, K_1 and the column scales are recomputed by every launch.
 *                   done [B] int32 (device, required).  Limits: 8 <= P <= 64 at acc 2 and 4, 10 <= P <= 64 at acc 6 (the forward
 *                   second derivative of row 2 reaches column 9); anything else, a null state or iters_this_launch < 1 is an error.
 *   pidm_darcy_gen_acc_lds_bytes: LDS per workgroup (four P^2 fields, 4P boundary residuals, the 3 x (acc+2) x 2 unit-spacing
 *                   coefficient table shared by both axes, the reduction slots); the entry fails when it exceeds the 160 KB of a
 *                   gfx950 workgroup.  0 for an order other than 2, 4, 6. */
size_t pidm_darcy_gen_acc_state_bytes(int P, int B);
size_t pidm_darcy_gen_acc_lds_bytes(int P, int acc);
int pidm_darcy_gen_acc(const double* basis, const double* z, int q, const double* K_in, int P, int acc, double d0, double d1,
                       double bc_sign, const double* int_w, const double* f_s, int max_iter, double rtol, int iters_this_launch,
                       int first_launch, void* state, double* K_out, double* p_out, double* res_mean, int32_t* iters,
                       double* relres, int32_t* done, int B, void* stream);
/*   pidm_darcy_gen_periodic: the same system under periodic boundary conditions - src/darcy_data_generation.py:129-163 with every
 *                   FinDiff(..., acc=acc) replaced by its central stencil of order acc in {2, 4, 6} on wrapped indices (tap i + o
 *                   reads point (i + o) mod P on both axes), the operators of ResidualsDarcy(bcs='periodic'); the reference's
 *                   generator has no such mode (main.py's bcs = 'periodic' reaches training only).  K_0 and K_1 come from the same
 *                   operators.  The four boundary row sets stay: -(D0 p) on row 0, +(D0 p) on row P-1, bc_sign (D1 p) on column 0,
 *                   -bc_sign (D1 p) on column P-1, with the wrapped D0 / D1.  Arguments, launch protocol, `state` layout (size:
 *                   pidm_darcy_gen_acc_state_bytes(P, B)) and outputs as pidm_darcy_gen_acc.  Limits: 8 <= P <= 64 at every order
 *                   (the wrapped stencil of order 6 spans 7 points); anything else, a null state or iters_this_launch < 1 is an
 *                   error.
 *   pidm_darcy_gen_periodic_lds_bytes: LDS per workgroup (four P^2 fields, 4P boundary residuals, the (acc+2) x 2 coefficient
 *                   table, the reduction slots).  0 for an order other than 2, 4, 6. */
size_t pidm_darcy_gen_periodic_lds_bytes(int P, int acc);
int pidm_darcy_gen_periodic(const double* basis, const double* z, int q, const double* K_in, int P, int acc, double d0, double d1,
                            double bc_sign, const double* int_w, const double* f_s, int max_iter, double rtol,
                            int iters_this_launch, int first_launch, void* state, double* K_out, double* p_out, double* res_mean,
                            int32_t* iters, double* relres, int32_t* done, int B, void* stream);

/* Mechanics training-data generation     replaces nothing in the reference: it never generated its topology-optimisation samples
 * (they were downloaded); these entries supply the data main.py:90-101 expects (one [65,65,10] .npy per sample), DESIGN section 4b
 *   pidm_simp_step: ONE iteration of SIMP compliance minimisation for B samples, one workgroup per sample, all in fp64, stateless:
 *                   (x [B, nel*nel] densities, u [B, ndof] warm start) -> (x_new, u_out = the solved displacements).  Per sample:
 *                     1. E_e = e_min + x_e^penal (1 - e_min)
 *                     2. K_closed(E) u = f by Jacobi-preconditioned CG on the matrix-free operator of pidm_mech_solve (bcs as there:
 *                        a non-zero entry of channels 0/1 pins that dof - identity row, f = 0; channels 2/3 are the loads), started
 *                        from u; stops at ||r|| <= pcg_rtol ||f|| or pcg_max_iter; the initial residual is tested too, so a
 *                        converged warm start costs 0 iterations and comes back unchanged
 *                     3. ce_e = u_e^T k_e u_e,  c = sum_e E_e ce_e,  dc_e = -penal x_e^(penal-1) (1 - e_min) max(ce_e, 0)
 *                        (the fp32 element stiffness is indefinite by its rounding: a rigidly moving element can show ce_e < 0)
 *                     4. dc~_e = sum_j H_ej x_j dc_j / (max(1e-3, x_e) sum_j H_ej),  H_ej = max(0, rmin - dist(e, j)) over the
 *                        window of ceil(rmin) - 1 elements each way, clipped at the domain edge
 *                     5. optimality criteria with exactly n_bisect bisection steps on lambda in [0, 1e9] (no tolerance exit):
 *                        x_new = max(0, max(x - move, min(1, min(x + move, x sqrt(-dc~ / lambda))))),
 *                        mean(x_new) > vf => l1 = lambda, else l2 = lambda; the x_new of the last step is the result
 *                   compliance [B] = c, change [B] = max |x_new - x|, pcg_iters [B], relres [B] = ||r|| / ||f|| at exit.
 *                   active (int32 [B], may be NULL): a sample with active[b] == 0 is copied through (x_new = x, u_out = u) and its
 *                   four scalar outputs are not written.  Reductions run in a fixed order: results are bit-identical run to run and
 *                   across batch sizes.  x_new / u_out must not alias x / u; mesh tables 16-byte aligned.  2 <= nel <= 79 (the search direction and the moduli
 *                   live in LDS), rmin > 1, n_bisect >= 1, penal >= 1, 0 < e_min < 1.
 *                   workspace: pidm_simp_ws_bytes(nel, B).
 *   pidm_simp_step_filtered: the same iteration in the three-field form: x are design variables, the density filter
 *                   x~ = (H x) / Hs (H_ej as in step 4 above, Hs_e = sum_j H_ej) and, for filter = 2, the projection
 *                   x^ = (tanh(beta eta) + tanh(beta (x~ - eta))) / (tanh(beta eta) + tanh(beta (1 - eta))) give the physical density
 *                   (filter = 1: x^ = x~).  Launch, precision, `active`, reductions, limits and workspace as pidm_simp_step.  Per sample:
 *                     1. x~, x^, d = dx^/dx~ (1, or beta (1 - tanh^2(beta (x~ - eta))) / (tanh(beta eta) + tanh(beta (1 - eta))),
 *                        evaluated as beta / cosh^2(..) / (..));  E_e = e_min + x^_e^penal (1 - e_min)
 *                     2. K_closed(E) u = f: the CG phase of pidm_simp_step, the same device function
 *                     3. ce_e = u_e^T k_e u_e,  c = sum_e E_e ce_e,  g_e = -penal x^_e^(penal-1) (1 - e_min) max(ce_e, 0)
 *                     4. dc_e = sum_j H_ej g_j d_j / Hs_j,  dv_e = sum_j H_ej d_j / Hs_j
 *                     5. n_bisect bisection steps on lambda in [0, 1e9]:
 *                        x_new = max(0, max(x - move, min(1, min(x + move, x sqrt(-dc / (dv lambda)))))),
 *                        mean(x^(x~(x_new))) > vf => l1 = lambda, else l2 = lambda: every step filters and projects the trial design
 *                        in LDS; the x_new of the last step is the result
 *                   x_new [B, nel*nel] = the design variables, x_phys_new [B, nel*nel] = x^(x~(x_new)) (must not alias x / x_new),
 *                   u_out, compliance = c, change = max |x_new - x|, pcg_iters, relres as pidm_simp_step.  An inactive sample is copied
 *                   through and its x_phys_new is x^(x~(x)) at the given beta.  filter must be 1 or 2, beta > 0, 0 < eta < 1.
 *   pidm_mech_fields: nodal conditioning fields of a solved state u_dofs [B, ndof] (fp32, as pidm_mech_solve writes it) with Young's
 *                   moduli rho [B, nel*nel]: per element, at its centre, the strain energy density 1/2 rho_e u_e^T k_e u_e / area
 *                   and the plane-stress von Mises stress sqrt(sx^2 - sx sy + sy^2 + 3 txy^2), sigma = rho_e C(nu) B(0,0) u_e, for
 *                   the regular mesh of unit squares with local nodes (bottom-left, bottom-right, top-right, top-left); every node
 *                   gets the mean of its 1-4 adjacent elements.  fields [B,2,nel+1,nel+1] (energy density, von Mises), fp32. */
size_t pidm_simp_ws_bytes(int nel, int B);
int pidm_simp_step(const double* x, const double* u, const float* bcs, const float* vf, const int32_t* active, const float* kloc,
                   int kloc_stride, const int32_t* elem_dofs, const int32_t* dof_elems, int nel, double penal, double e_min,
                   double rmin, double move, int n_bisect, int pcg_max_iter, double pcg_rtol, double* x_new, double* u_out,
                   double* compliance, double* change, int32_t* pcg_iters, double* relres, void* workspace, int B, void* stream);
int pidm_simp_step_filtered(const double* x, const double* u, const float* bcs, const float* vf, const int32_t* active,
                            const float* kloc, int kloc_stride, const int32_t* elem_dofs, const int32_t* dof_elems, int nel, double penal,
                            double e_min, double rmin, double move, int n_bisect, int pcg_max_iter, double pcg_rtol, int filter,
                            double beta, double eta, double* x_new, double* x_phys_new, double* u_out, double* compliance,
                            double* change, int32_t* pcg_iters, double* relres, void* workspace, int B, void* stream);
int pidm_mech_fields(const float* u_dofs, const float* rho, const float* kloc, int kloc_stride, const int32_t* elem_dofs, int nel,
                     double nu, float* fields, int B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * UNet engine                           replaces Unet3D.forward src/unet_model.py:542-623 + autograd
 * ------------------------------------------------------------------------------------------- */
typedef struct pidm_unet pidm_unet;
typedef struct pidm_unet_cfg {
  int dim;            /* base width (32 Darcy, 128 mechanics) */
  int channels;       /* input channels */
  int out_dim;        /* output channels */
  int n_levels;       /* len(dim_mults) */
  int dim_mults[8];
  int heads;          /* 8 */
  int dim_head;       /* 32 */
  int groups;         /* GroupNorm groups, 8 */
  int init_kernel;    /* 7 */
  int image_size;     /* P (square images) */
  int sigmoid_last_channel;
  int self_condition; /* 1: init_conv reads 2*channels inputs, cat(x_self_cond, x) (src/unet_model.py:428,564-566) */
  int padding_mode;   /* 0: zeros, 1: circular (Unet3D(padding_mode=...), src/unet_model.py:161-199,224-229,424,452-455).  Circular:
                       * every tap of init_conv, the 3x3 Block.proj, the 4x4/s2 Downsample and the transposed 4x4/s2 upsample that zero
                       * mode reads as 0 outside the image reads the pixel at the index wrapped modulo the extent - forward, input and
                       * weight gradients alike; emb_conv.2 of the conditioning branch stays zero-padded (:524).  The upsample
                       * parameters are then named ups.i.3.conv_transpose.{weight,bias} (CircularUpsample).  Every level needs an
                       * extent >= 2.  Fixed at pidm_unet_create; a zero-initialised struct gets zero padding. */
} pidm_unet_cfg;

int pidm_unet_create(const pidm_unet_cfg* cfg, pidm_unet** out);
void pidm_unet_destroy(pidm_unet* h);
/* canonical list of the parameter tensors forward() reads (state_dict names, 259 for the Darcy model) */
int pidm_unet_num_params(const pidm_unet* h);
const char* pidm_unet_param_name(const pidm_unet* h, int i);
size_t pidm_unet_param_numel(const pidm_unet* h, int i);
/* bytes of caller-provided device scratch needed for batch B (persistent region + per-call arena) */
size_t pidm_unet_workspace_bytes(const pidm_unet* h, int B, int training);
/* param_ptrs_host[i]: device pointer of parameter i in the reference's own layout
 * (Conv3d [Cout,Cin,1,k,k], ConvTranspose3d [Cin,Cout,1,k,k], Linear [out,in], ...).  grad_ptrs_host[i]:
 * where backward WRITES (not accumulates) d loss / d param i, same layout; may be NULL for inference. */
int pidm_unet_bind(pidm_unet* h, const void* const* param_ptrs_host, void* const* grad_ptrs_host);
/* x: [B,P*P,C] channels-last; t: int64 [B]; out: [B,out_dim,P,P] NCHW (reference output layout).
 * save_for_backward != 0 keeps activations in the workspace until pidm_unet_backward. */
int pidm_unet_forward(pidm_unet* h, const float* x_nhwc, const int64_t* t, float* out_nchw, int B,
                      int save_for_backward, int repack_weights, void* workspace, size_t workspace_bytes, void* stream);
/* Gradient-guidance conditioning branch (src/unet_model.py:521-528,571-587: x = combine_conv(cat(init_conv(x), emb_conv(cond)))).
 * Its 6 parameters (emb_conv.0/2, combine_conv; weight+bias) are the LAST pidm_unet_num_cond_params() entries of the
 * canonical list.  pidm_unet_enable_cond sizes the workspace for the branch (call it before pidm_unet_workspace_bytes);
 * pidm_unet_set_condition hands the (already classifier-free-masked) field [B,P*P,C] to the NEXT pidm_unet_forward only.
 * A backward whose forward had no conditioning input zero-fills the gradients of those 6 parameters. */
int pidm_unet_num_cond_params(const pidm_unet* h);
int pidm_unet_enable_cond(pidm_unet* h, int on);
int pidm_unet_set_condition(pidm_unet* h, const float* cond_nhwc);
/* grad_out: [B,out_dim,P,P] NCHW.  grad_x (may be NULL): [B,P*P,C].  Writes all bound grads. */
int pidm_unet_backward(pidm_unet* h, const float* grad_out_nchw, float* grad_x_nhwc, int B, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The input gradient alone (posterior guidance: the gradient of a potential of the x0 estimate with respect to x_t).  Same tape
 * contract as pidm_unet_backward (follows a save_for_backward forward of the same B, no conditioning input) and the same
 * input-gradient chain - same kernels, arguments and arena layout, so grad_x is bit-identical to pidm_unet_backward's - but no
 * convolution weight-gradient kernel, no time-MLP / FiLM backward, no gradient reduction, no side stream and no phase events.
 * Parameter-gradient by-products of the data-path kernels (GroupNorm / LayerNorm / attention-projection partials) stay in the
 * workspace; nothing is written through the gradient pointers of pidm_unet_bind, which may be NULL.  Replayed as a hipGraph of
 * its own from the third identical call on.  grad_x is required. */
int pidm_unet_backward_input(pidm_unet* h, const float* grad_out_nchw, float* grad_x_nhwc, int B, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Data-parallel overlap (no reference counterpart: the reference is single-process).  The deferred gradient
 * reduction of pidm_unet_backward runs in n_phases (1..3) launches - after the decoder half (ups.*, final_conv.*), after the
 * encoder half (downs.*, mid_*), at the end (everything else) - and records events[k] (hipEvent_t, may be NULL) on the
 * backward's stream after phase k, so the caller can start the collective over that phase's gradients while the rest of
 * backward is still running.  pidm_unet_grad_phase_range: canonical parameter index range [first, end) finalised by a phase;
 * the LAST phase additionally finalises every parameter outside the earlier phases' ranges. */
int pidm_unet_set_grad_events(pidm_unet* h, int n_phases, void* const* events);
int pidm_unet_grad_phase_range(const pidm_unet* h, int n_phases, int phase, int* first_param, int* end_param);

/* ---------------------------------------------------------------------------------------------
 * Unit-level kernel entry points (used by the parity tests; the engine calls the same launchers)
 * ------------------------------------------------------------------------------------------- */
typedef struct pidm_conv_desc {
  int B, Hi, Wi;        /* input  [B,Hi,Wi,C0(+C1)] channels-last */
  int C0, C1;           /* channels taken from src0 / src1 (concat elimination), C1 may be 0 */
  int ld0, ld1;         /* channel strides (floats per pixel) of src0 / src1 */
  int Cout;
  int KH, KW, stride, pad;
  int transposed;       /* 1: ConvTranspose 4x4 s2 p1 executed as 4 output-parity 2x2 convolutions */
  int out_nchw;         /* 1: write [B,Cout,Ho,Wo] instead of channels-last */
  int ldo;              /* channel stride of the output / residual (channels-last) */
  int pad_mode;         /* 0: zero padding; 1: circular - a tap outside the input reads the pixel at the index wrapped modulo the
                         * extent (Hi, Wi powers of two, pad <= extent); honoured by _forward, _forward_gn_partials, _dgrad, _wgrad
                         * and their workspace / packing queries.  For a transposed convolution the wrap is that of
                         * out[y] = sum_j x[j mod Hi] w[y + 1 - 2j] (the reference's CircularUpsample). */
} pidm_conv_desc;
size_t pidm_conv_packed_weight_floats(const pidm_conv_desc* d);
/* mode 0: forward pack from [Cout,Cin,KH,KW]; 1: dgrad pack (flipped+transposed) from the same tensor;
 * for transposed convs the source is [Cin,Cout,KH,KW]. */
int pidm_conv_pack_weights(const pidm_conv_desc* d, const float* w_ref, float* w_packed, int mode, void* stream);
int pidm_conv_forward(const pidm_conv_desc* d, const float* src0, const float* src1, const float* w_packed,
                      const float* bias, const float* residual, float* out, void* stream);
/* forward convolution feeding a GroupNorm (Block: proj -> norm, src/unet_model.py:227-241): besides `out`, the epilogue leaves
 * per-(image, chunk, group) sums and sums of squares of the output in partial[B][chunks][groups][2] (doubles; size it for H*W/32
 * chunks).  A chunk is a set of pixels of one image, the chunks of an image cover it once: 32 consecutive pixels behind the tile
 * kernels (H*W/32 chunks), a strip of 32 pixels x R rows behind the row-streaming kernel.  Returns the chunks per image
 * written, 0 when the shape has no statistics epilogue (then only `out` is written), < 0 on error. */
int pidm_conv_forward_gn_partials(const pidm_conv_desc* d, const float* src0, const float* src1, const float* w_packed,
                                  const float* bias, float* out, int groups, double* partial, void* stream);
/* One half of a ResnetBlock as the engine runs it (Block: proj -> norm -> FiLM -> SiLU, src/unet_model.py:227-241), 3x3 / stride 1:
 * a = conv(src) + bias, y = SiLU((GroupNorm(a) * gamma + beta) * (1 + scale) + shift) [+ res], stats[B][groups][2] = (mean, rstd);
 * scale | shift = ss[b][0..2 Cout) + ssb (ss NULL: none), res laid out like y (NULL: none).  Where a workgroup's tile holds whole
 * images (16 x 16 and 8 x 8 at engine batch sizes) the convolution finishes the GroupNorm itself: returns 1; else 0 (separate
 * GroupNorm launches), < 0 on error.  PIDM_NO_GN_FUSED=1: always separate.  ws: B*H*W/32*Cout*2 doubles + B*2*Cout floats. */
int pidm_conv_gn_forward(const pidm_conv_desc* d, const float* src0, const float* src1, const float* w_packed, const float* bias,
                         int groups, const float* gamma, const float* beta, const float* ss, const float* ssb, int ldss,
                         const float* res, float* a, float* y, float* stats, void* ws, void* stream);
/* ... and its backward: dy = input gradient of the convolution d (the block's NEXT convolution; weights packed with mode 1) from
 * g_c, dx = gradient wrt x of y = SiLU(FiLM(GroupNorm(x))) at dy (x, stats as the forward left them), dgb[B][2][C] = per-image
 * dgamma | dbeta rows, dss[B][ldss] = FiLM gradient rows (ss NULL: untouched).  Returns 1 when the convolution did all of it (dy is
 * then not written), 0 for separate launches, < 0 on error.  ws as above. */
int pidm_conv_dgrad_gn_backward(const pidm_conv_desc* d, const float* g_c, const float* w_packed_dgrad, const float* x,
                                const float* stats, int groups, const float* gamma, const float* beta, const float* ss,
                                const float* ssb, int ldss, float* dss, float* dgb, float* dy, float* dx, void* ws, void* stream);
/* adjoint wrt the input: dx[B,Hi,Wi,Cin] (+ residual) from dy[B,Ho,Wo,Cout]; weights packed with mode 1 */
size_t pidm_conv_dgrad_packed_weight_floats(const pidm_conv_desc* d);
int pidm_conv_dgrad(const pidm_conv_desc* d, const float* dy, int ld_dy, const float* w_packed_dgrad,
                    const float* residual, float* dx, int ld_dx, void* stream);
size_t pidm_conv_wgrad_ws(const pidm_conv_desc* d);
/* dW (reference layout) and dbias (may be NULL) from input x (src0/src1) and output-gradient dy */
int pidm_conv_wgrad(const pidm_conv_desc* d, const float* src0, const float* src1, const float* dy, int ld_dy,
                    float* dw_ref, float* dbias, void* workspace, void* stream);

/* Linear attention core of SpatialLinearAttention.forward (src/unet_model.py:281-299) between the to_qkv and to_out 1x1
 * convolutions: q.softmax(dim=-2) * scale, k.softmax(dim=-1), context = k v^T / N, out = context^T q.
 *   qkv  [B][N][3*heads*32] channels-last (q | k | v, head-major), N = h*w pixels;  out [B][N][heads*32]
 *   saved for the backward: kstat [B][heads*32][2], ctx [B][heads][32][32], qstat [B][N][heads][2]
 *   backward: d_out [B][N][heads*32] -> dqkv [B][N][3*heads*32]                                                     */
size_t pidm_linear_attention_ws(int B, int N, int heads);
int pidm_linear_attention_forward(const float* qkv, float* out, float* kstat, float* ctx, float* qstat, int B, int N,
                                  int heads, void* workspace, void* stream);
int pidm_linear_attention_backward(const float* qkv, const float* kstat, const float* qstat, const float* ctx,
                                   const float* d_out, float* dqkv, int B, int N, int heads, void* workspace, void* stream);
/* The same backward fused with the to_out 1x1 projection (src/unet_model.py:298): takes the gradient d_y [B][N][Cout] of the
 * projection's output and its weights w_out [Cout][heads*32] (reference layout), returns dqkv and the projection's weight
 * gradient dw_out [Cout][heads*32] without materialising d_out.  N % 128 == 0, Cout in {32, 64, 128}. */
/* forward counterpart: y [B][N][Cout] = to_out(attention(qkv)) + bias + residual (either may be NULL) without storing the
 * heads*32-channel attention output; workspace as pidm_linear_attention_ws. */
int pidm_linear_attention_out_forward(const float* qkv, const float* w_out, const float* bias, const float* residual, float* y,
                                      int Cout, float* kstat, float* ctx, float* qstat, int B, int N, int heads, void* workspace,
                                      void* stream);
size_t pidm_linear_attention_out_backward_ws(int B, int N, int heads, int Cout);
int pidm_linear_attention_out_backward(const float* qkv, const float* kstat, const float* qstat, const float* ctx,
                                       const float* d_y, int ld_dy, const float* w_out, int Cout, float* dqkv, float* dw_out,
                                       int B, int N, int heads, void* workspace, void* stream);

/* Linear attention WITHOUT a qkv tensor (csrc/k_attn_proj.hip)      replaces Residual(PreNorm(SpatialLinearAttention)) between the
 * LayerNorm and the residual add, src/unet_model.py:281-299 + :139-145, and its autograd.
 * xn [B,N,C] = LayerNorm output (channels-last); w_qkv [3*heads*32, C] and w_out [C, heads*32] in the reference layouts
 * (to_qkv.weight, to_out.weight); bias [C]; resid [B,N,C] = the block input x; y [B,N,C] = to_out(attention) + bias + x.
 * The forward keeps `saved` (pidm_lap_saved_floats floats: k-softmax statistics, M, ctx, P per image and head) and
 * qstat [B,N,heads,2] (q-softmax max, 1/sum) for the backward.  The backward takes dY = d loss / d y and WRITES d_xn (without
 * the residual's own dY -> dx share), d_w_qkv, d_w_out.  C in {32, 64}, N % 32 == 0, heads <= 8.  workspace: pidm_lap_ws bytes. */
size_t pidm_lap_ws(int B, int N, int heads, int C);
size_t pidm_lap_saved_floats(int B, int heads, int C);
int pidm_lap_forward(const float* xn, const float* w_qkv, const float* w_out, const float* bias, const float* resid, float* y,
                     float* saved, float* qstat, int C, int B, int N, int heads, void* workspace, void* stream);
int pidm_lap_backward(const float* xn, const float* dy, const float* w_qkv, const float* w_out, const float* saved,
                      const float* qstat, float* d_xn, float* d_w_qkv, float* d_w_out, int C, int B, int N, int heads,
                      void* workspace, void* stream);

/* measurement aid (tools/conv_trace.py): cycle stamps of the streaming 3x3 convolution kernel, written when PIDM_STREAM_TRACE is set */
int pidm_debug_stream_trace(unsigned long long* out256);
/* measurement aid (bench.py roofline.clock_probe): stamps of the last conv3x3_rs_kernel launch made with PIDM_RS_TRACE set -
 * out4 = {shader-clock counter, 100 MHz real-time counter} before and {.., ..} after the row loop of workgroup 0 / wave 0 */
int pidm_debug_conv_rs_trace(unsigned long long* out4);
/* cycle stamps of lap_bwd_kernel (PIDM_LAP_TRACE=1; tools/lap_trace.py): [wave slot < 2][tile round < 8][16] */
int pidm_debug_lap_trace(unsigned long long* out256);
/* test aid: host-to-device uploads of the deferred-reduction descriptor table since the library was loaded (a second identical
 * backward pass must not upload anything: the table is compared with what the device already holds) */
long long pidm_debug_reduce_table_uploads(void);
/* launch accounting since the library was loaded: out4 = {kernels enqueued launch by launch, hipGraphLaunch calls, kernels inside
 * the launched graphs, stream captures}.  pidm_unet_forward / pidm_unet_backward replay a captured hipGraph from the third call
 * with the same arguments on (PIDM_GRAPH=0: always launch by launch). */
int pidm_debug_launch_counts(long long* out4);
/* ---- data-parallel gradient exchange ----------------------------------------------------------------------
 * No reference counterpart: /root/reference/main.py:157-166 is single-device; north_star shards the batch over the GPUs of a node
 * and averages the gradients with an RCCL all-reduce over xGMI.  One communicator per process (= per GPU).  RCCL is bound with
 * dlopen at first use.  The reference-side binding: parallel.py (`PIDM_DP_NATIVE=1`) or any host with a way to hand rank 0's 128-byte
 * id to the other ranks.
 *   pidm_comm_available  every rank: 0 when RCCL could be bound, -1 + pidm_last_error() otherwise; starts no bootstrap thread
 *   pidm_comm_unique_id  rank 0: 128 opaque bytes to be sent to every rank (ncclGetUniqueId)
 *   pidm_comm_init       every rank, with the same id; uses the calling thread's current HIP device (ncclCommInitRank)
 *   pidm_allreduce_f32   in place on `buf[0..count)`, enqueued on `stream`; average != 0: mean over ranks, else sum
 *   pidm_comm_destroy    */
int pidm_comm_available(void);
int pidm_comm_unique_id(void* out128);
int pidm_comm_init(int rank, int world, const void* unique_id128, void** comm);
int pidm_allreduce_f32(void* comm, float* buf, size_t count, int average, void* stream);
int pidm_comm_destroy(void* comm);

/* The library reads each PIDM_* tuning variable from the environment once per process (the first time a launcher asks for it).
 * A process that changes one afterwards - the unit tests, A/B legs of bench.py - calls this to drop the snapshot; the next launch
 * re-reads.  No reference counterpart (the knobs select between kernels that compute the same result). */
int pidm_reload_knobs(void);

#ifdef __cplusplus
}
#endif
#endif /* PIDM_H */
