// Shared between k_mech.hip and k_guidance_mech.hip: the mesh tables of the matrix-free mechanics kernels, torch's bilinear source
// index and the mesh argument check.
#pragma once
#include "pidm_launch.h"

namespace pidm {

struct MechMesh {
  const int* elem_dofs;   // [E][8]
  const int* dof_elems;   // [ndof][4][2] = (element, local index) or (-1, -1)
  const float* kloc;      // [E][8][8] or [1][8][8] when kloc_stride == 0
  int kloc_stride;        // 0 (uniform mesh) or 64
  int E, ndof, nel, nn;   // nel = 64 elements per side, nn = 65 nodes per side
};

// source index / weight of torch's bilinear, align_corners=False, for output coordinate o
__device__ __forceinline__ void bil_src(int o, int n_in, int n_out, int* i0, int* i1, float* lam) {
  float src = ((float)o + 0.5f) * ((float)n_in / (float)n_out) - 0.5f;
  if (src < 0.f) src = 0.f;
  int a = (int)src;
  if (a > n_in - 1) a = n_in - 1;
  *i0 = a;
  *i1 = (a < n_in - 1) ? a + 1 : a;
  *lam = src - (float)a;
}

static inline int mech_args(int nel, int E, int ndof, const void* a, const void* b2, const void* c) {
  if (!a || !b2 || !c) return fail("mech: null mesh table");
  if (E != nel * nel || ndof != 2 * (nel + 1) * (nel + 1)) return fail("mech: mesh must be nel x nel quads with all dofs free");
  return 0;
}

}  // namespace pidm
