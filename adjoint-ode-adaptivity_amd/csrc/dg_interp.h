// dg_interp.h — the fine-grid solution of the ODE-ensemble sweeps (dg_fd.hip, dg_resnet.hip):
// the np.interp of the coarse solution, evaluated on the fly with numpy's arithmetic
// (host-computed interval codes, no FMA contraction) instead of being stored.
#pragma once
#include "dg_common.h"

namespace dgk {

// np.interp(t_fine[i], t_coarse, u) with numpy's case split (numpy/core/src/multiarray/
// compiled_base.c arr_interp): code >= 0 -> slope*(x - xp[j]) + fp[j] in interval j,
// code < 0 -> the coarse node -(code+1) exactly.
__device__ __forceinline__ double fine_u(int32_t code, double x, const double* __restrict__ tc,
                                         const double* __restrict__ U, int64_t n_ics,
                                         int64_t ic) {
  if (code < 0) return U[int64_t(-(code + 1)) * n_ics + ic];
  const double u0 = U[int64_t(code) * n_ics + ic], u1 = U[int64_t(code + 1) * n_ics + ic];
  const double slope = __ddiv_rn(__dsub_rn(u1, u0), __dsub_rn(tc[code + 1], tc[code]));
  return __dadd_rn(__dmul_rn(slope, __dsub_rn(x, tc[code])), u0);
}

}  // namespace dgk
