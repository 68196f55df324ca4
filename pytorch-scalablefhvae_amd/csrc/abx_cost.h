// abx_cost.h -- the frame cost of include/fhvae_abx.h, one definition for abx.hip and qbe.hip (include/fhvae_qbe.h takes the
// cost of that header as it stands).  Both files compile with -ffp-contract=off and correctly rounded f32 division and sqrt;
// nothing here is fused.
#pragma once
#include <math.h>

#include "../../include/fhvae_abx.h"

namespace fh {

// the float64 cost of two rows from their float64 dot and norms: the cosine clamped to [-1, 1], 0 against a zero row, then
// acos / pi or 1 - cos.  The caller rounds it once to f32
__device__ __forceinline__ double abx_frame_cost(double dot, double na, double nb, int metric) {
  double cs = 0.0;
  if (na != 0.0 && nb != 0.0) {
    cs = dot / (na * nb);
    cs = cs > 1.0 ? 1.0 : (cs < -1.0 ? -1.0 : cs);
  }
  return metric == FHVAE_ABX_ANGULAR ? acos(cs) / M_PI : 1.0 - cs;
}

}  // namespace fh
