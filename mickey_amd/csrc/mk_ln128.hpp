// mickey_amd -- LayerNorm over 128 features held as MFMA accumulators: shared by gemm_ln128_kernel (mk_heads.hip) and
// linattn_apply_fused_kernel (mk_linattn.hip), which must normalise with the same sums in the same order.
#pragma once
#include "mk_common.hpp"

namespace mk {

// LayerNorm over a row's 128 features held as MFMA accumulators (this lane's 32, the rest in lanes ^16, ^32): the row is centred
// in place, 1 / std is returned.  Shared by every kernel that normalises in the accumulators (same sums in the same order).
__device__ __forceinline__ float ln128_centre(f32x4 (&acc)[8], const float eps) {
  float sm = 0.f;
#pragma unroll
  for (int f = 0; f < 8; ++f) sm += (acc[f][0] + acc[f][1]) + (acc[f][2] + acc[f][3]);
  sm += __shfl_xor(sm, 16, 64);
  sm += __shfl_xor(sm, 32, 64);
  const float mean = sm * (1.0f / 128.0f);
  float qs = 0.f;
#pragma unroll
  for (int f = 0; f < 8; ++f) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[f][e] -= mean;
      qs += acc[f][e] * acc[f][e];
    }
  }
  qs += __shfl_xor(qs, 16, 64);
  qs += __shfl_xor(qs, 32, 64);
  return 1.0f / sqrtf(qs * (1.0f / 128.0f) + eps);
}
__device__ __forceinline__ f32x4 ln128_affine(const f32x4 c, const float rstd, const f32x4 ww, const f32x4 bb) {
  f32x4 y;
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] = c[e] * rstd * ww[e] + bb[e];
  return y;
}

}  // namespace mk
