// mickey_amd -- the eye grid of the VCRE (reference lib/benchmarks/reprojection.py:32-56): 7 x 4 x 7 virtual points in front of the
// camera, 0.3 m apart.  Shared by the training loss (mk_train_tail.hip) and the validation metrics (mk_metrics.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace mk {

constexpr int kEyePoints = 196;

// point p of the grid in the reference's order (np.meshgrid(x[7], y[4], z[7]) flattened: p = (j * 7 + i) * 7 + k)
__device__ __forceinline__ void eye_point(int p, float* e) {
  const int k = p % 7, i = (p / 7) % 7, j = p / 49;
  e[0] = ((float)i - 3.0f) * 0.3f;
  e[1] = ((float)j - 1.5f) * 0.3f;
  e[2] = (float)k * 0.3f + 1.8f;
}

}  // namespace mk
