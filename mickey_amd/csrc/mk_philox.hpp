// mickey_amd -- Philox4x32-10 and the Exp(1) draws of the exponential races: the outer sampler (mk_sampler.hip), the
// hypothesis draws of mk_ransac_hypotheses and the training-time RANSAC (mk_solver.hip) key their streams through these.
// Like mk_procrustes.hpp this header carries NO floating-point contraction pragma of its own: it is included after the
// including file's `#pragma clang fp contract(off)` and compiles in that file's mode.
#pragma once
#include "mk_common.hpp"

namespace mk {

struct U4 { unsigned x, y, z, w; };
__device__ __forceinline__ U4 philox4x32(unsigned k0, unsigned k1, U4 c) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    // one 32x32 -> 64 product per multiplier (the compiler can then use v_mad_u64_u32) instead of separate
    // v_mul_hi_u32 + v_mul_lo_u32: integer multiplies are quarter rate and were 37 of the ~105 instructions of the key loop
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * (unsigned long long)c.x;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * (unsigned long long)c.z;
    const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0;
    const unsigned hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// Exp(1) draw from 32 random bits: u in (0,1) on a 2^-24 grid, e = -log(u) > 0
__device__ __forceinline__ float exp1(unsigned r) { return -logf(((float)(r >> 8) + 0.5f) * 5.9604644775390625e-8f); }
// Race key p / e for the on-device (Philox) path: only the ORDER of the keys matters, so hardware log2 / rcp
// (1 ulp-class) replace libm logf and the IEEE divide (~35 -> ~10 instructions per key).  The injected-noise path
// keeps the exact p / e so that it stays bit-comparable with torch.
__device__ __forceinline__ float race_key(float p, unsigned r) {
  const float u = ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-8f;
  const float e = -0.69314718055994531f * __builtin_amdgcn_logf(u);
  return p * __builtin_amdgcn_rcpf(e);
}

// Optional device-resident part of the Philox stream offset (a captured hipGraph re-reads it at every replay)
__device__ __forceinline__ void add_device_offset(unsigned& off_lo, unsigned& off_hi, const unsigned long long* offp) {
  if (!offp) return;
  const unsigned long long o = (((unsigned long long)off_hi << 32) | off_lo) + *offp;
  off_lo = (unsigned)o;
  off_hi = (unsigned)(o >> 32);
}

}  // namespace mk
