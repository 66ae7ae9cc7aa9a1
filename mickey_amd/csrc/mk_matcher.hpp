// mickey_amd -- device helpers of the dual-softmax matcher shared by its forward (mk_matcher.hip) and its backward
// (mk_matcher_bwd.hip): the correlation tile on either path, the log2-domain (max, sum) merge, the XCD-aware grid decode.
// Moved here unchanged from mk_matcher.hip (its kernels compile to the same code: build/resource_usage.json).
#pragma once
#include "mk_common.hpp"

namespace mk {
namespace ds {

constexpr int NCHUNK = 4;   // column chunks of pass 1 (exact path)
constexpr int CMAX = 128;   // descriptor channels held in LDS

// ---- dual softmax: register-resident correlation ---------------------------------------------------------------
// v_mfma_f32_32x32x2_f32 takes ONE float per lane per operand (lane l: row/column l & 31, k = 2 kk + (l >> 5)), so a
// wave keeps the descriptors of its 32 rows in 64 VGPRs for its whole life and streams 32-column tiles of the other
// image straight from L2 (descriptors are ~1 MB per image): 64 coalesced 4-byte loads + 64 MFMAs per tile, no LDS, no
// barriers.  (The previous version staged 64 KiB through LDS with scalar loads per 64x64 tile and ran at ~10 % of the
// fp32 matrix rate.)  Everything is kept in the log2 domain: v2 = S / T * log2(e), exp2 is one v_exp_f32.
constexpr int RT = 32;       // rows per wave, columns per streamed tile

__device__ __forceinline__ void lse2_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  s = s * __builtin_amdgcn_exp2f(m - M) + s2 * __builtin_amdgcn_exp2f(m2 - M);
  m = M;
}

// A-side operand: this lane's 64 k-values of row i0 + (lane & 31); rows >= n are zero
template <bool FULLC>
__device__ __forceinline__ void load_operand(float (&a)[CMAX / 2], const float* __restrict__ d, int C, int n, int i, int hi) {
  const bool ok = i < n;
  const float* pa = d + (long long)hi * n + (ok ? i : n - 1);
#pragma unroll
  for (int kk = 0; kk < CMAX / 2; ++kk) {
    if (!FULLC && kk >= (C >> 1)) {
      a[kk] = 0.f;
    } else {
      const float v = pa[(long long)kk * 2 * n];
      a[kk] = ok ? v : 0.f;
    }
  }
}

// XCD-aware decode of a 1-D grid into (bx, by, unit): workgroups are dealt round-robin to the 8 XCDs, so the linear id
// is re-read as (xcd, slot) and ALL gx*gy workgroups of a unit (an image pair [x side]) land on one XCD, whose 4-MiB L2
// then holds that unit's ~2 MB of descriptors.  (Dealt naively, every XCD serves 8 pairs at a time, thrashes its L2 and
// pulls 1.9 GB of 128-byte pieces from memory per pass: measured 1.9 ms instead of 0.4.)  The grid is padded to a
// multiple of 8 units; returns false for padding.
// Y_FASTEST: consecutive workgroups of a unit walk the y index (the column chunks of the split passes) first: the workgroups
// in flight at one time then cover WHOLE rows of the output between them (kernels that write [rows, n1] matrices tile by tile:
// a wave's 256-byte row pieces meet their neighbours' in the same DRAM pages while those are open).
template <bool Y_FASTEST = false>
__device__ __forceinline__ bool decode_unit_grid(int gx, int gy, int nunits, int& bx, int& by, int& unit) {
  const int L = blockIdx.x, per = gx * gy;
  int within;
  if (nunits < 8) {   // too few units to give every XCD one: spread each unit over the whole chip instead
    unit = L / per;
    within = L - unit * per;
  } else {
    const int xcd = L & 7, slot = L >> 3;
    unit = (slot / per) * 8 + xcd;
    within = slot - (slot / per) * per;
  }
  if (Y_FASTEST) {
    by = within % gy;
    bx = within / gy;
  } else {
    bx = within % gx;
    by = within / gx;
  }
  return unit < nunits;
}

// Scheduling directive for the tile body (one basic block): all 64 operand loads first, then the 64 MFMAs.  Left alone,
// the scheduler keeps ONE operand register and emits load -> s_waitcnt vmcnt(0) -> MFMA, i.e. 64 serial memory round
// trips per tile (measured 32 us per tile instead of ~3).
#define MK_LOADS_THEN_MFMAS()                                  \
  do {                                                         \
    __builtin_amdgcn_sched_group_barrier(0x020, CMAX / 2, 0);  \
    __builtin_amdgcn_sched_group_barrier(0x002, CMAX / 2, 0);  \
    __builtin_amdgcn_sched_group_barrier(0x008, CMAX / 2, 0);  \
  } while (0)

template <bool FULLC>
__device__ __forceinline__ f32x16 corr_regs(const float (&a)[CMAX / 2], const float (&bq)[CMAX / 2], int C) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int kk = 0; kk < CMAX / 2; ++kk) {
    if (FULLC || kk < (C >> 1)) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], bq[kk], acc, 0, 0, 0);
  }
  return acc;
}

// ---- split-fp16 correlation (see mk_matcher.hip) -----------------------------------------------------------------------
constexpr int SP_KS = 8;        // K steps of 16 channels: C = 128
constexpr int SP_BLK_U4 = SP_KS * 2 * 64;   // uint4 per block of 32 keypoints (16 KiB)
constexpr int NCHUNK_S = 8;     // column chunks of the split passes (FIXED: the summation order of a row does not depend on B)
constexpr float SP_SCALE = 1024.0f;

struct SplitOperand {
  uint4 h[SP_KS], l[SP_KS];
  __device__ __forceinline__ void load(const uint4* __restrict__ blk, int lane) {
#pragma unroll
    for (int st = 0; st < SP_KS; ++st) {
      h[st] = blk[(st * 2) * 64 + lane];
      l[st] = blk[(st * 2 + 1) * 64 + lane];
    }
  }
};

// S' = 2^20 x (32 rows of a) . (32 columns of b): cross terms first, the large term last
__device__ __forceinline__ f32x16 corr_split(const SplitOperand& a, const SplitOperand& b) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int st = 0; st < SP_KS; ++st)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a.l[st]), __builtin_bit_cast(f16x8, b.h[st]), acc, 0, 0, 0);
#pragma unroll
  for (int st = 0; st < SP_KS; ++st)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a.h[st]), __builtin_bit_cast(f16x8, b.l[st]), acc, 0, 0, 0);
#pragma unroll
  for (int st = 0; st < SP_KS; ++st)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a.h[st]), __builtin_bit_cast(f16x8, b.h[st]), acc, 0, 0, 0);
  return acc;
}

// ---- host side: pieces of the forward the training entry points reuse (mk_matcher.hip) --------------------------------
// fp32 [nimg, 128, n] -> split planes [nimg, nblk, 8, 2, 64] x 16 B (dsc_split_kernel)
int split_planes(const float* dsc, uint4* planes, int n, int nblk, int nimg, hipStream_t st);
// The forward of mk_dual_softmax (split = 0) / mk_dual_softmax_split (split = 1) with the same kernels, except the merge of
// the partials: lse_merge_dev (dustbin read from a device pointer, NULL = none) writes lse [B, 2, max(n0, n1)] (log2
// domain), which pass 2 then reads.  work: the same size as the matching *_work_floats.
int dual_softmax_train_fwd(int split, const float* dsc0, const float* dsc1, const float* scr0, const float* scr1,
                           float inv_temperature, const float* dustbin, float* scores, float* kp_scores, float* final_scores,
                           float* lse, float* work, int B, int C, int n0, int n1, hipStream_t st);
// lse_final_kernel's merge with the dustbin term read on the device (mk_matcher_bwd.hip)
int lse_merge_dev(const float* partr, const float* partc, float* lse2, const float* dustbin, int B, int n0, int n1, int nrb,
                  int nchunk, hipStream_t st);

}  // namespace ds
}  // namespace mk
