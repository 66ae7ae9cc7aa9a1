// mickey_amd -- the validation tail of the trainer on gfx950: the per-pair pose / VCRE metrics and the epoch summary.
// reference lib/utils/metrics.py:12-53 (pose_error_torch), :83-125 (vcre_torch: ~60 ATen launches per batch, a torch.linalg.inv of
// 4x4 matrices, an upload of the eye grid per call), lib/models/MicKey/model.py:205-280 (on_validation_epoch_end: every record to the
// host, numpy precision_recall of lib/benchmarks/utils.py:138-188 three times).
//
//   mk_pose_metrics   one wave per pair.  fp64 arithmetic from the fp32 inputs, every result rounded ONCE to fp32; the 196 eye-grid
//                     points (mk_eye_grid.hpp) spread over the lanes, the wave's sum by the xor butterfly (a fixed order).  The
//                     residual pose is inv(cam2w_gt) cam2w_est in closed form: Rgt^T (R e + t - tgt).  Clips keep a NaN a NaN, as
//                     torch.clip does.  Writes one 8-float record per pair, straight into the epoch's record table.
//   mk_pose_summary   two launches, no atomics, no sort.  The average precision of precision_recall is
//                         AP = 1 / (N + failures) * sum_i cumTP_i / cumN_i,
//                     cumN_i = #{j : c_j >= c_i}, cumTP_i = #{j : c_j >= c_i and tp_j}: the reference sorts by confidence, takes one
//                     (precision, recall) point per group of tied confidences and weights the group's precision by its recall step,
//                     count / (N + failures); every member i of a group sees the group's cumTP / cumN, so the sum over records is
//                     the sum over groups.  Ties are exact by construction.  Launch 1: a thread owns record i, all records stream
//                     through LDS in tiles of kTile, the counts are integers, the quotient fp64; per-workgroup fp64 partials of the
//                     three AP sums, the four metric columns, the three accept counts, the non-finite confidences and the loss rows,
//                     added in lane / wave order.  Launch 2: one workgroup adds the partials in workgroup order.  Quadratic in N:
//                     N <= 2^18 (6.9e10 compares, milliseconds).
#include <math.h>

#include "mk_common.hpp"
#include "mk_eye_grid.hpp"

namespace {
using namespace mk;

constexpr int kTile = 256;          // records of an LDS tile = threads of a workgroup of launch 1 (mk_pose_summary_tile)
constexpr int kCols = 16;           // doubles of a partial row / of the final row
constexpr int kMaxRecords = 1 << 18;
constexpr double kDeg = 57.29577951308232087679815481410517;   // 180 / pi

// torch.clip / torch.minimum / torch.maximum semantics: a NaN comes out as a NaN (fmin / fmax would drop it)
__device__ __forceinline__ double clip_nan(double v, double lo, double hi) { return v != v ? v : fmin(fmax(v, lo), hi); }
__device__ __forceinline__ double min_nan(double a, double b) { return (a != a || b != b) ? a + b : fmin(a, b); }
__device__ __forceinline__ double max_nan(double a, double b) { return (a != a || b != b) ? a + b : fmax(a, b); }

__device__ __forceinline__ void proj(const double* K, const double* P, double* uv) {
  double q[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = K[a * 3] * P[0] + K[a * 3 + 1] * P[1] + K[a * 3 + 2] * P[2];
  const double z = q[2] + 1e-16;
  uv[0] = q[0] / z;
  uv[1] = q[1] / z;
}

__global__ __launch_bounds__(64) void pose_metrics_kernel(const float* __restrict__ R, const float* __restrict__ t,
                                                          const float* __restrict__ Tgt, const float* __restrict__ K,
                                                          const float* __restrict__ conf, float W, float H,
                                                          float* __restrict__ records, long long row0, int B) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  double Rm[9], tv[3], Rg[9], tg[3], Km[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    Rm[i] = (double)R[(long long)b * 9 + i];
    Km[i] = (double)K[(long long)b * 9 + i];
    Rg[i] = (double)Tgt[(long long)b * 16 + (i / 3) * 4 + (i % 3)];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    tv[i] = (double)t[(long long)b * 3 + i];
    tg[i] = (double)Tgt[(long long)b * 16 + i * 4 + 3];
  }
  // VCRE (metrics.py:83-125)
  double acc = 0.0;
  for (int p = lane; p < kEyePoints; p += 64) {
    float ef[3];
    eye_point(p, ef);
    const double e[3] = {(double)ef[0], (double)ef[1], (double)ef[2]};
    double uvg[2], uv[2], mv[3], rs[3];
    proj(Km, e, uvg);
#pragma unroll
    for (int a = 0; a < 3; ++a) mv[a] = Rm[a * 3] * e[0] + Rm[a * 3 + 1] * e[1] + Rm[a * 3 + 2] * e[2] + tv[a] - tg[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) rs[a] = Rg[a] * mv[0] + Rg[3 + a] * mv[1] + Rg[6 + a] * mv[2];   // Rgt^T (R e + t - tgt)
    proj(Km, rs, uv);
    const double du = clip_nan(uvg[0], 0.0, (double)W) - clip_nan(uv[0], 0.0, (double)W);
    const double dv = clip_nan(uvg[1], 0.0, (double)H) - clip_nan(uv[1], 0.0, (double)H);
    acc += sqrt(du * du + dv * dv + 1e-6);
  }
  const double vcre = wave_sum_d(acc) / (double)kEyePoints;
  if (lane != 0) return;
  // pose errors (metrics.py:12-53)
  const double st = sqrt(tv[0] * tv[0] + tv[1] * tv[1] + tv[2] * tv[2]);
  const double sg = sqrt(tg[0] * tg[0] + tg[1] * tg[1] + tg[2] * tg[2]);
  const double cos_t = clip_nan((tv[0] * tg[0] + tv[1] * tg[1] + tv[2] * tg[2]) / (st * sg + 1e-9), -1.0, 1.0);
  const double ang = acos(cos_t) * kDeg;
  const double d[3] = {tv[0] - tg[0], tv[1] - tg[1], tv[2] - tg[2]};
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) tr += Rm[i] * Rg[i];   // trace(R^T Rgt)
  const double cos_r = clip_nan((tr - 1.0) * 0.5, -1.0, 1.0);
  float* rec = records + (row0 + b) * 8;
  const f32x4 lo = {(float)min_nan(ang, 180.0 - ang), (float)(st / sg), (float)max_nan(st / sg, sg / st),
                    (float)sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])};
  const f32x4 hi = {(float)(acos(cos_r) * kDeg), (float)vcre, conf ? conf[b] : 0.0f, 0.0f};
  *(f32x4*)rec = lo;
  *(f32x4*)(rec + 4) = hi;
}

// the sum over the workgroup's WAVES waves, in a fixed order: the butterfly of each wave, then the waves in wave order
template <int WAVES>
__device__ __forceinline__ double block_sum(double s, double* red) {
  s = wave_sum_d(s);
  __syncthreads();   // (the previous use of red is over)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) r += red[w];
  return r;
}

struct Thresholds { float t, R, t2, R2, px; };

// what the ranking needs of a record: its confidence (not finite: -inf, ranked last) and its three acceptance bits
__device__ __forceinline__ float rank_key(float c) { return (c - c == 0.0f) ? c : -INFINITY; }
__device__ __forceinline__ unsigned accept_bits(float t_euc, float R_err, float vcre, const Thresholds& th) {
  return (unsigned)(t_euc < th.t && R_err < th.R) | ((unsigned)(t_euc < th.t2 && R_err < th.R2) << 1) | ((unsigned)(vcre < th.px) << 2);
}

// ---- launch 1: workgroup k owns records k * kTile .. ; partial row k of `work` ------------------------------------------------------
// columns: 0..2 sum_i cumTP_i / cumN_i of the three tests | 3..6 sums of t_err_ang, t_err_euc, R_err, vcre | 7..9 accepted records |
// 10 records with a non-finite confidence | 11..13 sums of the loss rows s = k * kTile + lane, + gridDim * kTile, ... | 14, 15 zero
__global__ __launch_bounds__(kTile) void pose_summary_rank_kernel(const float* __restrict__ records, int N,
                                                                  const float* __restrict__ losses, int S, Thresholds th,
                                                                  double* __restrict__ work) {
  __shared__ float s_key[kTile];
  __shared__ unsigned s_pack[kTile], s_tp2[kTile];   // pack: 1 | tp0 << 10 | tp1 << 20 (a tile adds at most kTile = 2^8 to a field)
  __shared__ double red[kTile / 64];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kTile + tid;
  const bool have = i < N;
  float ci = 0.f;
  double col[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) col[c] = 0.0;
  if (have) {
    const f32x4 lo = *(const f32x4*)(records + (long long)i * 8), hi = *(const f32x4*)(records + (long long)i * 8 + 4);
    ci = rank_key(hi[2]);
    const unsigned f = accept_bits(lo[3], hi[0], hi[1], th);
    col[3] = (double)lo[0];
    col[4] = (double)lo[3];
    col[5] = (double)hi[0];
    col[6] = (double)hi[1];
    col[7] = (double)(f & 1);
    col[8] = (double)((f >> 1) & 1);
    col[9] = (double)((f >> 2) & 1);
    col[10] = (hi[2] - hi[2] == 0.0f) ? 0.0 : 1.0;
  }
  int cum_n = 0, cum_tp0 = 0, cum_tp1 = 0, cum_tp2 = 0;
  for (int j0 = 0; j0 < N; j0 += kTile) {
    __syncthreads();   // (the previous tile has been read)
    const int j = j0 + tid;
    if (j < N) {
      const f32x4 lo = *(const f32x4*)(records + (long long)j * 8), hi = *(const f32x4*)(records + (long long)j * 8 + 4);
      const unsigned f = accept_bits(lo[3], hi[0], hi[1], th);
      s_key[tid] = rank_key(hi[2]);
      s_pack[tid] = 1u | ((f & 1u) << 10) | (((f >> 1) & 1u) << 20);
      s_tp2[tid] = (f >> 2) & 1u;
    }
    __syncthreads();
    const int cnt = N - j0 < kTile ? N - j0 : kTile;
    unsigned pack = 0, tp2 = 0;
    for (int k = 0; k < cnt; ++k) {
      const bool ge = s_key[k] >= ci;
      pack += ge ? s_pack[k] : 0u;
      tp2 += ge ? s_tp2[k] : 0u;
    }
    cum_n += (int)(pack & 1023u);
    cum_tp0 += (int)((pack >> 10) & 1023u);
    cum_tp1 += (int)(pack >> 20);
    cum_tp2 += (int)tp2;
  }
  if (have) {   // cum_n >= 1: record i counts itself
    col[0] = (double)cum_tp0 / (double)cum_n;
    col[1] = (double)cum_tp1 / (double)cum_n;
    col[2] = (double)cum_tp2 / (double)cum_n;
  }
  if (losses) {
    for (long long s = (long long)blockIdx.x * kTile + tid; s < S; s += (long long)gridDim.x * kTile) {
#pragma unroll
      for (int c = 0; c < 3; ++c) col[11 + c] += (double)losses[s * 3 + c];
    }
  }
#pragma unroll
  for (int c = 0; c < kCols; ++c) {
    const double s = c < 14 ? block_sum<kTile / 64>(col[c], red) : 0.0;
    if (tid == 0) work[(long long)blockIdx.x * kCols + c] = s;
  }
}

// ---- launch 2 (one workgroup): the partial rows added in workgroup order -- thread t adds its run of consecutive rows, then the
// workgroup's fixed-order sum.  The final row goes to work[nblk * kCols ..] in fp64 and to out in fp32. -------------------------------
__global__ __launch_bounds__(kTile) void pose_summary_reduce_kernel(double* __restrict__ work, int nblk, int N, int failures, int S,
                                                                    int have_losses, float* __restrict__ out) {
  __shared__ double red[kTile / 64];
  __shared__ double tot[kCols];
  const int tid = threadIdx.x;
  const int per = (nblk + kTile - 1) / kTile;
  const int k0 = tid * per < nblk ? tid * per : nblk;
  const int k1 = k0 + per < nblk ? k0 + per : nblk;
  for (int c = 0; c < 14; ++c) {
    double s = 0.0;
    for (int k = k0; k < k1; ++k) s += work[(long long)k * kCols + c];
    s = block_sum<kTile / 64>(s, red);
    if (tid == 0) tot[c] = s;
  }
  __syncthreads();
  if (tid >= kCols) return;
  const double n = (double)N, all = (double)N + (double)failures;
  double v = 0.0;
  switch (tid) {
    case 0: v = n; break;
    case 1: v = tot[10]; break;
    case 2: case 3: case 4: case 5: v = tot[3 + (tid - 2)] / n; break;                 // means of t_err_ang, t_err_euc, R_err, vcre
    case 6: case 8: case 10: v = tot[7 + (tid - 6) / 2] / all; break;                  // precisions
    case 7: case 9: case 11: v = tot[(tid - 7) / 2] / all; break;                      // average precisions
    case 12: case 13: case 14: v = (have_losses && S > 0) ? tot[11 + (tid - 12)] / (double)S : 0.0; break;
    default: break;
  }
  work[(long long)nblk * kCols + tid] = v;
  out[tid] = (float)v;
}

}  // namespace

extern "C" {

int mk_pose_metrics(const float* R, const float* t, const float* T_gt, const float* K, const float* conf, float W, float H,
                    float* records, long long row0, int B, long long capacity, mk_stream_t stream) {
  MK_CHECK_ARG(R && t && T_gt && K && records, "mk_pose_metrics: R, t, T_gt, K and records must not be NULL");
  MK_CHECK_ARG(((uintptr_t)records & 15) == 0, "mk_pose_metrics: records must be 16-byte aligned");
  MK_CHECK_ARG(B >= 1, "mk_pose_metrics: need B >= 1 (got %d)", B);
  MK_CHECK_ARG(row0 >= 0, "mk_pose_metrics: need row0 >= 0 (got %lld)", row0);
  MK_CHECK_ARG(capacity >= B && row0 <= capacity - B, "mk_pose_metrics: rows [%lld, %lld + %d) do not fit into %lld records", row0,
               row0, B, capacity);
  hipLaunchKernelGGL(pose_metrics_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, R, t, T_gt, K, conf, W, H, records, row0, B);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_pose_summary_tile(void) { return kTile; }

long long mk_pose_summary_work_doubles(int N) { return N > 0 ? ((long long)((N + kTile - 1) / kTile) + 1) * kCols : 0; }

int mk_pose_summary(const float* records, int N, int failures, float th_t, float th_R, float th_t2, float th_R2, float th_px,
                    const float* losses, int S, float* out, double* work, mk_stream_t stream) {
  MK_CHECK_ARG(records && ((uintptr_t)records & 15) == 0, "mk_pose_summary: records must be a 16-byte aligned pointer");
  MK_CHECK_ARG(N >= 1 && N <= kMaxRecords, "mk_pose_summary: need 1 <= N <= %d (the ranking is quadratic in N; got %d)", kMaxRecords, N);
  MK_CHECK_ARG(failures >= 0, "mk_pose_summary: need failures >= 0 (got %d)", failures);
  MK_CHECK_ARG(losses ? S >= 1 : S == 0, "mk_pose_summary: need S >= 1 loss rows with losses, S == 0 without (got %d)", S);
  MK_CHECK_ARG(out && work && ((uintptr_t)work & 7) == 0, "mk_pose_summary: out and an 8-byte aligned work must not be NULL");
  const int nblk = (N + kTile - 1) / kTile;
  const Thresholds th = {th_t, th_R, th_t2, th_R2, th_px};
  hipLaunchKernelGGL(pose_summary_rank_kernel, dim3((unsigned)nblk), dim3(kTile), 0, (hipStream_t)stream, records, N, losses, S, th, work);
  MK_CHECK_LAUNCH();
  hipLaunchKernelGGL(pose_summary_reduce_kernel, dim3(1), dim3(kTile), 0, (hipStream_t)stream, work, nblk, N, failures, S,
                     losses ? 1 : 0, out);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

}  // extern "C"
