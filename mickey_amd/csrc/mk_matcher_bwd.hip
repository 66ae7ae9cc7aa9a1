// mickey_amd -- backward of the dual-softmax matcher for training (reference lib/models/MicKey/model.py:124-134 pushes
// d loss / d final_scores through final_scores = dualSoftmax(dsc0, dsc1) * (scr0^T scr1), feature_matcher.py:64-83,
// compute_correspondences.py:46-50, model.py:201).
//
// Per pair, S = dsc0^T dsc1 / T, optional dustbin alpha on the last row / column / corner, lr / lc the row / column log-sums of
// the augmented matrix, A = exp(S - lr), Bm = exp(S - lc), P = A Bm (cropped), F = P s0 s1^T.  Given G = dL/dF:
//   u_i = sum_j G P s1_j  (= dL/ds0_i),  v_j = sum_i G P s0_i  (= dL/ds1_j),  r = s0 u,  c = s1 v
//   dS  = 2 G s0 s1 P - A r - Bm c,  dL/ddsc0 = dsc1 dS^T / T,  dL/ddsc1 = dsc0 dS / T
//   dL/dalpha = -sum_i exp(alpha - lr_i) r_i - sum_j exp(alpha - lc_j) c_j
// No [n0, n1] intermediate is stored: the forward keeps only the merged log-sums (mk_dual_softmax_train: `lse`, log2 domain,
// exactly what its pass 2 read), and every sweep below recomputes the correlation on the matrix cores from the descriptors,
// on the forward's path (split-fp16 or exact fp32, mk_matcher.hpp):
//   sweep 1    bwd_uv_kernel: the forward's pass-1 grid; per tile G P -> row partials u (per column chunk) and column partials
//              v (per 32-row block); bwd_uv_merge_kernel sums them in a fixed order, bwd_dustbin_kernel reduces dL/dalpha;
//   sweep 2    bwd_dsc_kernel<COLS = 0> (waves own 32 rows) and <COLS = 1> (waves own 32 columns): correlation -> dS in the
//              accumulators -> the gradient GEMM on v_mfma_f32_32x32x2_f32 (exact fp32: dS is not bounded, no split scale
//              needed), the accumulator registers of dS being the MFMA's B operand as they are; partials per chunk of the
//              swept side, summed by bwd_dsc_merge_kernel.  One kernel per gradient instead of one for both: the transposed
//              GEMM in the same sweep would need a partial per 32-row block (60 MB per pair at n = 1938) -- recomputing the
//              correlation is cheaper than writing and re-reading that.
// Deterministic and batch-invariant: every sum has a fixed order (fixed chunk counts, fixed butterflies, fixed-order merges), no
// atomics; a pair's workgroups read and write only that pair's data.
#include "mk_matcher.hpp"

namespace {
using namespace mk;
using namespace mk::ds;

constexpr int NCH2 = 4;        // chunks of the swept side in sweep 2 (FIXED: the summation order does not depend on B)
constexpr float LOG2E_F = 1.4426950408889634f;
constexpr float PAD_L2 = 1e30f;   // log2-sum of a padding row / column: every exp2(v - PAD_L2) is 0
constexpr int GP_BLK = 128 * 32;  // floats per block of 32 keypoints in the gradient-operand planes

// the dustbin in the log2 domain, rounded as the host-side forward rounds `dustbin * LOG2E` (kept from being fused into an fma)
__device__ __forceinline__ float dustbin2(const float* dustbin) {
  float beta2 = dustbin[0] * LOG2E_F;
  asm volatile("" : "+v"(beta2));
  return beta2;
}

// lse_final_kernel (mk_matcher.hip) with the dustbin read on the device: lse2[(b*2+side)*nmax + idx] = log2 sum 2^v2
__global__ __launch_bounds__(256) void lse_merge_dev_kernel(const float* __restrict__ partr, const float* __restrict__ partc,
                                                            float* __restrict__ lse2, const float* __restrict__ dustbin, int n0, int n1,
                                                            int nmax, int nrb, int nchunk) {
  const int idx = blockIdx.x * 256 + threadIdx.x, side = blockIdx.y, b = blockIdx.z;
  if (idx >= (side ? n1 : n0)) return;
  float m = -1e30f, s = 0.f;
  if (side == 0) {
    for (int c = 0; c < nchunk; ++c) {
      const float* q = partr + (((long long)b * nchunk + c) * n0 + idx) * 2;
      lse2_merge(m, s, q[0], q[1]);
    }
  } else {
    for (int rb = 0; rb < nrb; ++rb) {
      const float* q = partc + (((long long)b * nrb + rb) * n1 + idx) * 2;
      lse2_merge(m, s, q[0], q[1]);
    }
  }
  if (dustbin) lse2_merge(m, s, dustbin2(dustbin), 1.0f);
  lse2[((long long)b * 2 + side) * nmax + idx] = m + __builtin_amdgcn_logf(s);
}

// Gradient-operand planes: fp32 [nimg, 128, n] -> [nimg, nblk, 4 (channel block cb), 4 (q), 64 (lane)] x f32x4, element e of
// (cb, q, lane) = dsc[cb*32 + (lane & 31)][blk*32 + e + 8q + 4(lane >> 5)]: the A operand of the gradient GEMM at k-step
// 4q + e, whose B operand is accumulator register 4q + e of a dS tile.  grid (nblk, nimg), 256 threads = (cb, lane)
__global__ __launch_bounds__(256) void grad_planes_kernel(const float* __restrict__ dsc, f32x4* __restrict__ gp, int n, int nblk) {
  const int blk = blockIdx.x, img = blockIdx.y;
  const int cb = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const float* src = dsc + ((long long)img * 128 + cb * 32 + l31) * n;
  f32x4* o = gp + (((long long)img * nblk + blk) * 4 + cb) * 4 * 64 + lane;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int y = blk * 32 + e + 8 * q + 4 * hi;
      w[e] = y < n ? src[y] : 0.f;
    }
    o[q * 64] = w;
  }
}

// sweep 1.  The forward's pass-1 grid (decode_unit_grid(gx = row blocks / 4, NCHUNK_S, B)): a wave holds 32 rows, streams the
// column tiles of one chunk; lane = column j of a tile, register r = row i0 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
// partu[(b*NCHUNK_S + chunk)*n0 + i] = sum over the chunk of G P s1,  partv[(b*nrb + rb)*n1 + j] = sum over the block of G P s0.
// G is read at clamped indices and masked: nothing outside [n0, n1] is touched.
template <bool SPLIT>
__global__ __launch_bounds__(256) void bwd_uv_kernel(
    const float* __restrict__ dsc0, const float* __restrict__ dsc1, const uint4* __restrict__ P0, const uint4* __restrict__ P1,
    float scale2, const float* __restrict__ lse2, const float* __restrict__ scr0, const float* __restrict__ scr1,
    const float* __restrict__ G, float* __restrict__ partu, float* __restrict__ partv, int n0, int n1, int nmax, int nrb, int ntb,
    int gx, int nunits) {
  int bx, by, b;
  if (!decode_unit_grid(gx, NCHUNK_S, nunits, bx, by, b)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int rb = bx * 4 + wave, i0 = rb * RT;
  if (rb >= nrb) return;
  SplitOperand as, bs;
  float a[CMAX / 2], bq[CMAX / 2];
  if (SPLIT)
    as.load(P0 + ((long long)b * nrb + rb) * SP_BLK_U4, lane);
  else
    load_operand<true>(a, dsc0 + (long long)b * 128 * n0, 128, n0, i0 + l31, hi);
  const int per = (ntb + NCHUNK_S - 1) / NCHUNK_S;
  const int jt0 = by * per, jt1 = min(ntb, jt0 + per);
  float lr[16], s0[16], ru[16];
  int ic[16];
  unsigned rowok = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
    ic[r] = i < n0 ? i : n0 - 1;
    rowok |= (i < n0 ? 1u : 0u) << r;
    lr[r] = lse2[((long long)b * 2 + 0) * nmax + ic[r]];
    s0[r] = scr0 ? scr0[(long long)b * n0 + ic[r]] : 1.f;
    ru[r] = 0.f;
  }
  const float* Gb = G + (long long)b * n0 * n1;
  for (int jt = jt0; jt < jt1; ++jt) {
    f32x16 acc;
    if (SPLIT) {
      bs.load(P1 + ((long long)b * ntb + jt) * SP_BLK_U4, lane);
      acc = corr_split(as, bs);
    } else {
      load_operand<true>(bq, dsc1 + (long long)b * 128 * n1, 128, n1, jt * RT + l31, hi);
      acc = corr_regs<true>(a, bq, 128);
      MK_LOADS_THEN_MFMAS();
    }
    const int j = jt * RT + l31;
    const bool jok = j < n1;
    const int jc = jok ? j : n1 - 1;
    const float lc = lse2[((long long)b * 2 + 1) * nmax + jc];
    const float s1 = scr1 ? scr1[(long long)b * n1 + jc] : 1.f;
    float cv = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float g = Gb[(long long)ic[r] * n1 + jc];
      const float v = acc[r] * scale2;
      const float p = __builtin_amdgcn_exp2f((v - lc) + (v - lr[r]));
      const float w = (jok && ((rowok >> r) & 1u)) ? g * p : 0.f;
      ru[r] += w * s1;
      cv += w * s0[r];
    }
    cv += __shfl_xor(cv, 32, 64);   // the other 16 rows of this column live in lane ^ 32
    if (hi == 0 && jok) partv[((long long)b * nrb + rb) * n1 + j] = cv;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {   // the 32 lanes that share rows (same hi): a fixed butterfly
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) ru[r] += __shfl_xor(ru[r], o, 64);
  }
  if (l31 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if ((rowok >> r) & 1u) partu[((long long)b * NCHUNK_S + by) * n0 + ic[r]] = ru[r];
  }
}

// merge of sweep 1 -> the per-side vectors of sweep 2: vec[((b*2 + side)*3 + k)*npad + idx], k = 0: log2-sum (PAD_L2 past the
// end), 1: keypoint score (1 without scores, 0 past the end), 2: r = s u / c = s v (0 past the end); u / v -> g_scr0 / g_scr1.
// grid (npad / 256, 2, B)
__global__ __launch_bounds__(256) void bwd_uv_merge_kernel(const float* __restrict__ partu, const float* __restrict__ partv,
                                                           const float* __restrict__ lse2, const float* __restrict__ scr0,
                                                           const float* __restrict__ scr1, float* __restrict__ vec,
                                                           float* __restrict__ g_scr0, float* __restrict__ g_scr1, int n0, int n1,
                                                           int nmax, int nrb, int npad) {
  const int idx = blockIdx.x * 256 + threadIdx.x, side = blockIdx.y, b = blockIdx.z;
  if (idx >= npad) return;
  const int n = side ? n1 : n0;
  float l2 = PAD_L2, s = 0.f, rr = 0.f;
  if (idx < n) {
    float u = 0.f;
    if (side == 0) {
      for (int c = 0; c < NCHUNK_S; ++c) u += partu[((long long)b * NCHUNK_S + c) * n0 + idx];
    } else {
      for (int rb = 0; rb < nrb; ++rb) u += partv[((long long)b * nrb + rb) * n1 + idx];
    }
    const float* sc = side ? scr1 : scr0;
    float* gs = side ? g_scr1 : g_scr0;
    l2 = lse2[((long long)b * 2 + side) * nmax + idx];
    s = sc ? sc[(long long)b * n + idx] : 1.f;
    rr = s * u;
    if (gs) gs[(long long)b * n + idx] = u;
  }
  float* o = vec + ((long long)b * 2 + side) * 3 * npad + idx;
  o[0] = l2;
  o[npad] = s;
  o[2 * npad] = rr;
}

// dL/dalpha of pair b = -sum_i 2^(alpha2 - lr2_i) r_i - sum_j 2^(alpha2 - lc2_j) c_j: one workgroup per pair, fixed order
__global__ __launch_bounds__(256) void bwd_dustbin_kernel(const float* __restrict__ vec, const float* __restrict__ dustbin,
                                                          float* __restrict__ g_dustbin, int n0, int n1, int npad) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const float beta2 = dustbin2(dustbin);
  float acc = 0.f;
  for (int side = 0; side < 2; ++side) {
    const float* v = vec + ((long long)b * 2 + side) * 3 * npad;
    const int n = side ? n1 : n0;
    for (int idx = threadIdx.x; idx < n; idx += 256) acc += __builtin_amdgcn_exp2f(beta2 - v[idx]) * v[2 * npad + idx];
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) g_dustbin[b] = -(((red[0] + red[1]) + red[2]) + red[3]);
}

// sweep 2.  X = the side whose gradient this instance forms (COLS = 0: image 0, rows of G; COLS = 1: image 1, columns of G),
// Y = the other.  grid decode_unit_grid(gx = X blocks / 4, NCH2, B): a wave holds 32 X keypoints and streams the Y tiles of
// one chunk.  Per tile the correlation is taken as [y][x] (the Y operand streamed as A, the X operand resident as B), so that a
// lane owns ONE x and register r holds y = y0 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5); dS in that layout is, register by
// register, the B operand of k-step r of  gX[c][x] += sum_y dY[c][y] dS[x][y]  (A operand: the gradient-operand planes of Y).
// part[((b*NCH2 + chunk)*128 + c)*npadX + x]: the chunk's sum, for every x of the existing blocks (npadX = X blocks * 32).
// COLS = 0 reads G[x][y] across lanes = 32 rows: the tile is staged coalesced through a wave-private LDS slice (in-order per
// wave: no barrier); COLS = 1 reads G[y][x] coalesced as it is.
template <bool SPLIT, bool COLS>
__global__ __launch_bounds__(256) void bwd_dsc_kernel(const float* __restrict__ dX, const float* __restrict__ dY,
                                                      const uint4* __restrict__ PX, const uint4* __restrict__ PY,
                                                      const f32x4* __restrict__ GPY, float scale2, const float* __restrict__ vec,
                                                      const float* __restrict__ G, float* __restrict__ part, int nX, int nY,
                                                      int nblkX, int nblkY, int npad, int gx, int nunits) {
  __shared__ float gt[4][32 * 33];
  int bx, by, b;
  if (!decode_unit_grid(gx, NCH2, nunits, bx, by, b)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int xb = bx * 4 + wave, x0 = xb * RT;
  if (xb >= nblkX) return;
  float* st = gt[wave];
  SplitOperand xs, ys;
  float xa[CMAX / 2], ya[CMAX / 2];
  if (SPLIT)
    xs.load(PX + ((long long)b * nblkX + xb) * SP_BLK_U4, lane);
  else
    load_operand<true>(xa, dX + (long long)b * 128 * nX, 128, nX, x0 + l31, hi);
  const float* vX = vec + ((long long)b * 2 + (COLS ? 1 : 0)) * 3 * npad;
  const float* vY = vec + ((long long)b * 2 + (COLS ? 0 : 1)) * 3 * npad;
  const int x = x0 + l31;
  const bool xok = x < nX;
  const int xc = xok ? x : nX - 1;
  const float lX = vX[x], sX = vX[npad + x], rX = vX[2 * npad + x];
  const float* Gb = G + (long long)b * nX * nY;
  f32x16 gacc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) gacc[cb][i] = 0.f;
  const int per = (nblkY + NCH2 - 1) / NCH2;
  const int yt0 = by * per, yt1 = min(nblkY, yt0 + per);
  for (int yt = yt0; yt < yt1; ++yt) {
    const int y0 = yt * RT;
    f32x16 acc;
    if (SPLIT) {
      ys.load(PY + ((long long)b * nblkY + yt) * SP_BLK_U4, lane);
      acc = corr_split(ys, xs);
    } else {
      load_operand<true>(ya, dY + (long long)b * 128 * nY, 128, nY, y0 + l31, hi);
      acc = corr_regs<true>(ya, xa, 128);
      MK_LOADS_THEN_MFMAS();
    }
    float g[16];
    if (!COLS) {
      // G rows x0 .. x0 + 31, columns y0 .. y0 + 31: two rows of 128 bytes per load instruction
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int xi = x0 + 2 * rr + hi, yj = y0 + l31;
        const float v = Gb[(long long)(xi < nX ? xi : nX - 1) * nY + (yj < nY ? yj : nY - 1)];
        st[(2 * rr + hi) * 33 + l31] = (xi < nX && yj < nY) ? v : 0.f;
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r = 0; r < 16; ++r) g[r] = st[l31 * 33 + (r & 3) + 8 * (r >> 2) + 4 * hi];
      __builtin_amdgcn_wave_barrier();
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int y = y0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const float v = Gb[(long long)(y < nY ? y : nY - 1) * nX + xc];
        g[r] = (xok && y < nY) ? v : 0.f;
      }
    }
    float dS[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int yq = y0 + 8 * q + 4 * hi;   // 4 consecutive y: registers 4q .. 4q + 3 (16-byte aligned: npad % 32 == 0)
      const f32x4 lY = *(const f32x4*)(vY + yq), sY = *(const f32x4*)(vY + npad + yq), rY = *(const f32x4*)(vY + 2 * npad + yq);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * q + e;
        const float v = acc[r] * scale2;
        const float ax = __builtin_amdgcn_exp2f(v - lX), ay = __builtin_amdgcn_exp2f(v - lY[e]);
        const float d = 2.f * g[r] * sX * sY[e] * (ax * ay) - ax * rX - ay * rY[e];
        dS[r] = (xok && yq + e < nY) ? d : 0.f;
      }
    }
    const f32x4* gp = GPY + ((long long)b * nblkY + yt) * 4 * 4 * 64 + lane;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 w = gp[(cb * 4 + q) * 64];
#pragma unroll
        for (int e = 0; e < 4; ++e) gacc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], dS[4 * q + e], gacc[cb], 0, 0, 0);
      }
  }
  const int npadX = nblkX * RT;
  float* o = part + ((long long)b * NCH2 + by) * 128 * npadX + x;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[(long long)(cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi) * npadX] = gacc[cb][r];
}

// g[b][c][x] = inv_T x the NCH2 chunk partials in order.  grid (nX / 256, 128, B)
__global__ __launch_bounds__(256) void bwd_dsc_merge_kernel(const float* __restrict__ part, float* __restrict__ g, float inv_temperature,
                                                            int nX, int npadX) {
  const int x = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (x >= nX) return;
  float s = 0.f;
  for (int ch = 0; ch < NCH2; ++ch) s += part[(((long long)b * NCH2 + ch) * 128 + c) * npadX + x];
  g[((long long)b * 128 + c) * nX + x] = s * inv_temperature;
}

inline long long up4(long long n) { return (n + 3) & ~3LL; }

// work layout of mk_dual_softmax_bwd (fp32 elements, every piece a multiple of 4: 16-byte aligned when `work` is)
struct BwdWork {
  uint4 *P0, *P1;
  f32x4 *GP0, *GP1;
  float *partu, *partv, *vec, *part0, *part1;
  long long total;
  BwdWork(float* w, int B, int n0, int n1, int split) {
    const long long nrb = (n0 + RT - 1) / RT, ntb = (n1 + RT - 1) / RT, npad = (nrb > ntb ? nrb : ntb) * RT;
    long long off = 0;
    auto take = [&](long long n) {
      float* p = w ? w + off : nullptr;
      off += up4(n);
      return p;
    };
    P0 = (uint4*)take(split ? (long long)B * nrb * SP_BLK_U4 * 4 : 0);   // split planes: the split path only
    P1 = (uint4*)take(split ? (long long)B * ntb * SP_BLK_U4 * 4 : 0);
    GP0 = (f32x4*)take((long long)B * nrb * GP_BLK);
    GP1 = (f32x4*)take((long long)B * ntb * GP_BLK);
    partu = take((long long)B * NCHUNK_S * n0);
    partv = take((long long)B * nrb * n1);
    vec = take((long long)B * 2 * 3 * npad);
    part0 = take((long long)B * NCH2 * 128 * nrb * RT);
    part1 = take((long long)B * NCH2 * 128 * ntb * RT);
    total = off;
  }
};

}  // namespace

namespace mk {
namespace ds {

int lse_merge_dev(const float* partr, const float* partc, float* lse2, const float* dustbin, int B, int n0, int n1, int nrb,
                  int nchunk, hipStream_t st) {
  const int nmax = n0 > n1 ? n0 : n1;
  hipLaunchKernelGGL(lse_merge_dev_kernel, dim3((nmax + 255) / 256, 2, B), dim3(256), 0, st, partr, partc, lse2, dustbin, n0, n1, nmax,
                     nrb, nchunk);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

}  // namespace ds
}  // namespace mk

extern "C" {

long long mk_dual_softmax_train_work_floats(int B, int n0, int n1, int split) {
  return split ? mk_dual_softmax_split_work_floats(B, n0, n1) : mk_dual_softmax_work_floats(B, n0, n1, 0);
}

int mk_dual_softmax_train(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                          const float* dustbin, float* scores, float* kp_scores, float* final_scores, float* lse, float* work, int B,
                          int C, int n0, int n1, int split, mk_stream_t stream) {
  MK_CHECK_ARG(dsc0 && dsc1 && lse && work, "mk_dual_softmax_train: null pointer");
  MK_CHECK_ARG(B > 0 && n0 > 0 && n1 > 0 && C == 128, "mk_dual_softmax_train: need B, n0, n1 > 0 and C == 128");
  MK_CHECK_ARG(scores || final_scores, "mk_dual_softmax_train: needs scores or final_scores");
  MK_CHECK_ARG(((uintptr_t)work & 15) == 0, "mk_dual_softmax_train: work must be 16-byte aligned");
  return mk::ds::dual_softmax_train_fwd(split, dsc0, dsc1, scr0, scr1, inv_temperature, dustbin, scores, kp_scores, final_scores, lse,
                                        work, B, C, n0, n1, (hipStream_t)stream);
}

long long mk_dual_softmax_bwd_work_floats(int B, int n0, int n1, int split) {
  return BwdWork(nullptr, B, n0, n1, split).total;
}

int mk_dual_softmax_bwd(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                        const float* dustbin, const float* lse, const float* G, float* g_dsc0, float* g_dsc1, float* g_scr0,
                        float* g_scr1, float* g_dustbin, float* work, int B, int C, int n0, int n1, int split, mk_stream_t stream) {
  MK_CHECK_ARG(dsc0 && dsc1 && lse && G && work, "mk_dual_softmax_bwd: null pointer");
  MK_CHECK_ARG(B > 0 && n0 > 0 && n1 > 0 && C == 128, "mk_dual_softmax_bwd: need B, n0, n1 > 0 and C == 128");
  MK_CHECK_ARG((scr0 != nullptr) == (scr1 != nullptr), "mk_dual_softmax_bwd: scr0 and scr1 go together");
  MK_CHECK_ARG(scr0 || (!g_scr0 && !g_scr1), "mk_dual_softmax_bwd: g_scr0 / g_scr1 need scr0 and scr1");
  MK_CHECK_ARG(dustbin || !g_dustbin, "mk_dual_softmax_bwd: g_dustbin needs a dustbin");
  MK_CHECK_ARG(((uintptr_t)work & 15) == 0, "mk_dual_softmax_bwd: work must be 16-byte aligned");
  MK_CHECK_ARG(!split || (inv_temperature > 0.f && inv_temperature * LOG2E_F <= 100.f),
               "mk_dual_softmax_bwd: temperature %g too small for the split path", 1.0 / inv_temperature);
  hipStream_t st = (hipStream_t)stream;
  const int nmax = n0 > n1 ? n0 : n1, nrb = (n0 + RT - 1) / RT, ntb = (n1 + RT - 1) / RT;
  const int npad = (nrb > ntb ? nrb : ntb) * RT;
  BwdWork w(work, B, n0, n1, split);
  const float scale2 = split ? inv_temperature * LOG2E_F / (SP_SCALE * SP_SCALE) : inv_temperature * LOG2E_F;
  const int B8 = (B + 7) / 8 * 8;   // see decode_unit_grid
  if (split) {
    int rc = mk::ds::split_planes(dsc0, w.P0, n0, nrb, B, st);
    if (rc == MK_OK) rc = mk::ds::split_planes(dsc1, w.P1, n1, ntb, B, st);
    if (rc != MK_OK) return rc;
  }
  if (g_dsc1) hipLaunchKernelGGL(grad_planes_kernel, dim3(nrb, B), dim3(256), 0, st, dsc0, w.GP0, n0, nrb);
  if (g_dsc0) hipLaunchKernelGGL(grad_planes_kernel, dim3(ntb, B), dim3(256), 0, st, dsc1, w.GP1, n1, ntb);
  MK_CHECK_LAUNCH();
  const int gx1 = (nrb + 3) / 4;
  const dim3 g1((unsigned)gx1 * NCHUNK_S * B8);
  if (split)
    hipLaunchKernelGGL(bwd_uv_kernel<true>, g1, dim3(256), 0, st, dsc0, dsc1, w.P0, w.P1, scale2, lse, scr0, scr1, G, w.partu, w.partv,
                       n0, n1, nmax, nrb, ntb, gx1, B);
  else
    hipLaunchKernelGGL(bwd_uv_kernel<false>, g1, dim3(256), 0, st, dsc0, dsc1, w.P0, w.P1, scale2, lse, scr0, scr1, G, w.partu, w.partv,
                       n0, n1, nmax, nrb, ntb, gx1, B);
  MK_CHECK_LAUNCH();
  hipLaunchKernelGGL(bwd_uv_merge_kernel, dim3((npad + 255) / 256, 2, B), dim3(256), 0, st, w.partu, w.partv, lse, scr0, scr1, w.vec,
                     g_scr0, g_scr1, n0, n1, nmax, nrb, npad);
  MK_CHECK_LAUNCH();
  if (g_dustbin) {
    hipLaunchKernelGGL(bwd_dustbin_kernel, dim3(B), dim3(256), 0, st, w.vec, dustbin, g_dustbin, n0, n1, npad);
    MK_CHECK_LAUNCH();
  }
  if (g_dsc0) {   // X = image 0 (rows), Y = image 1
    const int gx = (nrb + 3) / 4;
    const dim3 g2((unsigned)gx * NCH2 * B8);
    if (split)
      hipLaunchKernelGGL((bwd_dsc_kernel<true, false>), g2, dim3(256), 0, st, dsc0, dsc1, w.P0, w.P1, w.GP1, scale2, w.vec, G, w.part0,
                         n0, n1, nrb, ntb, npad, gx, B);
    else
      hipLaunchKernelGGL((bwd_dsc_kernel<false, false>), g2, dim3(256), 0, st, dsc0, dsc1, w.P0, w.P1, w.GP1, scale2, w.vec, G, w.part0,
                         n0, n1, nrb, ntb, npad, gx, B);
    MK_CHECK_LAUNCH();
    hipLaunchKernelGGL(bwd_dsc_merge_kernel, dim3((n0 + 255) / 256, 128, B), dim3(256), 0, st, w.part0, g_dsc0, inv_temperature, n0,
                       nrb * RT);
    MK_CHECK_LAUNCH();
  }
  if (g_dsc1) {   // X = image 1 (columns), Y = image 0
    const int gx = (ntb + 3) / 4;
    const dim3 g2((unsigned)gx * NCH2 * B8);
    if (split)
      hipLaunchKernelGGL((bwd_dsc_kernel<true, true>), g2, dim3(256), 0, st, dsc1, dsc0, w.P1, w.P0, w.GP0, scale2, w.vec, G, w.part1,
                         n1, n0, ntb, nrb, npad, gx, B);
    else
      hipLaunchKernelGGL((bwd_dsc_kernel<false, true>), g2, dim3(256), 0, st, dsc1, dsc0, w.P1, w.P0, w.GP0, scale2, w.vec, G, w.part1,
                         n1, n0, ntb, nrb, npad, gx, B);
    MK_CHECK_LAUNCH();
    hipLaunchKernelGGL(bwd_dsc_merge_kernel, dim3((n1 + 255) / 256, 128, B), dim3(256), 0, st, w.part1, g_dsc1, inv_temperature, n1,
                       ntb * RT);
    MK_CHECK_LAUNCH();
  }
  return MK_OK;
}

}  // extern "C"
