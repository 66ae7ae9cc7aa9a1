// mickey_amd -- trainable EncoderLayer of the heads' transformer (reference att_layers/transformer_utils.py:40-66 under autograd):
// the bias-free nn.Linears (forward, input gradient, weight gradient) and the two LayerNorm(128) (forward, backward), all fp32.
//
//   forward linear   out[M, N]  = act([A1 | A2][M, K1 + K2] . W[N, K1 + K2]^T)        the [x | m] concat is never materialised
//   input gradient   gA[M, K]   = (G[M, N] . W[N, K]) (* (mask > 0)), columns [0, K1) to one buffer and [K1, K) to another,
//                                 each optionally added to what is there (one writer per element)
//   weight gradient  dW[N, K]   = G^T . [A1 | A2], summed over the M rows in chunks: per-chunk partials, added in chunk order
//   LayerNorm        xh = (u - mean) rstd,  out = xh gamma + beta (+ resid);   gu = rstd (gamma g - mean(gamma g) - xh mean(gamma g xh))
//
// Every contraction runs on v_mfma_f32_16x16x4_f32 (bitwise an fp32 fma chain) in a k order that depends on the shape alone:
// results are bit-identical from run to run, a row of a forward / input-gradient result does not depend on the other rows of the
// call, and every result is linear in the incoming gradient bit for bit under a power-of-two scale.  No atomics anywhere.
//
// One tile for the three GEMM forms: a 64 x 64 output block per workgroup of 4 waves (each 32 x 32 = 2 x 2 MFMA tiles), 16
// contraction steps per LDS stage.  LDS rows hold 16 floats of the contraction index + 4 of padding (80 B: the 16-byte fragment
// reads of 16 rows fall on distinct banks); the forms differ only in how a stage is fetched: both operands along their rows
// (forward), W down its columns (input gradient), both down their columns (weight gradient; transposed on the way into LDS).
// The next stage's global loads are in flight while the MFMAs of the current one run.
#include "mk_common.hpp"

namespace {
using namespace mk;

constexpr int BT = 64;        // output tile edge
constexpr int KT = 16;        // contraction steps per LDS stage
constexpr int LD = KT + 4;    // LDS row, floats
constexpr int STEP = 128;     // rows per weight-gradient / LayerNorm-backward step
constexpr int MAXCHUNK = 32;  // most row chunks of a weight gradient (a chunk is a whole number of steps)
constexpr int DLN = 128;      // LayerNorm width
constexpr int LNB_WAVES = 16; // waves of a LayerNorm-backward workgroup (8 rows of a step each)

// one LDS stage: acc[i][j] += sum_k sRow[32 wm + 16 i + r][k] sCol[32 wn + 16 j + c][k].  A lane ends up with
// rows r = lane & 15, columns c = 4 (lane >> 4) + 0..3 of every 16 x 16 tile.  MFMA e of a lane's 16-byte chunk contracts
// k = {e, 4 + e, 8 + e, 12 + e}: both operands take the same k per lane, the four MFMAs cover the stage once.
__device__ __forceinline__ void mma_stage(const float* sRow, const float* sCol, f32x4 (&acc)[2][2], int wm, int wn, int lane) {
  const int fr = lane & 15, fg = lane >> 4;
  f32x4 rf[2], cf[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    rf[i] = *(const f32x4*)(sRow + (wm * 32 + i * 16 + fr) * LD + fg * 4);
    cf[i] = *(const f32x4*)(sCol + (wn * 32 + i * 16 + fr) * LD + fg * 4);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(cf[j][e], rf[i][e], acc[i][j], 0, 0, 0);
}

__device__ __forceinline__ void zero_acc(f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ void put_row(float* s, int row, int kq, f32x4 v) { *(f32x4*)(s + row * LD + kq) = v; }
__device__ __forceinline__ void put_col(float* s, int row4, int k, f32x4 v) {   // transposing store
#pragma unroll
  for (int e = 0; e < 4; ++e) s[(row4 + e) * LD + k] = v[e];
}

// columns [c, c + 4) of row m of the two-source operand [A1 | A2] (K1 % 4 == 0: a quad never straddles the seam)
__device__ __forceinline__ f32x4 load_cat(const float* __restrict__ a1, long long lda1, int K1, const float* __restrict__ a2,
                                          long long lda2, long long m, int c) {
  return c < K1 ? *(const f32x4*)(a1 + m * lda1 + c) : *(const f32x4*)(a2 + m * lda2 + (c - K1));
}

// row n of a weight that may be given as up to three matrices of wsplit rows each (wq | wk | wv read in place; wsplit == 0: one)
__device__ __forceinline__ const float* w_row(const float* __restrict__ w, const float* __restrict__ w2, const float* __restrict__ w3,
                                              int wsplit, long long n, int K) {
  if (wsplit == 0 || n < wsplit) return w + n * K;
  return n < 2 * wsplit ? w2 + (n - wsplit) * K : w3 + (n - 2 * wsplit) * K;
}

// columns [c, c + 4) of row m of a gradient that may lie as planes of gsplit columns, gplane elements apart (gq | gk | gv as the
// attention backward leaves them; gsplit == 0: one matrix)
__device__ __forceinline__ const float* g_at(const float* __restrict__ g, long long ldg, long long gplane, int gsplit, long long m, int c) {
  if (gsplit == 0) return g + m * ldg + c;
  const int pl = c / gsplit;
  return g + pl * gplane + m * ldg + (c - pl * gsplit);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lin_fwd_kernel(const float* __restrict__ a1, long long lda1, int K1, const float* __restrict__ a2,
                                                      long long lda2, int K2, const float* __restrict__ w, const float* __restrict__ w2,
                                                      const float* __restrict__ w3, int wsplit, float* __restrict__ out,
                                                      long long ldo, int M, int N, int relu) {
  __shared__ __attribute__((aligned(16))) float sA[BT * LD], sW[BT * LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BT, n0 = blockIdx.y * BT, K = K1 + K2;
  const int row = t >> 2, kq = (t & 3) * 4;
  const long long m = m0 + row, n = n0 + row;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto ldA = [&](int k0) { return m < M ? load_cat(a1, lda1, K1, a2, lda2, m, k0 + kq) : zero; };
  const float* wr = n < N ? w_row(w, w2, w3, wsplit, n, K) : nullptr;
  auto ldW = [&](int k0) { return wr ? *(const f32x4*)(wr + k0 + kq) : zero; };
  f32x4 acc[2][2];
  zero_acc(acc);
  f32x4 ra = ldA(0), rw = ldW(0);
  for (int k0 = 0; k0 < K; k0 += KT) {
    put_row(sA, row, kq, ra);
    put_row(sW, row, kq, rw);
    __syncthreads();
    if (k0 + KT < K) {
      ra = ldA(k0 + KT);
      rw = ldW(k0 + KT);
    }
    mma_stage(sA, sW, acc, wm, wn, lane);
    __syncthreads();
  }
  const int fr = lane & 15, fg = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long om = m0 + wm * 32 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int on = n0 + wn * 32 + j * 16 + fg * 4;
      if (om >= M || on >= N) continue;
      f32x4 v = acc[i][j];
      if (relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : (v[e] != v[e] ? v[e] : 0.f);   // a NaN stays a NaN
      }
      *(f32x4*)(out + om * ldo + on) = v;
    }
  }
}

// ---- forward with the LayerNorm(128) in the accumulators (merge + norm1, mlp[2] + norm2 + the residual) --------------------------
// N == 128: a workgroup owns 64 whole rows, wave w rows 16 w .. 16 w + 15 and all 8 column tiles.  A lane holds 32 values of one
// row (columns 16 j + 4 (lane >> 4) + e); the row sums finish over the 4 lanes that share lane & 15 (xor 16, 32).  Two passes
// over the registers (mean, then squared deviations), as the row kernel does.
__global__ __launch_bounds__(256) void lin_ln_fwd_kernel(const float* __restrict__ a1, long long lda1, int K1, const float* __restrict__ a2,
                                                         long long lda2, int K2, const float* __restrict__ w, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, const float* __restrict__ resid,
                                                         long long ldr, float* __restrict__ out, float* __restrict__ xhat,
                                                         float* __restrict__ rstd_out, int M) {
  __shared__ __attribute__((aligned(16))) float sA[BT * LD], sW[DLN * LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * BT, K = K1 + K2;
  const int row = t >> 2, kq = (t & 3) * 4;
  const long long m = m0 + row;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto ldA = [&](int k0) { return m < M ? load_cat(a1, lda1, K1, a2, lda2, m, k0 + kq) : zero; };
  auto ldW = [&](int k0, int h) { return *(const f32x4*)(w + (long long)(row + 64 * h) * K + k0 + kq); };
  f32x4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = zero;
  f32x4 ra = ldA(0), rw0 = ldW(0, 0), rw1 = ldW(0, 1);
  const int fr = lane & 15, fg = lane >> 4;
  for (int k0 = 0; k0 < K; k0 += KT) {
    put_row(sA, row, kq, ra);
    put_row(sW, row, kq, rw0);
    put_row(sW, row + 64, kq, rw1);
    __syncthreads();
    if (k0 + KT < K) {
      ra = ldA(k0 + KT);
      rw0 = ldW(k0 + KT, 0);
      rw1 = ldW(k0 + KT, 1);
    }
    const f32x4 rf = *(const f32x4*)(sA + (wave * 16 + fr) * LD + fg * 4);
    f32x4 cf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cf[j] = *(const f32x4*)(sW + (j * 16 + fr) * LD + fg * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(cf[j][e], rf[e], acc[j], 0, 0, 0);
    __syncthreads();
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += (acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3]);
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  const float mean = s * (1.0f / DLN);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc[j] -= mean;
    q += (acc[j][0] * acc[j][0] + acc[j][1] * acc[j][1]) + (acc[j][2] * acc[j][2] + acc[j][3] * acc[j][3]);
  }
  q += __shfl_xor(q, 16, 64);
  q += __shfl_xor(q, 32, 64);
  const float rstd = 1.0f / sqrtf(q * (1.0f / DLN) + eps);
  const long long om = m0 + wave * 16 + fr;
  if (om >= M) return;   // (after the shuffles: every lane took part)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int n = j * 16 + fg * 4;
    const f32x4 xh = acc[j] * rstd;
    f32x4 o = xh * *(const f32x4*)(gamma + n) + *(const f32x4*)(beta + n);
    if (resid) o += *(const f32x4*)(resid + om * ldr + n);
    *(f32x4*)(out + om * DLN + n) = o;
    if (xhat) *(f32x4*)(xhat + om * DLN + n) = xh;
  }
  if (rstd_out && fg == 0) rstd_out[om] = rstd;
}

// ---- input gradient -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lin_dgrad_kernel(const float* __restrict__ g, long long ldg, long long gplane, int gsplit, const float* __restrict__ w,
                                                        const float* __restrict__ w2, const float* __restrict__ w3, int wsplit,
                                                        const float* __restrict__ mask, long long ldmask, float* __restrict__ o1,
                                                        long long ldo1, int K1, float* __restrict__ o2, long long ldo2, int K2,
                                                        int accumulate, int M, int N) {
  __shared__ __attribute__((aligned(16))) float sG[BT * LD], sW[BT * LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BT, j0 = blockIdx.y * BT, K = K1 + K2;
  const int row = t >> 2, kq = (t & 3) * 4;   // G: along its rows
  const int kk = t >> 4, jq = (t & 15) * 4;   // W: row n = c0 + kk, columns j0 + jq ..
  const long long m = m0 + row;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto ldG = [&](int c0) { return m < M ? *(const f32x4*)g_at(g, ldg, gplane, gsplit, m, c0 + kq) : zero; };
  auto ldW = [&](int c0) { return j0 + jq < K ? *(const f32x4*)(w_row(w, w2, w3, wsplit, c0 + kk, K) + j0 + jq) : zero; };
  f32x4 acc[2][2];
  zero_acc(acc);
  f32x4 rg = ldG(0), rw = ldW(0);
  for (int c0 = 0; c0 < N; c0 += KT) {
    put_row(sG, row, kq, rg);
    put_col(sW, jq, kk, rw);
    __syncthreads();
    if (c0 + KT < N) {
      rg = ldG(c0 + KT);
      rw = ldW(c0 + KT);
    }
    mma_stage(sG, sW, acc, wm, wn, lane);
    __syncthreads();
  }
  const int fr = lane & 15, fg = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long om = m0 + wm * 32 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int oj = j0 + wn * 32 + j * 16 + fg * 4;
      if (om >= M || oj >= K) continue;
      f32x4 v = acc[i][j];
      if (mask) {   // ReLU backward: an exact zero where the activation is <= 0, the gradient elsewhere (a NaN activation passes it)
        const f32x4 h = *(const f32x4*)(mask + om * ldmask + oj);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = h[e] <= 0.f ? 0.f : v[e];
      }
      float* dst = oj < K1 ? o1 + om * ldo1 + oj : o2 + om * ldo2 + (oj - K1);
      if (accumulate & (oj < K1 ? 1 : 2)) v += *(const f32x4*)dst;
      *(f32x4*)dst = v;
    }
  }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// chunk c (blockIdx.z) sums rows [c rows_per_chunk, (c + 1) rows_per_chunk) of the call into part[c * chunk_stride + n K + k];
// a chunk past the last row writes zeros (a call with fewer rows than the one that sized the work buffer)
__global__ __launch_bounds__(256) void lin_wgrad_kernel(const float* __restrict__ g, long long ldg, long long gplane, int gsplit, const float* __restrict__ a1,
                                                        long long lda1, int K1, const float* __restrict__ a2, long long lda2, int K2,
                                                        float* __restrict__ part, long long chunk_stride, int rows_per_chunk, int M,
                                                        int N) {
  __shared__ __attribute__((aligned(16))) float sG[BT * LD], sA[BT * LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * BT, k0 = blockIdx.y * BT, K = K1 + K2;
  const long long r0 = (long long)blockIdx.z * rows_per_chunk;
  const long long r1 = min((long long)M, r0 + rows_per_chunk);
  const int kk = t >> 4, q4 = (t & 15) * 4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto ldG = [&](long long r) { return (r + kk < r1 && n0 + q4 < N) ? *(const f32x4*)g_at(g, ldg, gplane, gsplit, r + kk, n0 + q4) : zero; };
  auto ldA = [&](long long r) { return (r + kk < r1 && k0 + q4 < K) ? load_cat(a1, lda1, K1, a2, lda2, r + kk, k0 + q4) : zero; };
  f32x4 acc[2][2];
  zero_acc(acc);
  f32x4 rg = ldG(r0), ra = ldA(r0);
  for (long long r = r0; r < r1; r += KT) {
    put_col(sG, q4, kk, rg);
    put_col(sA, q4, kk, ra);
    __syncthreads();
    if (r + KT < r1) {
      rg = ldG(r + KT);
      ra = ldA(r + KT);
    }
    mma_stage(sG, sA, acc, wm, wn, lane);
    __syncthreads();
  }
  const int fr = lane & 15, fg = lane >> 4;
  float* dst = part + (long long)blockIdx.z * chunk_stride;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int on = n0 + wm * 32 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ok = k0 + wn * 32 + j * 16 + fg * 4;
      if (on < N && ok < K) *(f32x4*)(dst + (long long)on * K + ok) = acc[i][j];
    }
  }
}

// ---- the tail: chunk partials -> gradients, added in chunk order ---------------------------------------------------------------
// out[j] = sum_c wpart[c wstride + j] for j < nw (weight gradients), out[nw + j] = sum_s lpart[s lstride + j] for j < nl (LayerNorm)
__global__ __launch_bounds__(256) void tail_kernel(const float* __restrict__ wpart, long long wstride, int wchunks, long long nw,
                                                   const float* __restrict__ lpart, long long lstride, int lsteps, long long nl,
                                                   float* __restrict__ out) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= nw + nl) return;
  const float* p = j < nw ? wpart + j : lpart + (j - nw);
  const long long stride = j < nw ? wstride : lstride;
  const int n = j < nw ? wchunks : lsteps;
  float s = 0.f;
#pragma unroll 8
  for (int c = 0; c < n; ++c) s += p[c * stride];
  out[j] = s;
}

// ---- LayerNorm(128) -----------------------------------------------------------------------------------------------------------
// a wave per row, a lane holds columns 2 lane, 2 lane + 1; row sums by xor-shuffle (the same tree for every row)
__device__ __forceinline__ void ln_row_stats(float2 u, float eps, float& mean, float& rstd) {
  mean = wave_sum(u.x + u.y) * (1.0f / DLN);
  const float dx = u.x - mean, dy = u.y - mean;
  const float var = wave_sum(dx * dx + dy * dy) * (1.0f / DLN);
  rstd = 1.0f / sqrtf(var + eps);
}

__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ u, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps, const float* __restrict__ resid,
                                                     long long ldr, float* __restrict__ out, float* __restrict__ xhat,
                                                     float* __restrict__ rstd_out, int M) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float2 gm = *(const float2*)(gamma + 2 * lane), bt = *(const float2*)(beta + 2 * lane);
  for (long long m = (long long)blockIdx.x * 16 + wave; m < min((long long)M, (long long)blockIdx.x * 16 + 16); m += 4) {
    const float2 v = *(const float2*)(u + m * DLN + 2 * lane);
    float mean, rstd;
    ln_row_stats(v, eps, mean, rstd);
    const float2 xh = make_float2((v.x - mean) * rstd, (v.y - mean) * rstd);
    float2 o = make_float2(xh.x * gm.x + bt.x, xh.y * gm.y + bt.y);
    if (resid) {
      const float2 r = *(const float2*)(resid + m * ldr + 2 * lane);
      o.x += r.x;
      o.y += r.y;
    }
    *(float2*)(out + m * DLN + 2 * lane) = o;
    if (xhat) *(float2*)(xhat + m * DLN + 2 * lane) = xh;
    if (rstd_out && lane == 0) rstd_out[m] = rstd;
  }
}

// block = one step of 128 rows; gu for its rows, and the step's column sums of g xh | g to part[step * part_stride + 0..255]
// (16 waves of 8 rows each, their partials added in wave order; part may be null: no affine gradient wanted)
__global__ __launch_bounds__(LNB_WAVES * 64) void ln_bwd_kernel(const float* __restrict__ g, const float* __restrict__ xhat,
                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                     float* __restrict__ gu, float* __restrict__ part, long long part_stride, int M) {
  __shared__ float red[LNB_WAVES][2 * DLN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float2 gm = *(const float2*)(gamma + 2 * lane);
  const long long m0 = (long long)blockIdx.x * STEP, m1 = min((long long)M, m0 + STEP);
  float2 sgx = make_float2(0.f, 0.f), sg = make_float2(0.f, 0.f);
  for (long long m = m0 + wave; m < m1; m += LNB_WAVES) {
    const float2 gv = *(const float2*)(g + m * DLN + 2 * lane), xh = *(const float2*)(xhat + m * DLN + 2 * lane);
    sgx.x += gv.x * xh.x;
    sgx.y += gv.y * xh.y;
    sg.x += gv.x;
    sg.y += gv.y;
    if (gu) {
      const float2 a = make_float2(gv.x * gm.x, gv.y * gm.y);
      const float c1 = wave_sum(a.x + a.y) * (1.0f / DLN);
      const float c2 = wave_sum(a.x * xh.x + a.y * xh.y) * (1.0f / DLN);
      const float rs = rstd[m];
      *(float2*)(gu + m * DLN + 2 * lane) = make_float2(rs * (a.x - c1 - xh.x * c2), rs * (a.y - c1 - xh.y * c2));
    }
  }
  if (!part) return;   // (uniform: a kernel argument)
  red[wave][2 * lane] = sgx.x;
  red[wave][2 * lane + 1] = sgx.y;
  red[wave][DLN + 2 * lane] = sg.x;
  red[wave][DLN + 2 * lane + 1] = sg.y;
  __syncthreads();
  const int c = threadIdx.x;
  if (c >= 2 * DLN) return;
  float r = red[0][c];
#pragma unroll
  for (int w = 1; w < LNB_WAVES; ++w) r += red[w][c];
  part[(long long)blockIdx.x * part_stride + c] = r;
}

bool al16(const void* p) { return p && ((uintptr_t)p & 15) == 0; }
bool ld_ok(long long ld, int cols) { return ld >= cols && ld % 4 == 0; }
bool g_ok(long long ldg, long long gplane, int gsplit, int N) {
  if (gsplit == 0) return ld_ok(ldg, N);
  return gsplit > 0 && gsplit % KT == 0 && N % gsplit == 0 && ld_ok(ldg, gsplit) && gplane >= 0 && gplane % 4 == 0;
}
int steps_of(int M) { return (M + STEP - 1) / STEP; }
int rows_per_chunk_of(int M) { return STEP * ((steps_of(M) + MAXCHUNK - 1) / MAXCHUNK); }

}  // namespace

int mk_train_rows_per_chunk(int M) { return M > 0 ? rows_per_chunk_of(M) : 0; }
int mk_train_chunks(int M) { return M > 0 ? (M + rows_per_chunk_of(M) - 1) / rows_per_chunk_of(M) : 0; }
int mk_train_ln_steps(int M) { return M > 0 ? steps_of(M) : 0; }

int mk_train_linear_fwd(const float* a1, long long lda1, int K1, const float* a2, long long lda2, int K2, const float* w, const float* w2,
                        const float* w3, int wsplit, float* out, long long ldo, int M, int N, int relu, mk_stream_t stream) {
  MK_CHECK_ARG(M > 0 && N > 0 && N % 4 == 0 && K1 > 0 && K1 % KT == 0 && K2 >= 0 && K2 % KT == 0,
               "mk_train_linear_fwd: bad shape (M %d, N %d, K1 %d, K2 %d; N %% 4 == 0, K1 and K2 multiples of 16)", M, N, K1, K2);
  MK_CHECK_ARG(al16(a1) && ld_ok(lda1, K1) && (K2 == 0 || (al16(a2) && ld_ok(lda2, K2))),
               "mk_train_linear_fwd: operands must be non-null, 16-byte aligned, row strides >= K and multiples of 4");
  MK_CHECK_ARG(al16(w) && al16(out) && ld_ok(ldo, N), "mk_train_linear_fwd: w and out must be non-null and 16-byte aligned, ldo >= N, ldo %% 4 == 0");
  MK_CHECK_ARG(wsplit == 0 || (wsplit % KT == 0 && N == 3 * wsplit && al16(w2) && al16(w3)),
               "mk_train_linear_fwd: a split weight is three 16-byte aligned matrices of wsplit rows, wsplit %% 16 == 0, N == 3 wsplit");
  MK_CHECK_ARG((N + BT - 1) / BT <= 65535, "mk_train_linear_fwd: N %d too large", N);
  hipLaunchKernelGGL(lin_fwd_kernel, dim3((M + BT - 1) / BT, (N + BT - 1) / BT), dim3(256), 0, (hipStream_t)stream, a1, lda1, K1, a2, lda2,
                     K2, w, w2, w3, wsplit, out, ldo, M, N, relu);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_train_linear_ln128_fwd(const float* a1, long long lda1, int K1, const float* a2, long long lda2, int K2, const float* w,
                              const float* gamma, const float* beta, float eps, const float* resid, long long ldr, float* out,
                              float* xhat, float* rstd, int M, mk_stream_t stream) {
  MK_CHECK_ARG(M > 0 && K1 > 0 && K1 % KT == 0 && K2 >= 0 && K2 % KT == 0 && eps >= 0.f && eps == eps,
               "mk_train_linear_ln128_fwd: bad shape or eps (M %d, K1 %d, K2 %d, eps %g; K1 and K2 multiples of 16)", M, K1, K2, (double)eps);
  MK_CHECK_ARG(al16(a1) && ld_ok(lda1, K1) && (K2 == 0 || (al16(a2) && ld_ok(lda2, K2))),
               "mk_train_linear_ln128_fwd: operands must be non-null, 16-byte aligned, row strides >= K and multiples of 4");
  MK_CHECK_ARG(al16(w) && al16(gamma) && al16(beta) && al16(out), "mk_train_linear_ln128_fwd: w, gamma, beta, out must be non-null and 16-byte aligned");
  MK_CHECK_ARG((!resid || (al16(resid) && ld_ok(ldr, DLN))) && (!xhat || al16(xhat)) && (!rstd || al16(rstd)),
               "mk_train_linear_ln128_fwd: resid, xhat, rstd must be 16-byte aligned, ldr >= 128 and a multiple of 4");
  hipLaunchKernelGGL(lin_ln_fwd_kernel, dim3((M + BT - 1) / BT), dim3(256), 0, (hipStream_t)stream, a1, lda1, K1, a2, lda2, K2, w, gamma,
                     beta, eps, resid, ldr, out, xhat, rstd, M);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_train_linear_dgrad(const float* g, long long ldg, long long gplane, int gsplit, const float* w, const float* w2, const float* w3, int wsplit, const float* mask, long long ldmask, float* o1,
                          long long ldo1, int K1, float* o2, long long ldo2, int K2, int accumulate, int M, int N,
                          mk_stream_t stream) {
  MK_CHECK_ARG(M > 0 && N > 0 && N % KT == 0 && K1 > 0 && K1 % 4 == 0 && K2 >= 0 && K2 % 4 == 0,
               "mk_train_linear_dgrad: bad shape (M %d, N %d, K1 %d, K2 %d; N %% 16 == 0, K1 and K2 multiples of 4)", M, N, K1, K2);
  MK_CHECK_ARG(al16(g) && g_ok(ldg, gplane, gsplit, N) && al16(w),
               "mk_train_linear_dgrad: g and w must be non-null and 16-byte aligned, ldg >= the row's width, ldg and gplane multiples of 4, N %% gsplit == 0");
  MK_CHECK_ARG(!mask || (al16(mask) && ld_ok(ldmask, K1 + K2)), "mk_train_linear_dgrad: mask must be 16-byte aligned with ldmask >= K, ldmask %% 4 == 0");
  MK_CHECK_ARG(al16(o1) && ld_ok(ldo1, K1) && (K2 == 0 || (al16(o2) && ld_ok(ldo2, K2))),
               "mk_train_linear_dgrad: outputs must be non-null, 16-byte aligned, row strides >= their width and multiples of 4");
  MK_CHECK_ARG(wsplit == 0 || (wsplit % KT == 0 && N == 3 * wsplit && al16(w2) && al16(w3)),
               "mk_train_linear_dgrad: a split weight is three 16-byte aligned matrices of wsplit rows, wsplit %% 16 == 0, N == 3 wsplit");
  MK_CHECK_ARG((K1 + K2 + BT - 1) / BT <= 65535, "mk_train_linear_dgrad: K %d too large", K1 + K2);
  hipLaunchKernelGGL(lin_dgrad_kernel, dim3((M + BT - 1) / BT, (K1 + K2 + BT - 1) / BT), dim3(256), 0, (hipStream_t)stream, g, ldg, gplane, gsplit, w, w2, w3,
                     wsplit, mask, ldmask, o1, ldo1, K1, o2, ldo2, K2, accumulate, M, N);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_train_linear_wgrad(const float* g, long long ldg, long long gplane, int gsplit, const float* a1, long long lda1, int K1, const float* a2, long long lda2,
                          int K2, float* part, long long chunk_stride, int rows_per_chunk, int chunks, int M, int N,
                          mk_stream_t stream) {
  MK_CHECK_ARG(M > 0 && N > 0 && N % 4 == 0 && K1 > 0 && K1 % 4 == 0 && K2 >= 0 && K2 % 4 == 0,
               "mk_train_linear_wgrad: bad shape (M %d, N %d, K1 %d, K2 %d; N, K1, K2 multiples of 4)", M, N, K1, K2);
  MK_CHECK_ARG(al16(g) && g_ok(ldg, gplane, gsplit, N) && al16(a1) && ld_ok(lda1, K1) && (K2 == 0 || (al16(a2) && ld_ok(lda2, K2))),
               "mk_train_linear_wgrad: operands must be non-null, 16-byte aligned, row strides >= their width and multiples of 4");
  MK_CHECK_ARG(rows_per_chunk > 0 && rows_per_chunk % KT == 0 && chunks > 0 && chunks <= 65535 &&
                   (long long)rows_per_chunk * chunks >= M,
               "mk_train_linear_wgrad: %d chunks of %d rows (a multiple of 16) do not cover M %d", chunks, rows_per_chunk, M);
  MK_CHECK_ARG(al16(part) && chunk_stride >= (long long)N * (K1 + K2) && chunk_stride % 4 == 0,
               "mk_train_linear_wgrad: part must be non-null and 16-byte aligned, chunk_stride >= N K and a multiple of 4");
  MK_CHECK_ARG((K1 + K2 + BT - 1) / BT <= 65535, "mk_train_linear_wgrad: K %d too large", K1 + K2);
  hipLaunchKernelGGL(lin_wgrad_kernel, dim3((N + BT - 1) / BT, (K1 + K2 + BT - 1) / BT, chunks), dim3(256), 0, (hipStream_t)stream, g, ldg,
                     gplane, gsplit, a1, lda1, K1, a2, lda2, K2, part, chunk_stride, rows_per_chunk, M, N);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_train_tail(const float* wpart, long long wstride, int wchunks, long long nw, const float* lpart, long long lstride, int lsteps,
                  long long nl, float* out, mk_stream_t stream) {
  MK_CHECK_ARG(nw >= 0 && nl >= 0 && nw + nl > 0 && out, "mk_train_tail: nothing to add (nw %lld, nl %lld) or out is null", nw, nl);
  MK_CHECK_ARG(nw == 0 || (wpart && wchunks > 0 && wstride >= nw), "mk_train_tail: weight partials need wpart, wchunks > 0, wstride >= nw");
  MK_CHECK_ARG(nl == 0 || (lpart && lsteps > 0 && lstride >= nl), "mk_train_tail: LayerNorm partials need lpart, lsteps > 0, lstride >= nl");
  hipLaunchKernelGGL(tail_kernel, dim3((unsigned)((nw + nl + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wpart, wstride, wchunks, nw,
                     lpart, lstride, lsteps, nl, out);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_train_ln128_fwd(const float* u, const float* gamma, const float* beta, float eps, const float* resid, long long ldr, float* out,
                       float* xhat, float* rstd, int M, mk_stream_t stream) {
  MK_CHECK_ARG(M > 0 && eps >= 0.f && eps == eps, "mk_train_ln128_fwd: bad M %d or eps %g", M, (double)eps);
  MK_CHECK_ARG(al16(u) && al16(gamma) && al16(beta) && al16(out), "mk_train_ln128_fwd: u, gamma, beta, out must be non-null and 16-byte aligned");
  MK_CHECK_ARG((!resid || (al16(resid) && ld_ok(ldr, DLN))) && (!xhat || al16(xhat)) && (!rstd || al16(rstd)),
               "mk_train_ln128_fwd: resid, xhat, rstd must be 16-byte aligned, ldr >= 128 and a multiple of 4");
  hipLaunchKernelGGL(ln_fwd_kernel, dim3((M + 15) / 16), dim3(256), 0, (hipStream_t)stream, u, gamma, beta, eps, resid, ldr, out, xhat, rstd, M);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_train_ln128_bwd(const float* g, const float* xhat, const float* rstd, const float* gamma, float* gu, float* part,
                       long long part_stride, int M, mk_stream_t stream) {
  MK_CHECK_ARG(M > 0, "mk_train_ln128_bwd: bad M %d", M);
  MK_CHECK_ARG(al16(g) && al16(xhat) && al16(rstd) && al16(gamma), "mk_train_ln128_bwd: g, xhat, rstd, gamma must be non-null and 16-byte aligned");
  MK_CHECK_ARG((!gu || al16(gu)) && (!part || (al16(part) && part_stride >= 2 * DLN)),
               "mk_train_ln128_bwd: gu and part must be 16-byte aligned, part_stride >= 256");
  if (!gu && !part) return MK_OK;
  hipLaunchKernelGGL(ln_bwd_kernel, dim3(steps_of(M)), dim3(LNB_WAVES * 64), 0, (hipStream_t)stream, g, xhat, rstd, gamma, gu, part, part_stride, M);
  MK_CHECK_LAUNCH();
  return MK_OK;
}
