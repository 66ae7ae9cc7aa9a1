// mickey_amd -- the glue of the heads' BasicBlock for TRAINING (reference utils/extractor_utils.py:12-35 under autograd): BatchNorm2d
// with batch statistics (or, in eval mode, the running ones), the residual add and the ReLU in one pass, forward and backward.  fp32
// data on the vector ALU, the forward in fp32 arithmetic, the backward's sums and x - mean terms in fp64 (see there); rows are [M, C] with the channels innermost (channels_last memory, what the 3x3 convolutions return).
//
// Layout of every kernel: a workgroup is 16 row slots x 16 lanes, a lane owns 4 consecutive channels (16-byte loads and stores), so a
// workgroup covers a slab of 64 channels (every lane busy at C = 64) and a chunk of kChunkRows rows, slot s walking rows s, s + 16, ...
// Every per-channel sum runs slot by slot, then chunk by chunk, each in index order: no atomics, no host synchronisation, results
// bit-identical from run to run.  A chunk's partial is written by one launch and combined in the prologue of the next one, by every
// workgroup for its own 64 channels: nothing crosses workgroups inside a launch.
#include "mk_common.hpp"

namespace {
using namespace mk;

constexpr int kChunkRows = 256;   // rows of one statistics partial (mk_train_bn_chunk_rows): 16 rows for each of a workgroup's 16 slots
constexpr int kMinC = 4, kMaxC = 1024;

struct Geo {
  int q, slot, c4;     // lane of the slab, row slot, channel quad
  bool on;             // the quad exists (C / 4 need be no multiple of 16)
  long long r0, r1;    // the chunk's rows
};
__device__ __forceinline__ Geo geo(int M, int C) {
  Geo g;
  g.q = threadIdx.x & 15;
  g.slot = threadIdx.x >> 4;
  g.c4 = blockIdx.y * 16 + g.q;
  g.on = g.c4 < (C >> 2);
  g.r0 = (long long)blockIdx.x * kChunkRows;
  g.r1 = g.r0 + kChunkRows < M ? g.r0 + kChunkRows : M;
  return g;
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 splat(float v) { return f32x4{v, v, v, v}; }

// the 16 slots' values of a quad, added in slot order; every thread of the quad's column gets the sum.  red: [16][16] quads
template <typename V>
__device__ __forceinline__ V slot_sum(V v, V* red, int slot, int q) {
  __syncthreads();   // (the previous use of red is over)
  red[slot * 16 + q] = v;
  __syncthreads();
  V s = red[q];
#pragma unroll
  for (int j = 1; j < 16; ++j) s += red[j * 16 + q];
  return s;
}

// per-channel sum over the chunks of f(chunk), for the slab's 64 channels: thread (run = t >> 6, channel = t & 63) adds its quarter of
// the chunks in chunk order, the four runs are then added in run order.  Every thread returns the sum of its own channel.
template <typename T, typename F>
__device__ __forceinline__ T chunk_sum(int chunks, T* red, F f) {
  const int cl = threadIdx.x & 63, run = threadIdx.x >> 6;
  const int per = (chunks + 3) >> 2;
  const int k0 = run * per, k1 = k0 + per < chunks ? k0 + per : chunks;
  T s = 0;
  for (int k = k0; k < k1; ++k) s += f(k);
  __syncthreads();
  red[run * 64 + cl] = s;
  __syncthreads();
  return ((red[cl] + red[64 + cl]) + red[128 + cl]) + red[192 + cl];
}

// ---- forward, launch 1: part[chunk][0][c] = the chunk's mean, part[chunk][1][c] = its sum of squared deviations from that mean ----
// Two passes over the chunk (the second one meets it in the cache): the sum is taken of x - K with K the chunk's first row, so that a
// mean far above the spread costs no digits, and the squares are taken about the chunk's own mean.
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, long long ldx, float* __restrict__ part, int M, int C) {
  __shared__ f32x4 red[256];
  const Geo g = geo(M, C);
  const float n = (float)(g.r1 - g.r0);
  const float* xc = x + g.c4 * 4;
  f32x4 K = splat(0.f), s = splat(0.f), m2 = splat(0.f);
  if (g.on) {
    K = ld4(xc + g.r0 * ldx);
#pragma unroll 4
    for (long long r = g.r0 + g.slot; r < g.r1; r += 16) s += ld4(xc + r * ldx) - K;
  }
  const f32x4 mean = K + slot_sum(s, red, g.slot, g.q) / n;
  if (g.on)
#pragma unroll 4
    for (long long r = g.r0 + g.slot; r < g.r1; r += 16) {
      const f32x4 d = ld4(xc + r * ldx) - mean;
      m2 += d * d;
    }
  m2 = slot_sum(m2, red, g.slot, g.q);
  if (g.on && g.slot == 0) {
    float* p = part + (long long)blockIdx.x * 2 * C + g.c4 * 4;
    *(f32x4*)p = mean;
    *(f32x4*)(p + C) = m2;
  }
}

// ---- forward, launch 2: y = act((x - mean) rstd gamma + beta (+ resid)) ------------------------------------------------------------
// TRAIN: mean and the biased variance from the partials -- mean = m_0 + sum_k n_k (m_k - m_0) / M, var = sum_k (M2_k + n_k (m_k - mean)^2)
// / M, the pairwise combination of centred moments written as two sums in chunk order -- and the workgroups of chunk 0 update the
// running statistics of their channels (the first of them the batch counter).  Eval: mean and var are the running ones.
template <bool TRAIN, bool RELU, bool RESID>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ resid, long long ldr,
                                                       float* running_mean, float* running_var, long long* nbt, float momentum, float eps,
                                                       const float* __restrict__ part, float* __restrict__ y, long long ldy,
                                                       float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                       unsigned char* __restrict__ mask, int M, int C) {
  __shared__ __attribute__((aligned(16))) float red[256];
  __shared__ __attribute__((aligned(16))) float smean[64], srstd[64];
  const Geo g = geo(M, C);
  {
    const int cl = threadIdx.x & 63, c = blockIdx.y * 64 + cl;
    const bool on = c < C;
    float mean = 0.f, var = 1.f;
    double dvar = 1.0;
    if (TRAIN) {
      const int chunks = (M + kChunkRows - 1) / kChunkRows;
      const float fM = (float)M;
      const float m0 = on ? part[c] : 0.f;
      auto rows = [&](int k) { return (float)(k + 1 < chunks ? kChunkRows : M - k * kChunkRows); };
      const float sd = chunk_sum(chunks, red, [&](int k) { return on ? rows(k) * (part[(long long)k * 2 * C + c] - m0) : 0.f; });
      mean = m0 + sd / fM;
      const float sv = chunk_sum(chunks, red, [&](int k) {
        if (!on) return 0.f;
        const float d = part[(long long)k * 2 * C + c] - mean;
        return part[(long long)k * 2 * C + C + c] + rows(k) * d * d;
      });
      dvar = (double)sv / (double)M;
      var = (float)dvar;
    } else if (on) {
      mean = running_mean[c];
      var = running_var[c];
      dvar = (double)var;
    }
    // once per channel, in double and rounded once: the backward's 1 - xhat^2 terms feel every bit of rstd when M is tiny
    const float rstd = (float)(1.0 / sqrt(dvar + (double)eps));
    if (threadIdx.x < 64) {
      smean[cl] = mean;
      srstd[cl] = rstd;
      if (blockIdx.x == 0 && on) {
        if (mean_out) mean_out[c] = mean;
        if (rstd_out) rstd_out[c] = rstd;
        if (TRAIN) {
          running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean;
          running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (var * ((float)M / (float)(M - 1)));
          if (c == 0) *nbt += 1;
        }
      }
    }
    __syncthreads();
  }
  if (!g.on) return;
  const f32x4 mean = *(const f32x4*)(smean + g.q * 4), rstd = *(const f32x4*)(srstd + g.q * 4);
  const f32x4 ga = ld4(gamma + g.c4 * 4), be = ld4(beta + g.c4 * 4);
#pragma unroll 4
  for (long long r = g.r0 + g.slot; r < g.r1; r += 16) {
    f32x4 v = (ld4(x + r * ldx + g.c4 * 4) - mean) * rstd * ga + be;
    if (RESID) v += ld4(resid + r * ldr + g.c4 * 4);
    if (RELU) {
      unsigned m = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        m |= v[i] > 0.f ? 1u << (8 * i) : 0u;
        v[i] = v[i] <= 0.f ? 0.f : v[i];   // (a NaN stays a NaN)
      }
      if (mask) *(unsigned*)(mask + r * C + g.c4 * 4) = m;
    }
    *(f32x4*)(y + r * ldy + g.c4 * 4) = v;
  }
}

// g' = g where the ReLU let the value through (mask NULL: no ReLU)
__device__ __forceinline__ f32x4 masked(f32x4 gv, const unsigned char* mask, long long r, int C, int c4) {
  if (mask) {
    const unsigned m = *(const unsigned*)(mask + r * C + c4 * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) gv[i] = (m >> (8 * i)) & 1u ? gv[i] : 0.f;
  }
  return gv;
}

typedef __attribute__((ext_vector_type(4))) double f64x4;
__device__ __forceinline__ f64x4 widen(f32x4 v) { return f64x4{(double)v[0], (double)v[1], (double)v[2], (double)v[3]}; }
__device__ __forceinline__ f32x4 narrow(f64x4 v) { return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]}; }

// The backward's sums and its x - mean terms run in DOUBLE (the passes stay memory-bound): with a handful of rows per channel all that
// is left of gx is g' (1 - xhat^2) eps-sized, and every fp32 rounding of x - mean, of a product g' (x - mean) or of rstd^2 would show
// in it at the 1e-3 level.  The variance is therefore retaken from x itself, about mean + delta with delta = mean(x - mean) the rounding
// the fp32 mean carries.
//
// ---- backward, launch 1: part[chunk][0..3][c] (doubles) = sum g', sum g' (x - mean), sum (x - mean)^2, sum (x - mean) over the
// chunk's rows --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_bwd_stats_kernel(const float* __restrict__ gr, long long ldg, const float* __restrict__ x,
                                                           long long ldx, const float* __restrict__ mean,
                                                           const unsigned char* __restrict__ mask, double* __restrict__ part, int M, int C) {
  __shared__ f64x4 red[256];
  const Geo g = geo(M, C);
  const f64x4 zero = {0., 0., 0., 0.};
  f64x4 sg = zero, sgx = zero, sxx = zero, sx = zero;
  if (g.on) {
    const f64x4 mu = widen(ld4(mean + g.c4 * 4));
#pragma unroll 4
    for (long long r = g.r0 + g.slot; r < g.r1; r += 16) {
      const f64x4 gv = widen(masked(ld4(gr + r * ldg + g.c4 * 4), mask, r, C, g.c4));
      const f64x4 xc = widen(ld4(x + r * ldx + g.c4 * 4)) - mu;
      sg += gv;
      sgx += gv * xc;
      sxx += xc * xc;
      sx += xc;
    }
  }
  sg = slot_sum(sg, red, g.slot, g.q);
  sgx = slot_sum(sgx, red, g.slot, g.q);
  sxx = slot_sum(sxx, red, g.slot, g.q);
  sx = slot_sum(sx, red, g.slot, g.q);
  if (g.on && g.slot == 0) {
    double* p = part + (long long)blockIdx.x * 4 * C + g.c4 * 4;
    *(f64x4*)p = sg;
    *(f64x4*)(p + C) = sgx;
    *(f64x4*)(p + 2 * C) = sxx;
    *(f64x4*)(p + 3 * C) = sx;
  }
}

// ---- backward, launch 2: gx = gamma rstd (g' - mean(g') - xhat mean(g' xhat))  (eval: gamma rstd g'), evaluated as
// g' - mean(g') - (x - mean - delta) q with q = mean(g' (x - mean - delta)) / (var + eps) per channel; gresid = g', and from the
// workgroups of chunk 0 dbeta = sum g', dgamma = sum g' xhat.  gx / gresid NULL: not wanted (the launch is then one chunk tall). ----
template <bool TRAIN>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ gr, long long ldg, const float* __restrict__ x,
                                                           long long ldx, const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const unsigned char* __restrict__ mask,
                                                           const double* __restrict__ part, float eps, float* __restrict__ gx,
                                                           long long ldgx, float* __restrict__ gresid, long long ldgr,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, int M, int C) {
  __shared__ __attribute__((aligned(32))) double red[256];
  __shared__ __attribute__((aligned(32))) double smg[64], sq[64], smu[64];
  const Geo g = geo(M, C);
  {
    const int cl = threadIdx.x & 63, c = blockIdx.y * 64 + cl;
    const bool on = c < C;
    const int chunks = (M + kChunkRows - 1) / kChunkRows;
    auto row = [&](int j) { return chunk_sum(chunks, red, [&](int k) { return on ? part[((long long)k * 4 + j) * C + c] : 0.; }); };
    const double sg = row(0);
    double sgx = row(1), delta = 0., q = 0.;
    if (TRAIN) {
      const double sxx = row(2);
      delta = row(3) / (double)M;
      sgx -= delta * sg;
      q = sgx / (double)M / (sxx / (double)M - delta * delta + (double)eps);
    }
    if (threadIdx.x < 64) {
      smg[cl] = sg / (double)M;
      sq[cl] = q;
      smu[cl] = (on ? (double)mean[c] : 0.) + delta;
      if (blockIdx.x == 0 && on) {
        if (dbeta) dbeta[c] = (float)sg;
        if (dgamma) dgamma[c] = (float)(sgx * (double)rstd[c]);
      }
    }
    __syncthreads();
  }
  if (!g.on || (!gx && !gresid)) return;
  const f64x4 mg = *(const f64x4*)(smg + g.q * 4), q = *(const f64x4*)(sq + g.q * 4), mu = *(const f64x4*)(smu + g.q * 4);
  const f32x4 gars = ld4(gamma + g.c4 * 4) * ld4(rstd + g.c4 * 4);
#pragma unroll 4
  for (long long r = g.r0 + g.slot; r < g.r1; r += 16) {
    const f32x4 gv = masked(ld4(gr + r * ldg + g.c4 * 4), mask, r, C, g.c4);
    if (gresid) *(f32x4*)(gresid + r * ldgr + g.c4 * 4) = gv;
    if (gx) {
      f32x4 v = gv;
      if (TRAIN) v = narrow(widen(gv) - mg - (widen(ld4(x + r * ldx + g.c4 * 4)) - mu) * q);
      *(f32x4*)(gx + r * ldgx + g.c4 * 4) = gars * v;
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool stride_ok(long long ld, int C) { return ld >= C && ld % 4 == 0; }
bool geometry_ok(int M, int C) { return M > 0 && C >= kMinC && C <= kMaxC && C % 4 == 0; }

}  // namespace

extern "C" {

int mk_train_bn_chunk_rows(void) { return kChunkRows; }

int mk_train_bn_chunks(long long M) { return M > 0 ? (int)((M + kChunkRows - 1) / kChunkRows) : 0; }

long long mk_train_bn_work_floats(long long M, int C) { return M > 0 && C > 0 ? (long long)mk_train_bn_chunks(M) * 8 * C : 0; }

int mk_train_bn_fwd(const float* x, long long ldx, const float* gamma, const float* beta, const float* resid, long long ldr,
                    float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, float* work,
                    float* y, long long ldy, float* mean, float* rstd, unsigned char* mask, int M, int C, int relu, int training,
                    mk_stream_t stream) {
  MK_CHECK_ARG(x && gamma && beta && y && running_mean && running_var, "mk_train_bn_fwd: null pointer");
  MK_CHECK_ARG(geometry_ok(M, C), "mk_train_bn_fwd: bad geometry (M >= 1, C a multiple of 4 in [4, 1024])");
  MK_CHECK_ARG(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(y) && aligned16(resid) && aligned16(mask),
               "mk_train_bn_fwd: x, gamma, beta, resid, y and mask must be 16-byte aligned");
  MK_CHECK_ARG(stride_ok(ldx, C) && stride_ok(ldy, C) && (!resid || stride_ok(ldr, C)),
               "mk_train_bn_fwd: row strides must be multiples of 4 and at least C");
  MK_CHECK_ARG(eps >= 0.f && eps <= 3.4e38f, "mk_train_bn_fwd: eps must be finite and non-negative");
  MK_CHECK_ARG(!training || (M > 1 && work && aligned16(work) && num_batches_tracked && momentum >= 0.f && momentum <= 3.4e38f),
               "mk_train_bn_fwd: batch statistics need M > 1, 16-byte aligned work memory, the batch counter and a finite non-negative momentum");
  MK_CHECK_ARG(!mask || relu, "mk_train_bn_fwd: a mask is written for the ReLU only");
  const dim3 grid((unsigned)mk_train_bn_chunks(M), (unsigned)((C + 63) / 64));
  hipStream_t st = (hipStream_t)stream;
  if (training) {
    hipLaunchKernelGGL(bn_stats_kernel, grid, dim3(256), 0, st, x, ldx, work, M, C);
    MK_CHECK_LAUNCH();
  }
#define MK_BN_APPLY(T, R, S)                                                                                                          \
  hipLaunchKernelGGL((bn_apply_kernel<T, R, S>), grid, dim3(256), 0, st, x, ldx, gamma, beta, resid, ldr, running_mean, running_var, \
                     num_batches_tracked, momentum, eps, work, y, ldy, mean, rstd, mask, M, C)
#define MK_BN_APPLY_T(T)                       \
  do {                                         \
    if (relu && resid) MK_BN_APPLY(T, true, true);   \
    else if (relu) MK_BN_APPLY(T, true, false);      \
    else if (resid) MK_BN_APPLY(T, false, true);     \
    else MK_BN_APPLY(T, false, false);               \
  } while (0)
  if (training) MK_BN_APPLY_T(true);
  else MK_BN_APPLY_T(false);
#undef MK_BN_APPLY_T
#undef MK_BN_APPLY
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_train_bn_bwd(const float* g, long long ldg, const float* x, long long ldx, const float* gamma, const float* mean,
                    const float* rstd, const unsigned char* mask, float* work, float* gx, long long ldgx, float* gresid,
                    long long ldgr, float* dgamma, float* dbeta, float eps, int M, int C, int training, mk_stream_t stream) {
  MK_CHECK_ARG(g && x && gamma && mean && rstd && work, "mk_train_bn_bwd: null pointer");
  MK_CHECK_ARG(geometry_ok(M, C), "mk_train_bn_bwd: bad geometry (M >= 1, C a multiple of 4 in [4, 1024])");
  MK_CHECK_ARG(aligned16(g) && aligned16(x) && aligned16(gamma) && aligned16(mean) && aligned16(rstd) && aligned16(mask) &&
                   aligned16(work) && aligned16(gx) && aligned16(gresid),
               "mk_train_bn_bwd: g, x, gamma, mean, rstd, mask, work, gx and gresid must be 16-byte aligned");
  MK_CHECK_ARG(stride_ok(ldg, C) && stride_ok(ldx, C) && (!gx || stride_ok(ldgx, C)) && (!gresid || stride_ok(ldgr, C)),
               "mk_train_bn_bwd: row strides must be multiples of 4 and at least C");
  MK_CHECK_ARG(!training || M > 1, "mk_train_bn_bwd: batch statistics need M > 1");
  MK_CHECK_ARG(eps >= 0.f && eps <= 3.4e38f, "mk_train_bn_bwd: eps must be finite and non-negative");
  if (!gx && !gresid && !dgamma && !dbeta) return MK_OK;   // nothing wanted: nothing launched
  const dim3 grid((unsigned)mk_train_bn_chunks(M), (unsigned)((C + 63) / 64));
  const dim3 grid2(gx || gresid ? grid.x : 1u, grid.y);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)work;
  hipLaunchKernelGGL(bn_bwd_stats_kernel, grid, dim3(256), 0, st, g, ldg, x, ldx, mean, mask, part, M, C);
  MK_CHECK_LAUNCH();
  if (training)
    hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, grid2, dim3(256), 0, st, g, ldg, x, ldx, gamma, mean, rstd, mask, part, eps, gx,
                       ldgx, gresid, ldgr, dgamma, dbeta, M, C);
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, grid2, dim3(256), 0, st, g, ldg, x, ldx, gamma, mean, rstd, mask, part, eps, gx,
                       ldgx, gresid, ldgr, dgamma, dbeta, M, C);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

}  // extern "C"
