// mickey_amd -- the tails of the four heads for TRAINING (reference mickey_extractor.py:98-124,134-140,172-176,211-216,248-249 and
// utils/extractor_utils.py:6-10 under autograd): the bias-free 1x1 convolution with 1 or 2 outputs and its activation, the per-image
// border-masked softmax of the detector, the descriptors' l2 normalisation, each forward and backward.  All fp32 on the vector ALU:
// a feature map is read once per pass, nothing here has matrix work.  Every sum runs in an order fixed by the shape (lanes, then
// waves, then chunks, each in index order): no atomics, bit-identical from run to run, a row of a forward / input-gradient result
// depends on its own image only.  The inference forms of the same steps are kp_depth_tail_kernel / det_norm_kernel /
// dsc_tail_kernel (mk_heads.hip), which this file leaves as they are.
#include "mk_common.hpp"

namespace {
using namespace mk;

constexpr int kChunkRows = 208;   // rows of one weight-gradient partial (mk_train_headtail_chunk_rows): 13 rows for each of a workgroup's
                                  // sixteen 16-lane groups; 150 workgroups at 8 images of 38 x 51
constexpr int kMaxC = 256;

__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}
// sum over the workgroup in lane, then wave order; every thread gets the result.  sred: one float per wave
__device__ __forceinline__ float block_sum(float v, float* sred) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_sum(v);
  __syncthreads();   // (the previous use of sred is over)
  if (lane == 0) sred[wave] = v;
  __syncthreads();
  float tot = 0.f;
  for (int i = 0; i < nw; ++i) tot += sred[i];
  return tot;
}

// ---- 1x1 tail forward: 16 lanes per pixel row (16 bytes per lane and step), 16 rows per workgroup --------------------------------
template <int COUT>
__global__ __launch_bounds__(256) void tail_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                       float* __restrict__ out, long long rows, int h, int wd, int C, int act,
                                                       float scale, int border) {
  const int l16 = threadIdx.x & 15;
  const long long row = blockIdx.x * 16LL + (threadIdx.x >> 4);
  if (row >= rows) return;   // a whole 16-lane group leaves together
  float a[COUT];
#pragma unroll
  for (int o = 0; o < COUT; ++o) a[o] = 0.f;
  for (int c4 = l16; c4 < (C >> 2); c4 += 16) {
    const f32x4 f = *(const f32x4*)(feat + row * C + c4 * 4);
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
      const f32x4 ww = *(const f32x4*)(w + o * C + c4 * 4);
      a[o] += f[0] * ww[0] + f[1] * ww[1] + f[2] * ww[2] + f[3] * ww[3];
    }
  }
#pragma unroll
  for (int o = 0; o < COUT; ++o) a[o] = group16_sum(a[o]);
  if (l16 < COUT) {
    const int n = h * wd;
    const long long img = row / n;
    const int p = (int)(row - img * n);
    const int y = p / wd, x = p - y * wd;
    const bool in = y >= border && y < h - border && x >= border && x < wd - border;
    float z = a[0];
#pragma unroll
    for (int o = 1; o < COUT; ++o) z = l16 == o ? a[o] : z;
    float v = z;                                       // MK_TAIL_IDENTITY, MK_TAIL_SOFTMAX (the raw logit)
    if (act == MK_TAIL_SIGMOID) v = scale * sigmoidf(z);
    if (act == MK_TAIL_MASKED_SIGMOID) v = in ? sigmoidf(z) : 0.f;
    out[(img * COUT + l16) * n + p] = v;
  }
}

// detector softmax of one image, in place on its logits: one workgroup per image, a thread keeps its own pixels through the
// three passes (mean, masked exponentials, division)
__global__ __launch_bounds__(1024) void tail_softmax_kernel(float* __restrict__ zy, int h, int wd, int border, float temperature,
                                                            float eps) {
  __shared__ float sred[16];
  const int n = h * wd;
  float* z = zy + (long long)blockIdx.x * n;
  float a = 0.f;
  for (int p = threadIdx.x; p < n; p += blockDim.x) a += z[p];
  const float mean = block_sum(a, sred) / (float)n + eps;
  float es = 0.f;
  for (int p = threadIdx.x; p < n; p += blockDim.x) {
    const int y = p / wd, x = p - y * wd;
    const bool in = y >= border && y < h - border && x >= border && x < wd - border;
    const float e = in ? expf((z[p] - mean) / temperature) : 0.f;
    z[p] = e;
    es += e;
  }
  const float inv = 1.0f / (block_sum(es, sred) + eps);
  for (int p = threadIdx.x; p < n; p += blockDim.x) z[p] = z[p] * inv;
}

// ---- 1x1 tail backward ------------------------------------------------------------------------------------------------------
// softmax only: dot[img] = sum_p g_p y_p, one workgroup per image
__global__ __launch_bounds__(256) void tail_dot_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                       float* __restrict__ dot, int n) {
  __shared__ float sred[4];
  const long long base = (long long)blockIdx.x * n;
  float a = 0.f;
  for (int p = threadIdx.x; p < n; p += blockDim.x) a += g[base + p] * y[base + p];
  a = block_sum(a, sred);
  if (threadIdx.x == 0) dot[blockIdx.x] = a;
}

// the row pass: one workgroup per chunk of kChunkRows rows; 16 lanes per row as in the forward, a 16-lane group walks rows
// grp, grp + 16, ... of the chunk.  GF: gfeat rows are written; GW: the chunk's partial of gw goes to part[chunk][COUT][C]
// (the 16 groups' sums added in group order).
template <int COUT, bool GF, bool GW>
__global__ __launch_bounds__(256) void tail_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                       const float* __restrict__ feat, const float* __restrict__ w,
                                                       const float* __restrict__ dot, float* __restrict__ gfeat,
                                                       float* __restrict__ part, long long rows, int n, int C, int act, float scale,
                                                       float temperature) {
  __shared__ __attribute__((aligned(16))) float red[GW ? 16 * COUT * kMaxC : 4];
  const int l16 = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const long long r0 = (long long)blockIdx.x * kChunkRows;
  const long long r1 = r0 + kChunkRows < rows ? r0 + kChunkRows : rows;
  const int C4 = C >> 2;
  f32x4 wv[COUT][4], acc[COUT][4];
#pragma unroll
  for (int o = 0; o < COUT; ++o)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[o][k] = f32x4{0.f, 0.f, 0.f, 0.f};
      wv[o][k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (GF && l16 + 16 * k < C4) wv[o][k] = *(const f32x4*)(w + o * C + (l16 + 16 * k) * 4);
    }
  for (long long row = r0 + grp; row < r1; row += 16) {
    const long long img = row / n;
    const int p = (int)(row - img * n);
    float gz[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
      const long long i = (img * COUT + o) * n + p;
      const float gg = g[i];
      gz[o] = gg;                                                         // MK_TAIL_IDENTITY
      if (act == MK_TAIL_SIGMOID || act == MK_TAIL_MASKED_SIGMOID) {      // (a masked pixel has y == 0)
        const float yy = y[i];
        gz[o] = gg * yy * (1.0f - yy / scale);
      } else if (act == MK_TAIL_SOFTMAX) {
        gz[o] = (y[i] / temperature) * (gg - dot[img]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c4 = l16 + 16 * k;
      if (c4 < C4) {
        if (GW) {
          const f32x4 f = *(const f32x4*)(feat + row * C + c4 * 4);
#pragma unroll
          for (int o = 0; o < COUT; ++o) acc[o][k] += gz[o] * f;
        }
        if (GF) {
          f32x4 v = gz[0] * wv[0][k];
#pragma unroll
          for (int o = 1; o < COUT; ++o) v += gz[o] * wv[o][k];
          *(f32x4*)(gfeat + row * C + c4 * 4) = v;
        }
      }
    }
  }
  if (GW) {
#pragma unroll
    for (int o = 0; o < COUT; ++o)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (l16 + 16 * k < C4) *(f32x4*)(red + (grp * COUT + o) * kMaxC + (l16 + 16 * k) * 4) = acc[o][k];
    __syncthreads();
    for (int i = threadIdx.x; i < COUT * C; i += 256) {
      const int o = i / C, c = i - o * C;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) s += red[(j * COUT + o) * kMaxC + c];
      part[(long long)blockIdx.x * COUT * C + i] = s;
    }
  }
}

// gw[i] = sum over the chunks of part[chunk][i]: wave s of 16 adds the s-th sixteenth of the chunks in chunk order, the sixteen sums
// are then added in wave order (a grouping fixed by the chunk count); a workgroup owns 64 elements, a lane one of them
__global__ __launch_bounds__(1024) void tail_add_kernel(const float* __restrict__ part, float* __restrict__ gw, int chunks, int nw) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const int per = (chunks + 15) >> 4;
  const int c0 = wave * per, c1 = c0 + per < chunks ? c0 + per : chunks;
  float s = 0.f;
  if (i < nw) {
#pragma unroll 8
    for (int c = c0; c < c1; ++c) s += part[(long long)c * nw + i];
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && i < nw) {
    float t = red[0][lane];
#pragma unroll
    for (int j = 1; j < 16; ++j) t += red[j][lane];
    gw[i] = t;
  }
}

// ---- descriptors: l2 normalisation over channels, [pixel, C] rows <-> [C, pixel] planes; workgroup = 64 pixels of one image ------
// forward: the arithmetic of dsc_tail_kernel (a wave per pixel, lane-strided sum of squares, xor butterfly), channels in slabs of
// 128 so that the transposing tile stays 33 KiB for every width
__global__ __launch_bounds__(256) void desc_fwd_kernel(const float* __restrict__ x, float* __restrict__ yout,
                                                       float* __restrict__ rnorm, int n, int C, float eps) {
  __shared__ float tile[128 * 65];
  __shared__ float rn[64];
  const int img = blockIdx.y, p0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int pp = wave; pp < 64; pp += 4) {
    const int p = p0 + pp;
    if (p >= n) break;
    const float* f = x + ((long long)img * n + p) * C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) q += f[c] * f[c];
    q = wave_sum(q);
    const float sc = 1.0f / sqrtf(q + eps);
    if (lane == 0) {
      rn[pp] = sc;
      if (rnorm) rnorm[(long long)img * n + p] = sc;
    }
  }
  __syncthreads();
  for (int c0 = 0; c0 < C; c0 += 128) {
    const int cw = C - c0 < 128 ? C - c0 : 128;
    for (int pp = wave; pp < 64; pp += 4) {
      const int p = p0 + pp;
      if (p >= n) break;
      const float* f = x + ((long long)img * n + p) * C + c0;
      const float sc = rn[pp];
      for (int c = lane; c < cw; c += 64) tile[c * 65 + pp] = f[c] * sc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cw * 64; i += 256) {
      const int c = i >> 6, pp = i & 63;
      if (p0 + pp < n) yout[((long long)img * C + c0 + c) * n + p0 + pp] = tile[c * 65 + pp];
    }
    __syncthreads();
  }
}

// backward: gx[p, c] = r_p (g[c, p] - y[c, p] s_p),  s_p = sum_c g[c, p] y[c, p]: lanes along pixels for the plane reads (wave w sums
// channels w, w + 4, ...; the four partial sums added in wave order), lanes along channels for the row writes
__global__ __launch_bounds__(256) void desc_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                       const float* __restrict__ rnorm, float* __restrict__ gx, int n, int C) {
  __shared__ float tile[128 * 65];
  __shared__ float sp[4][64];
  const int img = blockIdx.y, p0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = p0 + lane;
  const bool ok = p < n;
  const long long plane0 = (long long)img * C * n + p;
  float s = 0.f;
  if (ok)
    for (int c = wave; c < C; c += 4) s += g[plane0 + (long long)c * n] * y[plane0 + (long long)c * n];
  sp[wave][lane] = s;
  __syncthreads();
  s = ((sp[0][lane] + sp[1][lane]) + sp[2][lane]) + sp[3][lane];
  const float r = ok ? rnorm[(long long)img * n + p] : 0.f;
  for (int c0 = 0; c0 < C; c0 += 128) {
    const int cw = C - c0 < 128 ? C - c0 : 128;
    if (ok)
      for (int c = wave; c < cw; c += 4) {
        const long long i = plane0 + (long long)(c0 + c) * n;
        tile[c * 65 + lane] = r * (g[i] - y[i] * s);
      }
    __syncthreads();
    for (int pp = wave; pp < 64; pp += 4) {
      if (p0 + pp >= n) break;
      float* o = gx + ((long long)img * n + p0 + pp) * C + c0;
      for (int c = lane; c < cw; c += 64) o[c] = tile[c * 65 + pp];
    }
    __syncthreads();
  }
}

bool width_ok(int C) { return C >= 4 && C <= kMaxC && C % 4 == 0; }
bool act_ok(int act) { return act >= MK_TAIL_IDENTITY && act <= MK_TAIL_SOFTMAX; }

}  // namespace

extern "C" {

int mk_train_headtail_chunk_rows(void) { return kChunkRows; }

int mk_train_headtail_chunks(long long rows) { return rows > 0 ? (int)((rows + kChunkRows - 1) / kChunkRows) : 0; }

int mk_train_headtail_fwd(const float* feat, const float* w, float* out, int nimg, int h, int wd, int C, int Cout, int act,
                          float scale, int border, float temperature, float eps, mk_stream_t stream) {
  MK_CHECK_ARG(feat && w && out, "mk_train_headtail_fwd: null pointer");
  MK_CHECK_ARG((((uintptr_t)feat | (uintptr_t)w) & 15) == 0, "mk_train_headtail_fwd: feat and w must be 16-byte aligned");
  MK_CHECK_ARG(nimg > 0 && h > 0 && wd > 0 && (long long)h * wd <= 0x7fffffffLL && (long long)nimg * h * wd <= 0x7fffffffLL * 16 &&
                   width_ok(C) && (Cout == 1 || Cout == 2) && act_ok(act) && border >= 0,
               "mk_train_headtail_fwd: bad geometry (C a multiple of 4 in [4, 256], 1 or 2 outputs)");
  MK_CHECK_ARG(act < MK_TAIL_MASKED_SIGMOID || Cout == 1, "mk_train_headtail_fwd: the detector activations take one output");
  MK_CHECK_ARG(act != MK_TAIL_SIGMOID || scale > 0.f, "mk_train_headtail_fwd: scale must be positive");
  MK_CHECK_ARG(act != MK_TAIL_SOFTMAX || (temperature > 0.f && temperature <= 3.4e38f && eps >= 0.f && eps <= 3.4e38f),
               "mk_train_headtail_fwd: temperature must be finite and positive, eps finite and non-negative");
  const long long rows = (long long)nimg * h * wd;
  const dim3 grid((unsigned)((rows + 15) / 16));
  hipStream_t st = (hipStream_t)stream;
  if (Cout == 1)
    hipLaunchKernelGGL(tail_fwd_kernel<1>, grid, dim3(256), 0, st, feat, w, out, rows, h, wd, C, act, scale, border);
  else
    hipLaunchKernelGGL(tail_fwd_kernel<2>, grid, dim3(256), 0, st, feat, w, out, rows, h, wd, C, act, scale, border);
  MK_CHECK_LAUNCH();
  if (act == MK_TAIL_SOFTMAX) {
    hipLaunchKernelGGL(tail_softmax_kernel, dim3(nimg), dim3(1024), 0, st, out, h, wd, border, temperature, eps);
    MK_CHECK_LAUNCH();
  }
  return MK_OK;
}

int mk_train_headtail_bwd(const float* g, const float* y, const float* feat, const float* w, float* dot, float* gfeat, float* part,
                          float* gw, int nimg, int n, int C, int Cout, int act, float scale, float temperature,
                          mk_stream_t stream) {
  MK_CHECK_ARG(g, "mk_train_headtail_bwd: null gradient");
  MK_CHECK_ARG(nimg > 0 && n > 0 && (long long)nimg * n <= 0x7fffffffLL * 16 && width_ok(C) && (Cout == 1 || Cout == 2) && act_ok(act),
               "mk_train_headtail_bwd: bad geometry (C a multiple of 4 in [4, 256], 1 or 2 outputs)");
  MK_CHECK_ARG(act < MK_TAIL_MASKED_SIGMOID || Cout == 1, "mk_train_headtail_bwd: the detector activations take one output");
  MK_CHECK_ARG(act == MK_TAIL_IDENTITY || y, "mk_train_headtail_bwd: the activation's gradient needs the saved output y");
  MK_CHECK_ARG(act != MK_TAIL_SIGMOID || scale > 0.f, "mk_train_headtail_bwd: scale must be positive");
  MK_CHECK_ARG(act != MK_TAIL_SOFTMAX || (dot && temperature > 0.f && temperature <= 3.4e38f),
               "mk_train_headtail_bwd: the softmax needs dot [nimg] and a finite positive temperature");
  MK_CHECK_ARG(!gfeat || (w && (((uintptr_t)gfeat | (uintptr_t)w) & 15) == 0), "mk_train_headtail_bwd: gfeat needs w, both 16-byte aligned");
  MK_CHECK_ARG(!gw || (feat && part && (((uintptr_t)feat | (uintptr_t)part) & 15) == 0),
               "mk_train_headtail_bwd: gw needs feat and part, both 16-byte aligned");
  if (!gfeat && !gw) return MK_OK;   // nothing wanted: nothing launched
  const long long rows = (long long)nimg * n;
  const int chunks = mk_train_headtail_chunks(rows);
  hipStream_t st = (hipStream_t)stream;
  if (act == MK_TAIL_SOFTMAX) {
    hipLaunchKernelGGL(tail_dot_kernel, dim3(nimg), dim3(256), 0, st, g, y, dot, n);
    MK_CHECK_LAUNCH();
  }
  if (act == MK_TAIL_MASKED_SIGMOID) scale = 1.0f;
#define MK_TAIL_BWD(CO, GF, GW)                                                                                                  \
  hipLaunchKernelGGL((tail_bwd_kernel<CO, GF, GW>), dim3(chunks), dim3(256), 0, st, g, y, feat, w, dot, gfeat, part, rows, n, C, \
                     act, scale, temperature)
  if (Cout == 1) {
    if (gfeat && gw) MK_TAIL_BWD(1, true, true);
    else if (gfeat) MK_TAIL_BWD(1, true, false);
    else MK_TAIL_BWD(1, false, true);
  } else {
    if (gfeat && gw) MK_TAIL_BWD(2, true, true);
    else if (gfeat) MK_TAIL_BWD(2, true, false);
    else MK_TAIL_BWD(2, false, true);
  }
#undef MK_TAIL_BWD
  MK_CHECK_LAUNCH();
  if (gw) {
    const int nw = Cout * C;
    hipLaunchKernelGGL(tail_add_kernel, dim3((nw + 63) / 64), dim3(1024), 0, st, part, gw, chunks, nw);
    MK_CHECK_LAUNCH();
  }
  return MK_OK;
}

int mk_train_desc_l2norm_fwd(const float* x, float* y, float* rnorm, int nimg, int n, int C, float eps, mk_stream_t stream) {
  MK_CHECK_ARG(x && y, "mk_train_desc_l2norm_fwd: null pointer");
  MK_CHECK_ARG(nimg > 0 && nimg <= 65535 && n > 0 && width_ok(C) && eps >= 0.f && eps <= 3.4e38f,
               "mk_train_desc_l2norm_fwd: bad geometry (C a multiple of 4 in [4, 256], at most 65535 images, eps finite and >= 0)");
  hipLaunchKernelGGL(desc_fwd_kernel, dim3((n + 63) / 64, nimg), dim3(256), 0, (hipStream_t)stream, x, y, rnorm, n, C, eps);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_train_desc_l2norm_bwd(const float* g, const float* y, const float* rnorm, float* gx, int nimg, int n, int C,
                             mk_stream_t stream) {
  MK_CHECK_ARG(g && y && rnorm && gx, "mk_train_desc_l2norm_bwd: null pointer");
  MK_CHECK_ARG(nimg > 0 && nimg <= 65535 && n > 0 && width_ok(C),
               "mk_train_desc_l2norm_bwd: bad geometry (C a multiple of 4 in [4, 256], at most 65535 images)");
  hipLaunchKernelGGL(desc_bwd_kernel, dim3((n + 63) / 64, nimg), dim3(256), 0, (hipStream_t)stream, g, y, rnorm, gx, n, C);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

}  // extern "C"
