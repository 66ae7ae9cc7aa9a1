// mickey_amd -- row-wise kernels of the encoder: LayerNorm, patch im2col, CLS row.  All HBM-bound:
// one wave per row, 16-byte loads/stores, wave64 shuffle reductions, values held in registers
// between the statistics and the normalisation (single read of x).
#include "mk_common.hpp"
#include "mk_gemm_common.hpp"   // quad_stats / row16_sum: the one summation order of the row statistics

#include <stdarg.h>
#include <stdio.h>

namespace {
using namespace mk;

// out_is_f32 == 2: the row goes out as the (hi, lo) fp16 operand planes of the split-operand head kernels
// (mk_conv3x3_split / mk_gemm_grouped_split): y * scale = hi + lo, saturating at fp16's largest finite value
__device__ __forceinline__ void store_planes(void* hi, void* lo, long long o, const f32x4& y, float scale, int* sat_flag) {
  f16x4 oh, ol;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float sv = sat16(y[e] * scale, sat_flag);
    oh[e] = (_Float16)sv;
    ol[e] = (_Float16)(sv - (float)oh[e]);
  }
  *(f16x4*)((_Float16*)hi + o) = oh;
  if (lo) *(f16x4*)((_Float16*)lo + o) = ol;   // lo == nullptr: the row rounded to fp16 (what an fp16 LayerNorm outputs)
}

constexpr int LN_MAXV = 8;  // float4 per lane -> D <= 2048 (instantiated for 4 as well: D <= 1024 needs half the registers)

constexpr int LN_RPW = 4;   // rows per wave: the loads of row r+1 are in flight while row r is reduced and stored
                            // (a third buffer / 6 rows per wave measured 7 % slower in the forward)

// ---- the per-row arithmetic: ONE statement of it for every kernel that has to write the same bits (mk_layernorm and
// mk_layernorm_nchw are compared with torch.equal): same summation order, same contraction of the normalisation ----
// wide form: a row is a wave, lane l holds columns (i * 64 + l) * 4 ..
template <int MAXV>
__device__ __forceinline__ void ln_row_stats(const f32x4 (&cur)[MAXV], int lane, int D, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) s += (cur[i][0] + cur[i][1]) + (cur[i][2] + cur[i][3]);
  }
  mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = cur[i][e] - mean;
        q += d * d;
      }
    }
  }
  rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
}

// narrow form (D <= 128): a row is 32 lanes x 4 floats, the sums run over a half wave; v is zero in lanes without a column
__device__ __forceinline__ float ln_half_sum(float a) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  return a;
}
// d: the centred values v - mean (zero in lanes without a column), which the caller normalises with ln_scale
__device__ __forceinline__ void ln_narrow_stats(const f32x4& v, bool cok, int D, float eps, float& mean, float& rstd, f32x4& d) {
  mean = ln_half_sum((v[0] + v[1]) + (v[2] + v[3])) / (float)D;
  d = f32x4{0.f, 0.f, 0.f, 0.f};
  if (cok) d = v - mean;
  rstd = 1.0f / sqrtf(ln_half_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) / (float)D + eps);
}

// one element of the normalised row, both forms: from the centred value, or from x (the same subtraction, then the same rest)
__device__ __forceinline__ float ln_scale(float d, float rstd, float w, float b) { return d * rstd * w + b; }
__device__ __forceinline__ float ln_norm(float x, float mean, float rstd, float w, float b) { return ln_scale(x - mean, rstd, w, b); }

template <typename T, int MAXV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                        const float* __restrict__ b, float eps, void* out, int ldo,
                                                        int out_is_f32, float* resid, int ldr, int rows_out, int D,
                                                        int rows_per_img, int skip, int wgroup_rows, int bord_h, int bord_w,
                                                        int bord_m, void* out_lo, float plane_scale, int* sat_flag) {
  const int lane = threadIdx.x & 63;
  const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * LN_RPW;
  if (r0 >= rows_out) return;
  const int rpo = rows_per_img - skip;
  f32x4 v[2][MAXV];
  auto load_row = [&](int r, f32x4 (&dst)[MAXV]) {
    const long long rin = (long long)(r / rpo) * rows_per_img + skip + (r % rpo);
    const float* xr = x + rin * ldx;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < D) dst[i] = __builtin_nontemporal_load((const f32x4*)(xr + c));   // streamed once: do not displace the weights in L2
    }
  };
  load_row(r0, v[0]);
  // weight / bias shared by all rows (the encoder's case): once per wave, not once per row -- the compiler cannot hoist
  // them itself because `out` may alias them for all it knows (8 of the 12 load instructions per row)
  f32x4 wreg[MAXV], breg[MAXV];
  const bool shared_wb = wgroup_rows <= 0;
  if (shared_wb) {
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < D) {
        wreg[i] = *(const f32x4*)(w + c);
        breg[i] = *(const f32x4*)(b + c);
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < LN_RPW; ++rr) {
    const int r = r0 + rr;
    if (r >= rows_out) break;
    if (rr + 1 < LN_RPW && r + 1 < rows_out) load_row(r + 1, v[(rr + 1) & 1]);
    f32x4 (&cur)[MAXV] = v[rr & 1];
    // bordered output (feeds a 3x3 conv, mk_common.hpp): buffers of bord_m pixels each, one behind the other
    long long ro = r;
    if (bord_h > 0) {
      const int gb = r / bord_m, m = r - gb * bord_m;
      ro = gb * bordered_rows(bord_m / (bord_h * bord_w), bord_h, bord_w) + bordered_row(m, bord_h, bord_w);
    }
    const float* wr = w;
    const float* br = b;
    if (wgroup_rows > 0) {  // one (w, b) per block of wgroup_rows output rows
      wr += (long long)(r / wgroup_rows) * D;
      br += (long long)(r / wgroup_rows) * D;
    }
    float mean, rstd;
    ln_row_stats<MAXV>(cur, lane, D, eps, mean, rstd);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < D) {
        const f32x4 ww = shared_wb ? wreg[i] : *(const f32x4*)(wr + c), bb = shared_wb ? breg[i] : *(const f32x4*)(br + c);
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = ln_norm(cur[i][e], mean, rstd, ww[e], bb[e]);
        if (resid) {
          float* rp = resid + (long long)r * ldr + c;
          y += *(const f32x4*)rp;
          *(f32x4*)rp = y;
        }
        if (out) {
          if (out_is_f32 == 2) {
            store_planes(out, out_lo, ro * ldo + c, y, plane_scale, sat_flag);
          } else if (out_is_f32) {
            *(f32x4*)((float*)out + ro * ldo + c) = y;
          } else {
            typename Lp<T>::V4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (T)y[e];
            *(typename Lp<T>::V4*)((T*)out + ro * ldo + c) = o;
          }
        }
      }
    }
  }
}

// Narrow rows (D <= 128: the 128-channel LayerNorms of the heads' attention layers, 6 of the 7 stand-alone LayerNorms of a
// forward).  In the kernel above such a row occupies half a wave and a wave has one 512-byte row in flight: 2.2 TB/s.
// Here a row is 32 lanes x 4 floats, a wave works on TWO rows at a time and requests all 8 rows it owns (4 trips) before
// it reduces the first.  Same arithmetic per row (sum, then squares about the mean, both over the row's 32 lanes).
constexpr int LNN_TRIPS = 4;   // row pairs per wave
template <typename T>
__global__ __launch_bounds__(256) void layernorm_narrow_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                               const float* __restrict__ b, float eps, void* out, int ldo,
                                                               int out_is_f32, float* resid, int ldr, int rows_out, int D,
                                                               int rows_per_img, int skip, int wgroup_rows, int bord_h,
                                                               int bord_w, int bord_m, void* out_lo, float plane_scale, int* sat_flag) {
  const int lane = threadIdx.x & 63, half = lane >> 5, c = (lane & 31) * 4;
  const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * (2 * LNN_TRIPS);
  if (r0 >= rows_out) return;
  const bool cok = c < D;
  const int rpo = rows_per_img - skip;
  f32x4 v[LNN_TRIPS];
#pragma unroll
  for (int t = 0; t < LNN_TRIPS; ++t) {
    const int r = r0 + 2 * t + half;
    v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (r < rows_out && cok) {
      const long long rin = (long long)(r / rpo) * rows_per_img + skip + (r % rpo);
      v[t] = __builtin_nontemporal_load((const f32x4*)(x + rin * ldx + c));
    }
  }
#pragma unroll
  for (int t = 0; t < LNN_TRIPS; ++t) {
    const int r = r0 + 2 * t + half;
    const bool ok = r < rows_out && cok;
    float mean, rstd;
    f32x4 d;
    ln_narrow_stats(v[t], cok, D, eps, mean, rstd, d);
    if (!ok) continue;
    const long long wo = wgroup_rows > 0 ? (long long)(r / wgroup_rows) * D : 0;
    const f32x4 ww = *(const f32x4*)(w + wo + c), bb = *(const f32x4*)(b + wo + c);
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = ln_scale(d[e], rstd, ww[e], bb[e]);
    if (resid) {
      float* rp = resid + (long long)r * ldr + c;
      y += *(const f32x4*)rp;
      *(f32x4*)rp = y;
    }
    if (out) {
      long long ro = r;
      if (bord_h > 0) {
        const int gb = r / bord_m, m = r - gb * bord_m;
        ro = gb * bordered_rows(bord_m / (bord_h * bord_w), bord_h, bord_w) + bordered_row(m, bord_h, bord_w);
      }
      if (out_is_f32 == 2) {
        store_planes(out, out_lo, ro * ldo + c, y, plane_scale, sat_flag);
      } else if (out_is_f32) {
        *(f32x4*)((float*)out + ro * ldo + c) = y;
      } else {
        typename Lp<T>::V4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (T)y[e];
        *(typename Lp<T>::V4*)((T*)out + ro * ldo + c) = o;
      }
    }
  }
}

// The final norm written CHANNEL-major (mickey_hip.h, mk_layernorm_nchw): out[img][c][p], fp32.  A workgroup owns 64 pixels
// of one image -- the 256-byte store runs -- and every channel of them.
//   pass 1  the row statistics, exactly as the kernels above form them (ln_row_stats / ln_narrow_stats: a row per wave, or per
//           half wave for D <= 128); (mean, rstd) of the 64 rows stay in LDS.  Plain loads: the rows are wanted again.
//   pass 2  128 channels at a time: the rows are read a second time (by the workgroup that just read them: out of the cache
//           hierarchy, not HBM; streamed this time), normalised with ln_norm, written TRANSPOSED into a [128][64 + 1] LDS tile,
//           and the tile leaves as one 64-pixel run per channel, a wave per run.
// LDS banks (32 for every ds_write and for ds_read_b32, lanes conflict within a 32-lane half): a half wave of the transposing
// write holds 16 channel quads x 2 pixels, dword address (4 cq + e) * 65 + p = 4 cq + e + p (mod 32): cq and cq + 8 share a
// bank, nothing else does -- 2-way, which a ds_write_b32 hides behind its own data transfer; the read-out's half wave reads 32
// consecutive dwords of one tile row.  33.8 KB per workgroup: four workgroups per CU.
constexpr int NCHW_TP = 64;            // pixels per workgroup
constexpr int NCHW_CC = 128;           // channels per LDS round
constexpr int NCHW_LD = NCHW_TP + 1;   // tile row pitch in dwords (odd: see above)
template <int MAXV, bool NARROW>
__global__ __launch_bounds__(256) void layernorm_nchw_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                             const float* __restrict__ b, float eps, float* __restrict__ out,
                                                             int npix, int D, int rows_per_img, int skip, int tiles, int round_fp16) {
  __shared__ float tile[NCHW_CC * NCHW_LD];
  __shared__ float s_mean[NCHW_TP], s_rstd[NCHW_TP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x / tiles, p0 = (blockIdx.x - img * tiles) * NCHW_TP;
  const int np = min(NCHW_TP, npix - p0);   // pixels of this tile
  const float* xt = x + ((long long)img * rows_per_img + skip + p0) * ldx;
  if constexpr (NARROW) {
    constexpr int TRIPS = NCHW_TP / 8;   // row pairs per wave, LNN_TRIPS of them in flight at a time
    const int half = lane >> 5, c = (lane & 31) * 4;
    const bool cok = c < D;
#pragma unroll 1
    for (int t0 = 0; t0 < TRIPS; t0 += LNN_TRIPS) {
      f32x4 v[LNN_TRIPS];
#pragma unroll
      for (int t = 0; t < LNN_TRIPS; ++t) {
        const int p = (wave * TRIPS + t0 + t) * 2 + half;
        v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p < np && cok) v[t] = *(const f32x4*)(xt + (long long)p * ldx + c);
      }
#pragma unroll
      for (int t = 0; t < LNN_TRIPS; ++t) {
        const int p = (wave * TRIPS + t0 + t) * 2 + half;
        float mean, rstd;
        f32x4 d;
        ln_narrow_stats(v[t], cok, D, eps, mean, rstd, d);
        if ((lane & 31) == 0 && p < np) {
          s_mean[p] = mean;
          s_rstd[p] = rstd;
        }
      }
    }
  } else {
    constexpr int RPW = NCHW_TP / 4;   // rows per wave: p = rr * 4 + wave, the next row in flight while this one is reduced
    f32x4 v[2][MAXV];
    auto load_row = [&](int p, f32x4 (&dst)[MAXV]) {
      const float* xr = xt + (long long)p * ldx;
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < D) dst[i] = *(const f32x4*)(xr + c);
      }
    };
    auto step = [&](int p, f32x4 (&cur)[MAXV], f32x4 (&nxt)[MAXV]) {   // p is wave-uniform: the shuffles see whole waves
      if (p >= np) return;
      if (p + 4 < np) load_row(p + 4, nxt);
      float mean, rstd;
      ln_row_stats<MAXV>(cur, lane, D, eps, mean, rstd);
      if (lane == 0) {
        s_mean[p] = mean;
        s_rstd[p] = rstd;
      }
    };
    if (wave < np) load_row(wave, v[0]);
#pragma unroll 1
    for (int rr = 0; rr < RPW; rr += 2) {   // (rolled: unrolled, the compiler hoists all 16 rows' loads and the kernel needs 300 registers)
      step(rr * 4 + wave, v[0], v[1]);
      step(rr * 4 + 4 + wave, v[1], v[0]);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int c0 = 0; c0 < D; c0 += NCHW_CC) {
#pragma unroll 1
    for (int hb = 0; hb < NCHW_CC / 64; ++hb) {   // 64 channels x 64 pixels per trip: 16 quads x 16 pixels per step
      const int cl = hb * 64 + (tid & 15) * 4, c = c0 + cl;
      if (c < D) {
        const f32x4 ww = *(const f32x4*)(w + c), bb = *(const f32x4*)(b + c);
        f32x4 xv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = j * 16 + (tid >> 4);
          if (p < np) xv[j] = __builtin_nontemporal_load((const f32x4*)(xt + (long long)p * ldx + c));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = j * 16 + (tid >> 4);
          if (p < np) {
            const float mean = s_mean[p], rstd = s_rstd[p];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float y = ln_norm(xv[j][e], mean, rstd, ww[e], bb[e]);
              if (round_fp16) {
                // the fp32 value is rounded FIRST (as mk_layernorm writes it), then to fp16: left to itself hipcc fuses ln_norm's
                // fma and the conversion into one v_fma_mixlo_f16 -- a single rounding, which is not tensor.half() of the fp32 value
                asm volatile("" : "+v"(y));
                y = (float)(_Float16)y;   // nearest even, overflow to inf, NaN stays NaN
              }
              tile[(cl + e) * NCHW_LD + p] = y;
            }
          }
        }
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int it = 0; it < NCHW_CC * NCHW_TP / 256; ++it) {
      const int idx = it * 256 + tid;
      const int cl = idx >> 6, p = idx & (NCHW_TP - 1);   // a wave = one channel's run of 64 pixels
      const int c = c0 + cl;
      if (p < np && c < D) out[((long long)img * D + c) * npix + p0 + p] = tile[cl * NCHW_LD + p];
    }
    __syncthreads();
  }
}

// one thread per 4 output columns (k = ch*196 + dy*14 + dx); rows = patches
template <typename T>
__global__ __launch_bounds__(256) void im2col14_kernel(const float* __restrict__ img, long long stride_img,
                                                       long long stride_ch, int stride_row, int nimg, int gh, int gw,
                                                       T* __restrict__ out, int ldo) {
  const int cols4 = ldo >> 2;
  const long long total = (long long)nimg * gh * gw * cols4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % cols4);
    const long long m = i / cols4;
    const int pc = (int)(m % gw);
    const int pr = (int)((m / gw) % gh);
    const int im = (int)(m / ((long long)gw * gh));
    typename Lp<T>::V4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = c4 * 4 + e;
      float v = 0.f;
      if (k < 588) {
        const int ch = k / 196, rem = k - ch * 196, dy = rem / 14, dx = rem - dy * 14;
        v = img[im * stride_img + ch * stride_ch + (long long)(pr * 14 + dy) * stride_row + pc * 14 + dx];
      }
      o[e] = (T)v;
    }
    *(typename Lp<T>::V4*)(out + m * ldo + c4 * 4) = o;
  }
}

__global__ void cls_kernel(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ x, int nimg,
                           int ntok, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nimg * D) return;
  const int im = i / D, c = i - im * D;
  x[(long long)im * ntok * D + c] = cls[c] + pos[c];
}

// CLS row of the split residual stream (hi / lo planes) with its slot statistics: one wave per image; lane l owns columns
// c = l, l + 64, ...: slot c / 64 of the row statistics is a plain wave sum.
template <typename T>
__global__ __launch_bounds__(64) void cls_ln_kernel(const float* __restrict__ cls, const float* __restrict__ pos, T* __restrict__ xh,
                                                    T* __restrict__ xl, float* __restrict__ stats, int ntok, int D) {
  const int im = blockIdx.x, lane = threadIdx.x;
  const long long row = (long long)im * ntok;
  for (int c0 = 0; c0 < D; c0 += 64) {
    const float v = cls[c0 + lane] + pos[c0 + lane];
    const T h = (T)v;
    xh[row * D + c0 + lane] = h;
    xl[row * D + c0 + lane] = (T)(v - (float)h);
    const float s = mk::wave_sum(v), q = mk::wave_sum(v * v);
    if (lane == 0) ((float2*)stats)[row * (D / 64) + (c0 >> 6)] = make_float2(s, q);
  }
}

// Row centring of a freshly produced split stream (mickey_hip.h, mk_recentre_split): every row gets its own mean taken off
// -- LayerNorm, the stream's only reader, cannot tell -- so that the FIRST consumer of the folded LayerNorm (qkv of block 0, on
// the patch embedding's output) also multiplies rows whose 16-bit hi plane rounds x - mean rather than x; from then on the
// consumers publish the means and the producers keep the rows centred (GemmParams::ln_shift_*).  One wave per row, two reads
// of the row (the second one hits L1 / L2); statistics in the epilogues' order (quad_stats + row16_sum).
template <typename T>
__global__ __launch_bounds__(256) void recentre_kernel(T* __restrict__ xh, T* __restrict__ xl, float* __restrict__ stats,
                                                       long long rows, int D) {
  using V4 = typename mk::Lp<T>::V4;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nslot = D >> 6;
  T* ph = xh + row * D;
  T* pl = xl + row * D;
  const int quad = lane & 15, sub = lane >> 4;   // a 16-lane DPP row owns one 64-column slot at a time
  float sum = 0.f;
  for (int s0 = 0; s0 < nslot; s0 += 4) {
    const int slot = s0 + sub;
    if (slot < nslot) {
      const V4 h = *(const V4*)(ph + slot * 64 + quad * 4), l = *(const V4*)(pl + slot * 64 + quad * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += (float)h[e] + (float)l[e];
    }
  }
  const float mean = mk::wave_sum(sum) / (float)D;
  for (int s0 = 0; s0 < nslot; s0 += 4) {
    const int slot = s0 + sub;
    const bool ok = slot < nslot;
    f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ok) {
      const V4 h = *(const V4*)(ph + slot * 64 + quad * 4), l = *(const V4*)(pl + slot * 64 + quad * 4);
      V4 oh, ol;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[e] = ((float)h[e] + (float)l[e]) - mean;
        oh[e] = (T)x[e];
        ol[e] = (T)(x[e] - (float)oh[e]);
      }
      *(V4*)(ph + slot * 64 + quad * 4) = oh;
      *(V4*)(pl + slot * 64 + quad * 4) = ol;
    }
    float s, q;
    mk::gemm::quad_stats(x, s, q);
    s = mk::gemm::row16_sum(s);
    q = mk::gemm::row16_sum(q);
    if (ok && quad == 0) ((float2*)stats)[row * nslot + slot] = make_float2(s, q);
  }
}

}  // namespace

// ---- error string + version (host side) ---------------------------------------------------------------
static thread_local char g_err[512] = "";
void mk_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" {

int mk_version(void) { return 100; }

const char* mk_last_error(void) { return g_err; }

static int layernorm_launch(const float* x, int ldx, const float* w, const float* b, float eps, void* out, int ldo, int out_is_f32,
                            float* resid, int ldr, int rows_out, int D, int rows_per_img, int skip, int wgroup_rows, int bord_h,
                            int bord_w, int bord_m, int dtype, void* out_lo, float plane_scale, int* sat_flag, mk_stream_t stream) {
  MK_CHECK_ARG(x && w && b && (out || resid), "mk_layernorm: null pointer");
  MK_CHECK_ARG(bord_h == 0 || (bord_h > 0 && bord_w > 0 && bord_m > 0 && bord_m % (bord_h * bord_w) == 0 && rows_out % bord_m == 0),
               "mk_layernorm: bordered output needs rows_out = k * bord_m, bord_m = nimg * bord_h * bord_w");
  MK_CHECK_ARG(D > 0 && D % 4 == 0 && D <= LN_MAXV * 256, "mk_layernorm: D=%d must be a multiple of 4 and <= %d", D,
               LN_MAXV * 256);
  MK_CHECK_ARG(rows_out > 0 && rows_per_img > skip && skip >= 0 && ldx % 4 == 0 && ldo % 4 == 0 && ldr % 4 == 0,
               "mk_layernorm: bad geometry");
  MK_CHECK_ARG(ldx >= D && (!out || ldo >= D) && (!resid || ldr >= D),
               "mk_layernorm: leading dimensions (ldx=%d ldo=%d ldr=%d) must be >= D=%d", ldx, ldo, ldr, D);
  if (D <= 128) {
    dim3 gridn((rows_out + 8 * LNN_TRIPS - 1) / (8 * LNN_TRIPS));
#define MK_LNN(T_)                                                                                                         \
  hipLaunchKernelGGL((layernorm_narrow_kernel<T_>), gridn, dim3(256), 0, (hipStream_t)stream, x, ldx, w, b, eps, out, ldo, \
                     out_is_f32, resid, ldr, rows_out, D, rows_per_img, skip, wgroup_rows, bord_h, bord_w, bord_m, out_lo, plane_scale, sat_flag)
    if (dtype == MK_BF16) MK_LNN(__bf16);
    else if (dtype == MK_F16) MK_LNN(_Float16);
    else MK_LNN(float);
#undef MK_LNN
    MK_CHECK_LAUNCH();
    return MK_OK;
  }
  dim3 grid((rows_out + 4 * LN_RPW - 1) / (4 * LN_RPW));
#define MK_LN(T_, V_)                                                                                                  \
  hipLaunchKernelGGL((layernorm_kernel<T_, V_>), grid, dim3(256), 0, (hipStream_t)stream, x, ldx, w, b, eps, out, ldo, \
                     out_is_f32, resid, ldr, rows_out, D, rows_per_img, skip, wgroup_rows, bord_h, bord_w, bord_m, out_lo, plane_scale, sat_flag)
  if (dtype == MK_BF16) {
    if (D <= 1024) MK_LN(__bf16, 4); else MK_LN(__bf16, LN_MAXV);
  } else if (dtype == MK_F16) {
    if (D <= 1024) MK_LN(_Float16, 4); else MK_LN(_Float16, LN_MAXV);
  } else {
    if (D <= 1024) MK_LN(float, 4); else MK_LN(float, LN_MAXV);
  }
#undef MK_LN
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_layernorm(const float* x, int ldx, const float* w, const float* b, float eps, void* out, int ldo, int out_is_f32,
                 float* resid, int ldr, int rows_out, int D, int rows_per_img, int skip, int wgroup_rows, int bord_h,
                 int bord_w, int bord_m, int dtype, mk_stream_t stream) {
  return layernorm_launch(x, ldx, w, b, eps, out, ldo, out_is_f32 ? 1 : 0, resid, ldr, rows_out, D, rows_per_img, skip, wgroup_rows,
                          bord_h, bord_w, bord_m, dtype, nullptr, 1.0f, nullptr, stream);
}

int mk_layernorm_planes(const float* x, int ldx, const float* w, const float* b, float eps, void* out_hi, void* out_lo, int ldo,
                        float plane_scale, float* resid, int ldr, int rows_out, int D, int rows_per_img, int skip, int wgroup_rows,
                        int bord_h, int bord_w, int bord_m, int* sat_flag, mk_stream_t stream) {
  MK_CHECK_ARG(out_hi, "mk_layernorm_planes: null plane pointer");
  return layernorm_launch(x, ldx, w, b, eps, out_hi, ldo, 2, resid, ldr, rows_out, D, rows_per_img, skip, wgroup_rows, bord_h, bord_w,
                          bord_m, MK_F32, out_lo, plane_scale, sat_flag, stream);
}

int mk_layernorm_nchw(const float* x, int ldx, const float* w, const float* b, float eps, float* out, int nimg, int npix, int D,
                      int rows_per_img, int skip, int round_fp16, mk_stream_t stream) {
  MK_CHECK_ARG(x && w && b && out, "mk_layernorm_nchw: null pointer");
  MK_CHECK_ARG(D > 0 && D % 4 == 0 && D <= LN_MAXV * 256, "mk_layernorm_nchw: D=%d must be a multiple of 4 and <= %d", D,
               LN_MAXV * 256);
  MK_CHECK_ARG(nimg > 0 && npix > 0 && skip >= 0 && rows_per_img >= skip + npix && ldx >= D && ldx % 4 == 0,
               "mk_layernorm_nchw: bad geometry (nimg=%d npix=%d rows_per_img=%d skip=%d ldx=%d)", nimg, npix, rows_per_img, skip, ldx);
  const int tiles = (npix + NCHW_TP - 1) / NCHW_TP;
  MK_CHECK_ARG((long long)nimg * tiles <= 0x7fffffffLL, "mk_layernorm_nchw: too many tiles");
  const dim3 grid((unsigned)(nimg * tiles));
#define MK_LNT(V_, N_)                                                                                                      \
  hipLaunchKernelGGL((layernorm_nchw_kernel<V_, N_>), grid, dim3(256), 0, (hipStream_t)stream, x, ldx, w, b, eps, out, npix, D, \
                     rows_per_img, skip, tiles, round_fp16 ? 1 : 0)
  // the arithmetic form follows mk_layernorm's dispatch (layernorm_launch): the two entry points write the same bits
  if (D <= 128) MK_LNT(4, true);
  else if (D <= 1024) MK_LNT(4, false);
  else MK_LNT(LN_MAXV, false);
#undef MK_LNT
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_im2col_patch14(const float* img, long long stride_img, long long stride_ch, int stride_row, int nimg, int gh,
                      int gw, void* out, int ldo, int dtype, mk_stream_t stream) {
  MK_CHECK_ARG(img && out && nimg > 0 && gh > 0 && gw > 0, "mk_im2col_patch14: bad args");
  MK_CHECK_ARG(ldo >= 588 && ldo % 8 == 0, "mk_im2col_patch14: ldo=%d must be >= 588 and a multiple of 8", ldo);
  const long long total = (long long)nimg * gh * gw * (ldo / 4);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 16384) blocks = 16384;
  if (dtype == MK_BF16)
    hipLaunchKernelGGL(im2col14_kernel<__bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, stride_img, stride_ch,
                       stride_row, nimg, gh, gw, (__bf16*)out, ldo);
  else if (dtype == MK_F16)
    hipLaunchKernelGGL(im2col14_kernel<_Float16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, stride_img,
                       stride_ch, stride_row, nimg, gh, gw, (_Float16*)out, ldo);
  else
    hipLaunchKernelGGL(im2col14_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, stride_img,
                       stride_ch, stride_row, nimg, gh, gw, (float*)out, ldo);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_cls_token(const float* cls, const float* pos, float* x, int nimg, int ntok, int D, mk_stream_t stream) {
  MK_CHECK_ARG(cls && pos && x && nimg > 0 && ntok > 0 && D > 0, "mk_cls_token: bad args");
  hipLaunchKernelGGL(cls_kernel, dim3((nimg * D + 255) / 256), dim3(256), 0, (hipStream_t)stream, cls, pos, x, nimg, ntok, D);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

/* the CLS rows of the split residual stream (hi / lo planes) + their per-slot statistics */
int mk_cls_token_ln(const float* cls, const float* pos, void* xh, void* xl, float* stats, int nimg, int ntok, int D, int dtype,
                    mk_stream_t stream) {
  MK_CHECK_ARG(cls && pos && xh && xl && stats && nimg > 0 && ntok > 0 && D > 0 && D % 64 == 0, "mk_cls_token_ln: bad args");
  MK_CHECK_ARG(dtype == MK_BF16 || dtype == MK_F16, "mk_cls_token_ln: 16-bit dtypes only");
  if (dtype == MK_BF16)
    hipLaunchKernelGGL((cls_ln_kernel<__bf16>), dim3(nimg), dim3(64), 0, (hipStream_t)stream, cls, pos, (__bf16*)xh, (__bf16*)xl, stats, ntok, D);
  else
    hipLaunchKernelGGL((cls_ln_kernel<_Float16>), dim3(nimg), dim3(64), 0, (hipStream_t)stream, cls, pos, (_Float16*)xh, (_Float16*)xl, stats, ntok, D);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

/* centre every row of a split stream on its own mean (in place) and rewrite its per-slot statistics */
int mk_recentre_split(void* xh, void* xl, float* stats, long long rows, int D, int dtype, mk_stream_t stream) {
  MK_CHECK_ARG(xh && xl && stats && rows > 0 && D > 0 && D % 64 == 0, "mk_recentre_split: bad args");
  MK_CHECK_ARG(dtype == MK_BF16 || dtype == MK_F16, "mk_recentre_split: 16-bit dtypes only");
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (dtype == MK_BF16)
    hipLaunchKernelGGL((recentre_kernel<__bf16>), grid, dim3(256), 0, (hipStream_t)stream, (__bf16*)xh, (__bf16*)xl, stats, rows, D);
  else
    hipLaunchKernelGGL((recentre_kernel<_Float16>), grid, dim3(256), 0, (hipStream_t)stream, (_Float16*)xh, (_Float16*)xl, stats, rows, D);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

}  // extern "C"
