// mickey_amd -- the training side of the heads' 3x3 convolutions (reference utils/extractor_utils.py:18-31: nn.Conv2d(k=3, stride=1,
// padding=1, bias=False) in fp32, forward and backward through autograd).
//
// Forward and input gradient are mk_conv3x3_split_dscale -- mk_conv3x3_split's kernels (mk_gemm.hip, untouched) followed by one pass
// that applies the accumulator scale from DEVICE memory -- on operand planes prepared here, on the device, every step:
//   * absmax_*_kernel      deterministic abs-max of a tensor -> a power-of-two plane scale kept in device memory (s, 1 / s)
//   * planes_kernel        fp32 NCHW of any strides -> bordered (hi, lo) fp16 planes (a tiled transpose through LDS)
//   * weight_planes_kernel fp32 [Cout, Cin, 3, 3] -> the interleaved (32 hi | 32 lo) tap-major planes, forward order or the
//                          flipped / transposed order of the input gradient
// The weight gradient is the new GEMM.  Both operands are bordered maps, gY [rows, Cout] and X [rows, Cin], and because the border
// rows of gY are zero the gradient is a plain sum over ALL bordered rows with one row shift per tap:
//   dW[co, tap, ci] = sum_r gY[r, co] . X[r + dy (W+1) + dx, ci]
// i.e. A^T . B with M = Cout, N = 9 Cin and the contraction over rows, while both operands are channel-contiguous in memory.
// wgrad_kernel: 128 x 128 output tile, 4 waves (2 x 2, 64 x 64 each) of v_mfma_f32_16x16x32_f16; a K step is 32 rows; the four
// planes gY_hi, gY_lo, X_hi, X_lo of a step go HBM -> LDS by LDS-DMA as [32 rows][128 channels] images of 256-byte rows (one wave
// per image), double-buffered, one barrier per step; the fragments come out of LDS TRANSPOSED by ds_read_b64_tr_b16 (4 rows x 16
// channels per 16 lanes; two reads = the 8 contraction values of a lane).  The image's 16-byte chunks are XOR-swizzled with
// ((row & 3) << 2) | ((row >> 2) & 3): the four rows of a block land in four different 64-byte quarters of the 256-byte bank
// period and the two blocks of a 32-lane half (8 rows apart, same channels) in different chunks of a quarter -- conflict-free.
// The swizzle is applied to the per-lane SOURCE address of the DMA and to the read address.  Every lane always reads: out-of-range
// channels are redirected to channel 0 and their results dropped at the store (the transposed read needs EXEC all ones).
// Three MFMA sets per step from operands staged once: gY_hi.X_hi, gY_lo.X_hi, gY_hi.X_lo, fp32 accumulation.
// Split K: the rows are cut into fixed chunks of K steps (a function of the shape only), each (tile, chunk) writes its partial
// to `work`, and wgrad_reduce_kernel adds the partials in chunk order, undoes the plane scales and writes [Cout, Cin, 3, 3].
// No atomics anywhere: every result is bit-identical from run to run.
#include "mk_common.hpp"

namespace mk {
namespace trainconv {
namespace {

constexpr int ABSMAX_BLOCKS = 1024;

// ---- abs-max -> power-of-two scale --------------------------------------------------------------------------------------------
// |x| compared as raw bits: non-negative floats order like unsigned integers, Inf above every finite value, NaN above Inf -- a
// non-finite element always wins the maximum (max is exact: any order gives the same bits).
__device__ __forceinline__ unsigned block_max_u32(unsigned m, unsigned* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned other = (unsigned)__shfl_xor((int)m, o, 64);
    m = m > other ? m : other;
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  unsigned r = sh[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) r = r > sh[w] ? r : sh[w];
  return r;
}

// x: n elements; flat (d1 == 0): x[i]; otherwise a 4-d tensor [d0, d1, d2, d3] with element strides s0..s3
__global__ __launch_bounds__(256) void absmax_partial_kernel(const float* __restrict__ x, long long n, int d1, int d2, int d3,
                                                             long long s0, long long s1, long long s2, long long s3,
                                                             unsigned* __restrict__ part) {
  __shared__ unsigned sh[4];
  unsigned m = 0;
  const long long step = (long long)gridDim.x * 256;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += step) {
    long long off = i;
    if (d1 != 0) {
      const long long q3 = i / d3;
      const int i3 = (int)(i - q3 * d3);
      const long long q2 = q3 / d2;
      const int i2 = (int)(q3 - q2 * d2);
      const long long i0 = q2 / d1;
      const int i1 = (int)(q2 - i0 * d1);
      off = i0 * s0 + i1 * s1 + i2 * s2 + i3 * s3;
    }
    const unsigned b = __builtin_bit_cast(unsigned, x[off]) & 0x7fffffffu;
    m = m > b ? m : b;
  }
  m = block_max_u32(m, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

// scale[0] = s, a power of two with max|x| * s in [2^14, 2^15) (hi plane finite in fp16, lo plane of every element within 2^-17
// of the maximum clear of fp16's subnormals), exponent clamped to +-100; scale[1] = 1 / s.  All-zero tensor: s = 1.  A non-finite
// element: s = 1 and scale[1] = NaN, so that everything computed from these planes is non-finite whatever the planes hold.
__global__ __launch_bounds__(256) void absmax_final_kernel(const unsigned* __restrict__ part, int nb, float* __restrict__ scale) {
  __shared__ unsigned sh[4];
  unsigned m = 0;
  for (int i = threadIdx.x; i < nb; i += 256) m = m > part[i] ? m : part[i];
  m = block_max_u32(m, sh);
  if (threadIdx.x == 0) {
    float s = 1.f, inv = 1.f;
    if (m >= 0x7f800000u) {
      inv = __builtin_bit_cast(float, 0x7fc00000u);
    } else if (m != 0) {
      int e = (int)(m >> 23);
      e = e < 1 ? 1 : e;
      int be = 268 - e;   // biased exponent of 2^(14 - (e - 127))
      be = be < 27 ? 27 : (be > 227 ? 227 : be);
      s = __builtin_bit_cast(float, (unsigned)be << 23);
      inv = __builtin_bit_cast(float, (unsigned)(254 - be) << 23);
    }
    scale[0] = s;
    scale[1] = inv;
  }
}

// ---- fp32 NCHW (any strides) -> bordered (hi, lo) fp16 planes -----------------------------------------------------------------
// A block moves 64 pixels x 32 channels through LDS: read along the unit-stride dimension of the source (CFAST: channels, i.e.
// channels_last -- otherwise pixels), written along channels, 4 channels = 8 bytes per lane and plane.  x * s = hi + lo without
// clamping (|x * s| < 2^15 by construction of s; an Inf gives hi = Inf, lo = NaN).
template <bool CFAST>
__global__ __launch_bounds__(256) void planes_kernel(const float* __restrict__ src, long long sb, long long sc, long long sh, long long sw,
                                                     int npix, int C, int H, int Wd, const float* __restrict__ scale,
                                                     _Float16* __restrict__ hi, _Float16* __restrict__ lo, int ld) {
  __shared__ float tile[64][33];
  const int t = threadIdx.x;
  const int m0 = blockIdx.x * 64, c0 = blockIdx.y * 32;
  const float s = scale[0];
  auto src_off = [&](int m) -> long long {
    const int q = m / Wd, b = q / H;
    return b * sb + (q - b * H) * sh + (m - q * Wd) * sw;
  };
  if (CFAST) {
    const int c = c0 + (t & 31);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int pl = i * 8 + (t >> 5), m = m0 + pl;
      tile[pl][t & 31] = (m < npix && c < C) ? src[src_off(m) + c * sc] : 0.f;
    }
  } else {
    const int pl = t & 63, m = m0 + pl;
    const long long po = m < npix ? src_off(m) : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int cl = i * 4 + (t >> 6), c = c0 + cl;
      tile[pl][cl] = (m < npix && c < C) ? src[po + c * sc] : 0.f;
    }
  }
  __syncthreads();
  const int c4 = (t & 7) * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pl = i * 32 + (t >> 3), m = m0 + pl;
    if (m >= npix || c0 + c4 >= C) continue;   // C % 4 == 0
    f16x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = tile[pl][c4 + e] * s;
      h[e] = (_Float16)v;
      l[e] = (_Float16)(v - (float)h[e]);
    }
    const long long o = bordered_row(m, H, Wd) * ld + c0 + c4;
    *(f16x4*)(hi + o) = h;
    *(f16x4*)(lo + o) = l;
  }
}

// ---- fp32 [Cout, Cin, 3, 3] -> interleaved (32 hi | 32 lo) planes of w * s ----------------------------------------------------
// mode 0 (forward): row co, column k = tap Cin + ci                          <- w[co, ci, tap]
// mode 1 (input gradient): row ci, column k = tap Cp + co, co < Cp           <- w[co, ci, 8 - tap] (co >= Cout: 0), Cp = Cout
//         rounded up to 32: the conv that reads gY's planes [rows, Cp] and gives gX
// acc[0] = 1 / (s_w s_a): the accumulator scale of the conv that uses these planes with activation planes of scale s_a.
__global__ __launch_bounds__(256) void weight_planes_kernel(const float* __restrict__ w, int Cout, int Cin, int mode, int Cp,
                                                            const float* __restrict__ w_scale, const float* __restrict__ a_scale,
                                                            _Float16* __restrict__ planes, float* __restrict__ acc) {
  const int rows = mode ? Cin : Cout, cs = mode ? Cp : Cin, K = 9 * cs;
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t == 0) acc[0] = w_scale[1] * a_scale[1];
  if (t >= (long long)rows * K) return;
  const int r = (int)(t / K), k = (int)(t - (long long)r * K);
  const int tap = k / cs, c = k - tap * cs;
  float v = 0.f;
  if (mode == 0) v = w[((long long)r * Cin + c) * 9 + tap];
  else if (c < Cout) v = w[((long long)c * Cin + r) * 9 + (8 - tap)];
  v *= w_scale[0];
  const _Float16 h = (_Float16)v;
  const long long o = (long long)r * 2 * K + (k >> 5) * 64 + (k & 31);
  planes[o] = h;
  planes[o + 32] = (_Float16)(v - (float)h);
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------------
struct WgradParams {
  const _Float16 *gy_hi, *gy_lo;   // planes of gY, [rows, ldg], at bordered row 0
  const _Float16 *x_hi, *x_lo;     // planes of X, [rows, Cin], at bordered row 0
  float* work;             // [ksplit][Cout][N] partial sums
  int ldg, Cin, Cout, N, Wd, nsteps, chunk;
};

constexpr int W_STAGE = 4 * 8192;   // four [32][128] fp16 images

typedef __fp16 v4f16 __attribute__((__vector_size__(4 * sizeof(__fp16))));

__device__ __forceinline__ f16x8 tr_frag(const char* img, unsigned a0, unsigned a1) {
  const v4f16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) v4f16*)(img + a0));
  const v4f16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) v4f16*)(img + a1));
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
  const u32x2 a = __builtin_bit_cast(u32x2, lo), b = __builtin_bit_cast(u32x2, hi);
  return __builtin_bit_cast(f16x8, u32x4v{a[0], a[1], b[0], b[1]});
}

__global__ __launch_bounds__(256, 2) void wgrad_kernel(WgradParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][gY_hi | gY_lo | X_hi | X_lo]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntm = (p.Cout + 127) / 128;
  const int m0 = (blockIdx.x % ntm) * 128, n0 = (blockIdx.x / ntm) * 128;
  const int kt0 = blockIdx.y * p.chunk;
  const int nk = min(p.chunk, p.nsteps - kt0);

  // staging: wave w fills image w (8 pieces of 4 rows); this lane feeds row +(lane >> 4), chunk position lane & 15 of a piece
  const bool isx = wave >= 2;
  const _Float16* const base = wave == 0 ? p.gy_hi : wave == 1 ? p.gy_lo : wave == 2 ? p.x_hi : p.x_lo;
  const int ld = isx ? p.Cin : p.ldg;
  // DMA address = wave-uniform base (SGPRs: plane + K step + piece, lowered by `lead` rows so that no tap shift makes a lane offset
  // negative -- a matter of arithmetic only: nothing in front of the rows named in mickey_hip.h is read) + per-lane byte offset
  const int lead = p.Wd + 2;
  unsigned voff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ch = (lane & 15) ^ (((lane >> 4) << 2) | j);   // the source chunk that lands here (rows 4 piece + (lane >> 4))
    int col;
    if (isx) {
      int n = n0 + ch * 8;
      n = n < p.N ? n : 0;
      const int tap = n / p.Cin;
      col = ((tap / 3 - 1) * (p.Wd + 1) + tap % 3 - 1) * p.Cin + (n - tap * p.Cin);
    } else {
      const int co = m0 + ch * 8;
      col = co < p.ldg ? co : 0;
    }
    voff[j] = (unsigned)((((lane >> 4) + lead) * ld + col) * 2);
  }
  auto issue = [&](int kt, int stage) {
    char* dst = smem + stage * W_STAGE + wave * 8192;
    const char* sb = (const char*)base + ((long long)kt * 32 - lead) * ld * 2;
#pragma unroll
    for (int j = 0; j < 8; ++j) glds16_sv(sb + (long long)(8 * j) * ld, voff[j & 3], dst + j * 1024);
  };

  // transposed fragment reads: 16-lane group kg takes rows 8 kg + 4 h + q, lane 4 q + pp supplies columns 4 pp .. 4 pp + 3
  const int fr = lane & 15, kg = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int wm = wave >> 1, wn = wave & 1;
  unsigned ag[4][2], ax[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = kg * 8 + h * 4 + q;
      const int sw = (q << 2) | ((2 * kg + h) & 3);
      ag[i][h] = 256 * row + 16 * ((2 * (wm * 4 + i) + (pp >> 1)) ^ sw) + 8 * (pp & 1);
      ax[i][h] = 256 * row + 16 * ((2 * (wn * 4 + i) + (pp >> 1)) ^ sw) + 8 * (pp & 1);
    }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(kt0, 0);
  for (int it = 0; it < nk; ++it) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (it + 1 < nk) issue(kt0 + it + 1, (it + 1) & 1);
    const char* st = smem + (it & 1) * W_STAGE;
    f16x8 gf[2][4], xf[2][4];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        gf[pl][i] = tr_frag(st + pl * 8192, ag[i][0], ag[i][1]);
        xf[pl][i] = tr_frag(st + (2 + pl) * 8192, ax[i][0], ax[i][1]);
      }
#pragma unroll
    for (int pr = 0; pr < 3; ++pr)   // gY_hi . X_hi, gY_lo . X_hi, gY_hi . X_lo
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = Lp<_Float16>::mma16(xf[pr == 2][mi], gf[pr == 1][ni], acc[ni][mi]);
  }
  // lane: output row co = .. + fr, columns n .. n + 3 with n = .. + 4 kg
  float* const out = p.work + (long long)blockIdx.y * p.Cout * p.N;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int co = m0 + wm * 64 + ni * 16 + fr;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int n = n0 + wn * 64 + mi * 16 + kg * 4;
      if (co < p.Cout && n < p.N) *(f32x4*)(out + (long long)co * p.N + n) = acc[ni][mi];
    }
  }
}

// dW[co, ci, tap] = (1 / (s_g s_x)) * sum over the K chunks, in chunk order, of work[chunk][co][tap Cin + ci]
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ work, int ksplit, int Cout, int Cin,
                                                           const float* __restrict__ g_scale, const float* __restrict__ x_scale,
                                                           float* __restrict__ dw) {
  const int N = 9 * Cin;
  const long long total = (long long)Cout * N, t = blockIdx.x * 256LL + threadIdx.x;
  if (t >= total) return;
  float s = 0.f;
  for (int k = 0; k < ksplit; ++k) s += work[k * total + t];
  const int co = (int)(t / N), n = (int)(t - (long long)co * N);
  const int tap = n / Cin, ci = n - tap * Cin;
  dw[((long long)co * Cin + ci) * 9 + tap] = s * (g_scale[1] * x_scale[1]);
}

// out[i] *= scale[0]: the power-of-two plane scales come off the split conv's fp32 rows (bit-identical to scaling in its epilogue)
__global__ __launch_bounds__(256) void scale_rows_kernel(f32x4* __restrict__ out, long long n4, const float* __restrict__ scale) {
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t >= n4) return;
  const float s = scale[0];
  f32x4 v = out[t];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] *= s;
  out[t] = v;
}

// the K split of a shape: chunk = K steps per block (fixed by the shape alone), returns the number of chunks
int wgrad_split(int Cout, int Cin, int nimg, int H, int Wd, int* chunk, int* nsteps) {
  const long long rows = bordered_rows(nimg, H, Wd);
  const int ns = (int)((rows + 31) / 32);
  const long long tiles = (long long)((Cout + 127) / 128) * ((9LL * Cin + 127) / 128);
  long long ks = 512 / tiles;   // about two workgroups per CU of a 256-CU part
  ks = ks > ns / 4 ? ns / 4 : ks;
  ks = ks < 1 ? 1 : ks;
  const int c = (int)((ns + ks - 1) / ks);
  *chunk = c;
  *nsteps = ns;
  return (ns + c - 1) / c;
}

int check_geometry(int Cout, int Cin, int nimg, int H, int Wd, const char* who) {
  MK_CHECK_ARG(Cout > 0 && Cin > 0 && nimg > 0 && H > 0 && Wd > 0, "%s: sizes must be positive", who);
  MK_CHECK_ARG(Cin % 32 == 0 && Cout % 4 == 0, "%s: Cin must be a multiple of 32 and Cout of 4 (Cin=%d, Cout=%d)", who, Cin, Cout);
  MK_CHECK_ARG(bordered_rows(nimg, H, Wd) + 2LL * Wd + 64 < (1ll << 26), "%s: feature maps of 2^26 bordered rows or more", who);
  return MK_OK;
}

}  // namespace
}  // namespace trainconv
}  // namespace mk

using namespace mk;
using namespace mk::trainconv;

extern "C" {

long long mk_absmax_scale_work_floats(void) { return ABSMAX_BLOCKS; }

int mk_absmax_scale(const float* x, int d0, int d1, int d2, int d3, long long s0, long long s1, long long s2, long long s3,
                    float* work, float* scale, mk_stream_t stream) {
  MK_CHECK_ARG(x && work && scale, "mk_absmax_scale: null pointer");
  MK_CHECK_ARG(d0 > 0 && d1 > 0 && d2 > 0 && d3 > 0, "mk_absmax_scale: sizes must be positive");
  const long long n = (long long)d0 * d1 * d2 * d3;
  // dense in the given order: a flat sweep
  const bool flat = s3 == 1 && s2 == d3 && s1 == (long long)d2 * d3 && s0 == (long long)d1 * d2 * d3;
  long long nb = (n + 1023) / 1024;
  nb = nb > ABSMAX_BLOCKS ? ABSMAX_BLOCKS : nb;
  hipLaunchKernelGGL(absmax_partial_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, n, flat ? 0 : d1, d2, d3, s0, s1,
                     s2, s3, (unsigned*)work);
  MK_CHECK_LAUNCH();
  hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const unsigned*)work, (int)nb, scale);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

long long mk_conv_train_lead_rows(int Wd) { return Wd > 0 ? Wd + 2 : 0; }

long long mk_conv_train_plane_rows(int nimg, int H, int Wd) {
  if (nimg <= 0 || H <= 0 || Wd <= 0) return 0;
  return (Wd + 2) + (bordered_rows(nimg, H, Wd) + 31) / 32 * 32 + (Wd + 2);
}

int mk_conv_train_planes(const float* src, long long stride_b, long long stride_c, long long stride_h, long long stride_w, int nimg,
                         int C, int H, int Wd, const float* scale, void* hi, void* lo, int ld, mk_stream_t stream) {
  MK_CHECK_ARG(src && scale && hi && lo, "mk_conv_train_planes: null pointer");
  MK_CHECK_ARG(nimg > 0 && C > 0 && H > 0 && Wd > 0 && C % 4 == 0 && ld % 4 == 0 && ld >= C,
               "mk_conv_train_planes: sizes must be positive, C and ld multiples of 4, ld >= C");
  MK_CHECK_ARG(stride_b >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, "mk_conv_train_planes: negative stride");
  MK_CHECK_ARG((((uintptr_t)hi | (uintptr_t)lo) & 7) == 0, "mk_conv_train_planes: planes must be 8-byte aligned");
  MK_CHECK_ARG((long long)nimg * H * Wd < (1ll << 30), "mk_conv_train_planes: too many pixels");
  const int npix = nimg * H * Wd;
  const dim3 grid((npix + 63) / 64, (C + 31) / 32);
  if (stride_c == 1)
    hipLaunchKernelGGL(planes_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, stride_b, stride_c, stride_h, stride_w, npix, C, H,
                       Wd, scale, (_Float16*)hi, (_Float16*)lo, ld);
  else
    hipLaunchKernelGGL(planes_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, stride_b, stride_c, stride_h, stride_w, npix, C,
                       H, Wd, scale, (_Float16*)hi, (_Float16*)lo, ld);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_conv_train_weight_planes(const float* w, int Cout, int Cin, int transposed, const float* w_scale, const float* act_scale,
                                void* planes, float* acc_scale, mk_stream_t stream) {
  MK_CHECK_ARG(w && w_scale && act_scale && planes && acc_scale, "mk_conv_train_weight_planes: null pointer");
  MK_CHECK_ARG(Cout > 0 && Cin > 0 && Cin % 32 == 0 && Cout % 4 == 0,
               "mk_conv_train_weight_planes: Cin must be a multiple of 32 and Cout of 4 (Cin=%d, Cout=%d)", Cin, Cout);
  const int Cp = (Cout + 31) / 32 * 32;
  const long long total = transposed ? (long long)Cin * 9 * Cp : (long long)Cout * 9 * Cin;
  MK_CHECK_ARG(total < (1ll << 31), "mk_conv_train_weight_planes: weight too large");
  hipLaunchKernelGGL(weight_planes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin,
                     transposed ? 1 : 0, Cp, w_scale, act_scale, (_Float16*)planes, acc_scale);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_conv3x3_split_dscale(const void* in_hi, const void* in_lo, int C1, const void* W, int ldw, float* out, int Cout, int nimg, int H,
                            int Wd, const float* acc_scale, mk_stream_t stream) {
  MK_CHECK_ARG(in_hi && in_lo && W && out && acc_scale, "mk_conv3x3_split_dscale: null pointer");
  MK_CHECK_ARG(C1 > 0 && Cout > 0 && nimg > 0 && H > 0 && Wd > 0, "mk_conv3x3_split_dscale: sizes must be positive");
  MK_CHECK_ARG(C1 % 32 == 0 && Cout % 4 == 0 && ldw >= 18 * C1,
               "mk_conv3x3_split_dscale: C1 must be a multiple of 32, Cout of 4 and ldw >= 18 C1 (C1=%d, Cout=%d, ldw=%d)", C1, Cout, ldw);
  MK_CHECK_ARG(((uintptr_t)out & 15) == 0, "mk_conv3x3_split_dscale: out must be 16-byte aligned");
  // the accumulators leave the conv unscaled (fp32: sums of |hi . hi| <= 2^30 products, far from overflow) ...
  if (int e = mk_conv3x3_split(in_hi, in_lo, 0, C1, nullptr, nullptr, 0, 0, W, ldw, 0, nullptr, 0, out, nullptr, Cout, 0, 1, nimg, H, Wd,
                               MK_ACT_NONE, 0, 1.0f, 1.0f, nullptr, stream))
    return e;
  // ... and the scale the host never sees is applied in place
  const long long n4 = (long long)nimg * H * Wd * (Cout / 4);
  hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (f32x4*)out, n4, acc_scale);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

long long mk_conv_wgrad_work_floats(int Cout, int Cin, int nimg, int H, int Wd) {
  if (Cout <= 0 || Cin <= 0 || nimg <= 0 || H <= 0 || Wd <= 0) return 0;
  int chunk, nsteps;
  return (long long)wgrad_split(Cout, Cin, nimg, H, Wd, &chunk, &nsteps) * Cout * 9 * Cin;
}

int mk_conv_wgrad(const void* gy_hi, const void* gy_lo, int ldg, const void* x_hi, const void* x_lo, int Cout, int Cin, int nimg, int H,
                  int Wd, const float* gy_scale, const float* x_scale, float* work, float* dw, mk_stream_t stream) {
  MK_CHECK_ARG(gy_hi && gy_lo && x_hi && x_lo && gy_scale && x_scale && work && dw, "mk_conv_wgrad: null pointer");
  if (int e = check_geometry(Cout, Cin, nimg, H, Wd, "mk_conv_wgrad")) return e;
  MK_CHECK_ARG(ldg % 32 == 0 && ldg >= Cout, "mk_conv_wgrad: ldg must be a multiple of 32 and >= Cout");
  MK_CHECK_ARG((((uintptr_t)gy_hi | (uintptr_t)gy_lo | (uintptr_t)x_hi | (uintptr_t)x_lo | (uintptr_t)work | (uintptr_t)dw) & 15) == 0,
               "mk_conv_wgrad: planes, work and dw must be 16-byte aligned");
  WgradParams p;
  p.gy_hi = (const _Float16*)gy_hi; p.gy_lo = (const _Float16*)gy_lo;
  p.x_hi = (const _Float16*)x_hi; p.x_lo = (const _Float16*)x_lo;
  p.work = work; p.ldg = ldg; p.Cin = Cin; p.Cout = Cout; p.N = 9 * Cin; p.Wd = Wd;
  const int ksplit = wgrad_split(Cout, Cin, nimg, H, Wd, &p.chunk, &p.nsteps);
  static bool attr_done = false;   // benign race: the attribute call is idempotent
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute((const void*)wgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * W_STAGE);
    if (e != hipSuccess) {
      mk_set_error("mk_conv_wgrad: cannot reserve %d B of LDS: %s", 2 * W_STAGE, hipGetErrorString(e));
      return MK_ERR_LAUNCH;
    }
    attr_done = true;
  }
  const int tiles = ((Cout + 127) / 128) * ((p.N + 127) / 128);
  hipLaunchKernelGGL(wgrad_kernel, dim3(tiles, ksplit), dim3(256), 2 * W_STAGE, (hipStream_t)stream, p);
  MK_CHECK_LAUNCH();
  const long long total = (long long)Cout * p.N;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, work, ksplit, Cout,
                     Cin, gy_scale, x_scale, dw);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

}  // extern "C"
