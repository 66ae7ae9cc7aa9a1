// mickey_amd -- trainable linear attention of the heads' Transformer_self_att (reference att_layers/attention.py:46-64 under
// autograd): forward and backward, fp32 on the vector ALU.  Per image n and head h (D = 16 channels), phi(x) = elu(x) + 1:
//
//   forward   M[d, v] = sum_s phi(k)[s, d] (v[s, v] / S)      ks[d] = sum_s phi(k)[s, d]
//             den[l] = phi(q)[l] . ks + eps                   out[l, v] = (phi(q)[l] . M[:, v]) / den[l] * S
//   backward  gnum[l, v] = gO[l, v] S / den[l]                gden[l] = -(gO[l] . out[l]) / den[l]      (out, den recomputed)
//             gQ[l, d] = (sum_v gnum[l, v] M[d, v] + gden[l] ks[d]) phi'(q[l, d])
//             gM[d, v] = sum_l phi(q)[l, d] gnum[l, v]        gks[d] = sum_l phi(q)[l, d] gden[l]
//             gK[s, d] = (sum_v (v[s, v] / S) gM[d, v] + gks[d]) phi'(k[s, d])
//             gV[s, v] = (sum_d phi(k)[s, d] gM[d, v]) / S
//
// Both token sums (M | ks over S, gM | gks over L) are the SAME reduction -- sum_t A[t, d] (B[t, v] | c[t]) -- and run the way
// linattn_kv_partial / linattn_kv_reduce of mk_heads.hip do: a workgroup stages a chunk of 64 tokens in LDS (each element
// transformed once), one wave works on a token with lane = (head, half of v, quarter of d) holding a 4 x 8 block of the outer
// product, the 4 wave partials are added in wave order, the chunk partials in chunk order by the reduce kernel.  No atomics:
// results are bit-identical from run to run and do not depend on the number of images in the call.
// The work is memory- and launch-bound (32 flops per loaded float): 3 launches forward, 3 backward (2 / 1 when no gradient of
// k and v is wanted).
#include "mk_common.hpp"

namespace {
using namespace mk;

constexpr int KVW = 272;    // 16 x 16 M + 16 ks per (image, head): the layout of mk_linattn_kv's `kv`
constexpr int CHUNK = 64;   // tokens per partial block (64 KiB of staged rows at C = 128)
constexpr int MLD = 273;    // LDS row of one head's M | ks block: heads land on different banks

__device__ __forceinline__ float phi(float x) { return x > 0.f ? x + 1.0f : expf(x); }  // elu(x) + 1; NaN stays NaN

// chunk partial of  P[h][d * 16 + v] = sum_t A[t, h 16 + d] B[t, h 16 + v],  P[h][256 + d] = sum_t A[t, h 16 + d] c[t, h]
// from the staged rows st [CHUNK][2C] (A | B) and cv [CHUNK][H] (HAS_C; else c = 1) -> part [(img H + h) nchunk + chunk][KVW].
// Called by all 256 threads after a barrier behind the staging; st is reused for the wave partials.
template <bool HAS_C>
__device__ __forceinline__ void outer_partial(float* st, const float* cv, int ntok, int C, float* __restrict__ part, long long img,
                                              int chunk, int nchunk) {
  const int H = C >> 4;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = lane >> 3, vh = (lane >> 2) & 1, dg = lane & 3;
  float acc[4][8];
  float ks[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[a][e] = 0.f;
  if (h < H) {
    for (int s = wave; s < ntok; s += 4) {   // 3 LDS reads (one broadcast within 8 lanes each) per 32 FMAs
      const float* row = st + s * 2 * C + h * 16;
      const f32x4 a4 = *(const f32x4*)(row + dg * 4);
      const f32x4 b0 = *(const f32x4*)(row + C + vh * 8), b1 = *(const f32x4*)(row + C + vh * 8 + 4);
      const float c = HAS_C ? cv[s * H + h] : 1.0f;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[a][e] += a4[a] * b0[e];
          acc[a][4 + e] += a4[a] * b1[e];
        }
        ks[a] += HAS_C ? a4[a] * c : a4[a];
      }
    }
  }
  __syncthreads();   // everybody is done reading the staged rows: the buffer now takes the 4 wave partials [wave][H][KVW]
  if (h < H) {
    float* o = st + (wave * H + h) * KVW;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[(dg * 4 + a) * 16 + vh * 8 + e] = acc[a][e];
      if (vh == 0) o[256 + dg * 4 + a] = ks[a];
    }
  }
  __syncthreads();
  for (int i = t; i < H * KVW; i += 256) {
    const int hh = i / KVW, e = i - hh * KVW;
    const float r = ((st[(0 * H + hh) * KVW + e] + st[(1 * H + hh) * KVW + e]) + st[(2 * H + hh) * KVW + e]) + st[(3 * H + hh) * KVW + e];
    part[(((img * H + hh) * nchunk) + chunk) * KVW + e] = r;
  }
}

// forward, pass over S: stages phi(k) | v / S of one chunk of one image, then the partial M | ks of every head
__global__ __launch_bounds__(256) void attn_train_kv_partial(const float* __restrict__ k, long long ldk, long long sk,
                                                             const float* __restrict__ v, long long ldv, long long sv,
                                                             float* __restrict__ part, int S, int C, int nchunk) {
  extern __shared__ __attribute__((aligned(16))) float st[];   // [CHUNK][2C]
  const long long img = blockIdx.y;
  const int chunk = blockIdx.x, t = threadIdx.x;
  const int s0 = chunk * CHUNK, ntok = min(S, s0 + CHUNK) - s0;
  const float fS = (float)S;
  const int c4 = C >> 2;
  const float* kb = k + img * sk + (long long)s0 * ldk;
  const float* vb = v + img * sv + (long long)s0 * ldv;
  for (int i = t; i < ntok * c4; i += 256) {   // 16 B per lane, a row's lanes contiguous
    const int s = i / c4, c = (i - s * c4) * 4;
    f32x4 kk = *(const f32x4*)(kb + s * ldk + c), vv = *(const f32x4*)(vb + s * ldv + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      kk[e] = phi(kk[e]);
      vv[e] = vv[e] / fS;
    }
    *(f32x4*)(st + s * 2 * C + c) = kk;
    *(f32x4*)(st + s * 2 * C + C + c) = vv;
  }
  __syncthreads();
  outer_partial<false>(st, nullptr, ntok, C, part, img, chunk, nchunk);
}

// chunk partials -> the [N H][272] block, added in chunk order
__global__ __launch_bounds__(KVW) void attn_train_reduce(const float* __restrict__ part, float* __restrict__ kv, int nchunk) {
  const long long ih = blockIdx.x;
  const int t = threadIdx.x;
  float s = 0.f;
  for (int c = 0; c < nchunk; ++c) s += part[(ih * nchunk + c) * KVW + t];
  kv[ih * KVW + t] = s;
}

__device__ __forceinline__ void load_block(float* sM, const float* __restrict__ kv, long long img, int H) {
  for (int i = threadIdx.x; i < H * KVW; i += blockDim.x) sM[(i / KVW) * MLD + (i % KVW)] = kv[img * H * KVW + i];
}

// 16 channels of one (token, head): x -> phi(x), bit d of the returned mask set where x > 0 (phi' = 1; elsewhere phi' = phi)
__device__ __forceinline__ unsigned load_phi16(const float* __restrict__ p, float (&P)[16]) {
  unsigned pos = 0;
#pragma unroll
  for (int d4 = 0; d4 < 4; ++d4) {
    const f32x4 x = *(const f32x4*)(p + d4 * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      P[d4 * 4 + e] = phi(x[e]);
      pos |= (x[e] > 0.f ? 1u : 0u) << (d4 * 4 + e);
    }
  }
  return pos;
}

__device__ __forceinline__ void store16(float* __restrict__ p, const float (&r)[16]) {
#pragma unroll
  for (int d4 = 0; d4 < 4; ++d4) *(f32x4*)(p + d4 * 4) = f32x4{r[d4 * 4], r[d4 * 4 + 1], r[d4 * 4 + 2], r[d4 * 4 + 3]};
}

// forward, pass over L: block = (256 / H) tokens x H heads of one image, one thread per (token, head)
__global__ __launch_bounds__(256) void attn_train_apply(const float* __restrict__ q, long long ldq, long long sq,
                                                        const float* __restrict__ kv, float* __restrict__ out, float eps, int L,
                                                        int S, int C) {
  extern __shared__ __attribute__((aligned(16))) float sM[];   // [H][MLD]
  const int H = C >> 4;
  const long long img = blockIdx.y;
  load_block(sM, kv, img, H);
  __syncthreads();
  const int tpb = 256 / H;
  const int h = threadIdx.x % H;
  const int l = blockIdx.x * tpb + threadIdx.x / H;
  if (l >= L || threadIdx.x >= tpb * H) return;
  float Q[16];
  load_phi16(q + img * sq + (long long)l * ldq + h * 16, Q);
  const float* M = sM + h * MLD;
  float den = 0.f;
#pragma unroll
  for (int d = 0; d < 16; ++d) den += Q[d] * M[256 + d];
  const float r = (float)S / (den + eps);
  float o[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < 16; ++d) a += Q[d] * M[d * 16 + v];
    o[v] = a * r;
  }
  store16(out + (img * L + l) * C + h * 16, o);
}

// backward, pass over L: per (token, head) of a chunk recompute den and out, write gQ, stage phi(q) | gnum and gden; then the
// chunk partial of gM | gks (skipped when part is null: nobody wants gK or gV)
__global__ __launch_bounds__(256) void attn_train_bwd_q(const float* __restrict__ q, long long ldq, long long sq,
                                                        const float* __restrict__ kv, const float* __restrict__ go, float eps,
                                                        float* __restrict__ gq, float* __restrict__ part, int L, int S, int C,
                                                        int nchunk) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int H = C >> 4;
  float* st = sm;                    // [CHUNK][2C]: phi(q) | gnum
  float* sM = sm + CHUNK * 2 * C;    // [H][MLD]
  float* cv = sM + H * MLD;          // [CHUNK][H]: gden
  const long long img = blockIdx.y;
  const int chunk = blockIdx.x, t = threadIdx.x;
  const int l0 = chunk * CHUNK, ntok = min(L, l0 + CHUNK) - l0;
  load_block(sM, kv, img, H);
  __syncthreads();
  for (int p = t; p < ntok * H; p += 256) {
    const int tok = p / H, h = p - tok * H;
    const long long l = l0 + tok;
    float Q[16], G[16], gn[16];
    const unsigned pos = load_phi16(q + img * sq + l * ldq + h * 16, Q);
    const float* grow = go + (img * L + l) * C + h * 16;
#pragma unroll
    for (int d4 = 0; d4 < 4; ++d4) {
      const f32x4 x = *(const f32x4*)(grow + d4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) G[d4 * 4 + e] = x[e];
    }
    const float* M = sM + h * MLD;
    float den = 0.f;
#pragma unroll
    for (int d = 0; d < 16; ++d) den += Q[d] * M[256 + d];
    den += eps;
    const float r = (float)S / den;
    float dot = 0.f;   // gO . out
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      float a = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) a += Q[d] * M[d * 16 + v];
      dot += G[v] * (a * r);
      gn[v] = G[v] * r;
    }
    const float gden = -dot / den;
    if (gq) {
      float g[16];
#pragma unroll
      for (int d = 0; d < 16; ++d) {
        float a = gden * M[256 + d];
#pragma unroll
        for (int v = 0; v < 16; ++v) a += gn[v] * M[d * 16 + v];
        g[d] = a * ((pos >> d) & 1u ? 1.0f : Q[d]);
      }
      store16(gq + (img * L + l) * C + h * 16, g);
    }
    if (part) {
      store16(st + tok * 2 * C + h * 16, Q);
      store16(st + tok * 2 * C + C + h * 16, gn);
      cv[tok * H + h] = gden;
    }
  }
  if (!part) return;   // (uniform: a kernel argument)
  __syncthreads();
  outer_partial<true>(st, cv, ntok, C, part, img, chunk, nchunk);
}

// backward, pass over S: gK and gV (either may be null) from gM | gks, one thread per (token, head)
__global__ __launch_bounds__(256) void attn_train_bwd_kv(const float* __restrict__ k, long long ldk, long long sk,
                                                         const float* __restrict__ v, long long ldv, long long sv,
                                                         const float* __restrict__ gkv, float* __restrict__ gk,
                                                         float* __restrict__ gv, int S, int C) {
  extern __shared__ __attribute__((aligned(16))) float sM[];   // [H][MLD]: gM | gks
  const int H = C >> 4;
  const long long img = blockIdx.y;
  load_block(sM, gkv, img, H);
  __syncthreads();
  const int tpb = 256 / H;
  const int h = threadIdx.x % H;
  const int s = blockIdx.x * tpb + threadIdx.x / H;
  if (s >= S || threadIdx.x >= tpb * H) return;
  const float fS = (float)S;
  const float* G = sM + h * MLD;
  float K[16];
  const unsigned pos = load_phi16(k + img * sk + (long long)s * ldk + h * 16, K);
  if (gk) {
    float V[16], g[16];
    const float* vrow = v + img * sv + (long long)s * ldv + h * 16;
#pragma unroll
    for (int d4 = 0; d4 < 4; ++d4) {
      const f32x4 x = *(const f32x4*)(vrow + d4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) V[d4 * 4 + e] = x[e] / fS;
    }
#pragma unroll
    for (int d = 0; d < 16; ++d) {
      float a = G[256 + d];
#pragma unroll
      for (int e = 0; e < 16; ++e) a += V[e] * G[d * 16 + e];
      g[d] = a * ((pos >> d) & 1u ? 1.0f : K[d]);
    }
    store16(gk + (img * S + s) * C + h * 16, g);
  }
  if (gv) {
    float g[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float a = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) a += K[d] * G[d * 16 + e];
      g[e] = a / fS;
    }
    store16(gv + (img * S + s) * C + h * 16, g);
  }
}

bool rows_ok(const float* p, long long ld, long long stride, int C) {
  return p && ((uintptr_t)p & 15) == 0 && ld >= C && ld % 4 == 0 && stride >= 0 && stride % 4 == 0;
}
bool dense_ok(const float* p) { return p && ((uintptr_t)p & 15) == 0; }
bool shape_ok(int nimg, int L, int S, int C) { return nimg > 0 && nimg <= 65535 && L > 0 && S > 0 && C > 0 && C % 16 == 0 && C <= 128; }
size_t stage_bytes(int C) { return (size_t)CHUNK * 2 * C * sizeof(float); }   // >= the 4 wave partials, 4 (C / 16) KVW floats
size_t block_bytes(int C) { return (size_t)(C / 16) * MLD * sizeof(float); }

}  // namespace

long long mk_linattn_train_work_floats(int nimg, int L, int S, int C) {
  if (!shape_ok(nimg, L, S, C)) return 0;
  const int n = L > S ? L : S;
  return (long long)nimg * (C / 16) * ((n + CHUNK - 1) / CHUNK) * KVW;
}

int mk_linattn_train_fwd(const float* q, long long ldq, long long sq, const float* k, long long ldk, long long sk, const float* v,
                         long long ldv, long long sv, float eps, float* out, float* kv, float* work, int nimg, int L, int S, int C,
                         mk_stream_t stream) {
  MK_CHECK_ARG(shape_ok(nimg, L, S, C), "mk_linattn_train_fwd: bad shape (nimg %d, L %d, S %d, C %d; C %% 16 == 0, C <= 128)", nimg, L, S, C);
  MK_CHECK_ARG(rows_ok(q, ldq, sq, C) && rows_ok(k, ldk, sk, C) && rows_ok(v, ldv, sv, C),
               "mk_linattn_train_fwd: q, k, v must be non-null, 16-byte aligned, with row strides >= C and all strides multiples of 4");
  MK_CHECK_ARG(dense_ok(out) && dense_ok(kv) && dense_ok(work), "mk_linattn_train_fwd: out, kv and work must be non-null and 16-byte aligned");
  const int H = C / 16, nchunk = (S + CHUNK - 1) / CHUNK;
  hipLaunchKernelGGL(attn_train_kv_partial, dim3(nchunk, nimg), dim3(256), stage_bytes(C), (hipStream_t)stream, k, ldk, sk, v, ldv, sv,
                     work, S, C, nchunk);
  MK_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_train_reduce, dim3(nimg * H), dim3(KVW), 0, (hipStream_t)stream, work, kv, nchunk);
  MK_CHECK_LAUNCH();
  const int tpb = 256 / H;
  hipLaunchKernelGGL(attn_train_apply, dim3((L + tpb - 1) / tpb, nimg), dim3(256), block_bytes(C), (hipStream_t)stream, q, ldq, sq, kv,
                     out, eps, L, S, C);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_linattn_train_bwd(const float* q, long long ldq, long long sq, const float* k, long long ldk, long long sk, const float* v,
                         long long ldv, long long sv, const float* kv, const float* go, float eps, float* work, float* gkv, float* gq,
                         float* gk, float* gv, int nimg, int L, int S, int C, mk_stream_t stream) {
  MK_CHECK_ARG(shape_ok(nimg, L, S, C), "mk_linattn_train_bwd: bad shape (nimg %d, L %d, S %d, C %d; C %% 16 == 0, C <= 128)", nimg, L, S, C);
  MK_CHECK_ARG(rows_ok(q, ldq, sq, C) && rows_ok(k, ldk, sk, C) && rows_ok(v, ldv, sv, C),
               "mk_linattn_train_bwd: q, k, v must be non-null, 16-byte aligned, with row strides >= C and all strides multiples of 4");
  MK_CHECK_ARG(dense_ok(kv) && dense_ok(go), "mk_linattn_train_bwd: kv and go must be non-null and 16-byte aligned");
  MK_CHECK_ARG((!gq || dense_ok(gq)) && (!gk || dense_ok(gk)) && (!gv || dense_ok(gv)), "mk_linattn_train_bwd: gq, gk, gv must be 16-byte aligned");
  const bool want_kv = gk || gv;
  MK_CHECK_ARG(!want_kv || (dense_ok(work) && dense_ok(gkv)), "mk_linattn_train_bwd: gk / gv need work and gkv (16-byte aligned)");
  if (!gq && !want_kv) return MK_OK;
  const int H = C / 16, nchunk = (L + CHUNK - 1) / CHUNK;
  const size_t lds = stage_bytes(C) + block_bytes(C) + (size_t)CHUNK * H * sizeof(float);
  static bool attr_done = false;   // benign race: the attribute call is idempotent
  if (!attr_done) {
    const int most = (int)(stage_bytes(128) + block_bytes(128) + (size_t)CHUNK * 8 * sizeof(float));
    hipError_t e = hipFuncSetAttribute((const void*)attn_train_bwd_q, hipFuncAttributeMaxDynamicSharedMemorySize, most);
    if (e != hipSuccess) {
      mk_set_error("mk_linattn_train_bwd: cannot reserve %d B of LDS: %s", most, hipGetErrorString(e));
      return MK_ERR_LAUNCH;
    }
    attr_done = true;
  }
  hipLaunchKernelGGL(attn_train_bwd_q, dim3(nchunk, nimg), dim3(256), lds, (hipStream_t)stream, q, ldq, sq, kv, go, eps, gq,
                     want_kv ? work : (float*)nullptr, L, S, C, nchunk);
  MK_CHECK_LAUNCH();
  if (!want_kv) return MK_OK;
  hipLaunchKernelGGL(attn_train_reduce, dim3(nimg * H), dim3(KVW), 0, (hipStream_t)stream, work, gkv, nchunk);
  MK_CHECK_LAUNCH();
  const int tpb = 256 / H;
  hipLaunchKernelGGL(attn_train_bwd_kv, dim3((S + tpb - 1) / tpb, nimg), dim3(256), block_bytes(C), (hipStream_t)stream, k, ldk, sk, v, ldv,
                     sv, gkv, gk, gv, S, C);
  MK_CHECK_LAUNCH();
  return MK_OK;
}
