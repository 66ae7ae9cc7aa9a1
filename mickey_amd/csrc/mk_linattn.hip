// mickey_amd -- every linear-attention kernel of the heads (reference att_layers/attention.py:46-64): inference on fp32 qkv rows,
// inference with the projections inside, and the trainable fp32 forward / backward.  Per image and head (D = 16 channels),
// phi(x) = elu(x) + 1, S = number of k / v tokens (inference: S = L):
//
//   forward   M[d, v] = sum_s phi(k)[s, d] (v[s, v] / S)      ks[d] = sum_s phi(k)[s, d]
//             den[l] = phi(q)[l] . ks + eps                   out[l, v] = (phi(q)[l] . M[:, v]) * (S / den[l])
//   backward  gnum[l, v] = gO[l, v] S / den[l]                gden[l] = -(gO[l] . out[l]) / den[l]      (out, den recomputed)
//             gQ[l, d] = (sum_v gnum[l, v] M[d, v] + gden[l] ks[d]) phi'(q[l, d])
//             gM[d, v] = sum_l phi(q)[l, d] gnum[l, v]        gks[d] = sum_l phi(q)[l, d] gden[l]
//             gK[s, d] = (sum_v (v[s, v] / S) gM[d, v] + gks[d]) phi'(k[s, d])
//             gV[s, v] = (sum_d phi(k)[s, d] gM[d, v]) / S
//
// M | ks of a head is one block of KVW = 272 floats (`kv`).  Both token sums (M | ks over S, gM | gks over L) are the SAME
// reduction -- sum_t A[t, d] (B[t, v] | c[t]) -- in the same order everywhere: chunks of KV_CHUNK tokens, within a chunk wave b
// sums tokens b, b + 4, ..., the four wave partials are added as ((0 + 1) + 2) + 3 (kv_chunk_partial, or the fused kernel's own
// token sets), the chunk partials in chunk order (linattn_kv_reduce).  No atomics: results are bit-identical from run to run and
// do not depend on the number of images in the call; the fused launches equal the unfused ones bit for bit.
//
//   pass                     inference, fp32 qkv rows   inference, projections inside   training
//   M | ks over S            linattn_kv_partial         linattn_kv_fused_kernel         attn_train_kv_partial
//   chunk partials -> block  linattn_kv_reduce          linattn_kv_reduce               linattn_kv_reduce (forward and backward)
//   out over L               linattn_apply_kernel       linattn_apply_fused_kernel      attn_train_apply
//   gQ, gM | gks over L                                                                 attn_train_bwd_q
//   gK, gV over S                                                                       attn_train_bwd_kv
//
// Inference multiplies v by the rounded 1 / L and fixes eps = 1e-6; training divides v by S and takes eps from the caller.
// None of this is FLOP-heavy (32 flops per loaded float): the kernels are written for few launches (training: 3 forward, 3
// backward, 2 / 1 when no gradient of k and v is wanted), coalesced 16-byte accesses and deterministic reductions.
#include "mk_common.hpp"
#include "mk_ln128.hpp"

namespace {
using namespace mk;

constexpr int KVW = 272;     // 16x16 KV + 16 Ksum per (group, image, head)
constexpr int KV_CHUNK = 64; // tokens per partial block (64 KiB of staged rows at C = 128; 32 measured the same here and doubled the reduce)
constexpr int MLD = 273;     // LDS row of one head's KV | Ksum block: heads land on different banks

__device__ __forceinline__ float phi(float x) { return x > 0.f ? x + 1.0f : expf(x); }  // elu(x) + 1; NaN stays NaN

// One token's contribution to a lane's 4 x NV block of a head's 16 x 16 KV sum (k4: 4 values of phi(k), vs: NV values of v / L,
// rounded) and to its 4 entries of Ksum, which take the token's weight c with HAS_C (the backward's gks; else c is not read and
// nothing is multiplied).  Every kernel that builds KV goes through here, whatever its lane layout.
template <int NV, bool HAS_C>
__device__ __forceinline__ void kv_outer(float (&acc)[4][NV], float (&ks)[4], const f32x4 k4, const float (&vs)[NV], const float c) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[a][e] += k4[a] * vs[e];
    ks[a] += HAS_C ? k4[a] * c : k4[a];
  }
}

// NV columns of the msg of one (token, head): Q = phi(q) of the head's 16 channels, kvat(d, v) / ksat(d) = the head's KV sum and
// Ksum wherever the caller keeps them (LDS, registers).  a[v] = (Q . KV[:, v]) * L / (Q . Ksum + eps), each dot product a chain over
// d = 0..15 in order, handed to put(v, a[v]); den = Q . Ksum + eps is returned.  Every kernel that applies KV goes through here.
template <int NV, typename KVAT, typename KSAT, typename PUT>
__device__ __forceinline__ float linattn_apply_cols(const float (&Q)[16], KVAT kvat, KSAT ksat, const int L, const float eps, PUT put) {
  float z = 0.f;
#pragma unroll
  for (int d = 0; d < 16; ++d) z += Q[d] * ksat(d);
  const float den = z + eps;
  const float scale = (float)L / den;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 16; ++d) s += Q[d] * kvat(d, v);
    s *= scale;
    put(v, s);
  }
  return den;
}

// chunk partial of  P[h][d * 16 + v] = sum_t A[t, h 16 + d] vop(B[t, h 16 + v]),  P[h][256 + d] = sum_t A[t, h 16 + d] c[t, h]
// from the staged rows st [KV_CHUNK][2C] (A | B) and cv [KV_CHUNK][H] (HAS_C; else c = 1) -> part [(img H + h) nchunk + chunk][KVW].
// Called by all 256 threads after a barrier behind the staging; st is reused for the wave partials.  ONE wave works on a token:
// lane = (head, half of v, quarter of d) holds a 4 x 8 block of the head's 16 x 16 outer product, 3 LDS reads (one broadcast
// within 8 lanes each) per 32 FMAs.  The block's 4 waves take every 4th token and their partial sums are combined in wave order.
template <bool HAS_C, typename VOP>
__device__ __forceinline__ void kv_chunk_partial(float* st, const float* cv, int ntok, int C, float* __restrict__ part, long long img,
                                                 int chunk, int nchunk, VOP vop) {
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
    for (int s = wave; s < ntok; s += 4) {
      const float* row = st + s * 2 * C + h * 16;
      const f32x4 k4 = *(const f32x4*)(row + dg * 4);
      const f32x4 v0 = *(const f32x4*)(row + C + vh * 8), v1 = *(const f32x4*)(row + C + vh * 8 + 4);
      const float v8[8] = {vop(v0[0]), vop(v0[1]), vop(v0[2]), vop(v0[3]), vop(v1[0]), vop(v1[1]), vop(v1[2]), vop(v1[3])};
      kv_outer<8, HAS_C>(acc, ks, k4, v8, HAS_C ? cv[s * H + h] : 0.f);
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

// chunk partials -> the [images x H][KVW] block, added in chunk order
__global__ __launch_bounds__(KVW) void linattn_kv_reduce(const float* __restrict__ part, float* __restrict__ kv, int nchunk) {
  const long long gih = blockIdx.x;
  const int t = threadIdx.x;
  float s = 0.f;
  for (int c = 0; c < nchunk; ++c) s += part[(gih * nchunk + c) * KVW + t];
  kv[gih * KVW + t] = s;
}

// one image's [H][KVW] blocks -> LDS rows of MLD floats
__device__ __forceinline__ void load_block(float* sM, const float* __restrict__ kv, long long img, int H) {
  for (int i = threadIdx.x; i < H * KVW; i += blockDim.x) sM[(i / KVW) * MLD + (i % KVW)] = kv[img * H * KVW + i];
}

// ---- inference on fp32 qkv rows [G, nimg * L, 3C] ---------------------------------------------------------------------------

// partial KV over a chunk of KV_CHUNK tokens for ALL heads of one (group, image) (C = 128: 8 heads of 16).
// The chunk's k and v rows (1 KiB per token, contiguous in the 3C-wide qkv row) are staged into LDS by LDS-DMA (no register
// round trip, everything in flight at once), phi() is applied to the k half in place (once per element), v / L is taken when the
// outer product reads the row (kv_chunk_partial)
// -- the first version had one thread per (head, d, half of v) read k and v straight from global memory: every v float4
// was requested by 16 lanes and every k by 2 (1 KiB of requests per 128 unique bytes), 2.4 TB/s.
__global__ __launch_bounds__(256) void linattn_kv_partial(const float* __restrict__ qkv, float* __restrict__ part, int L, int C,
                                                          int nchunk) {
  extern __shared__ __attribute__((aligned(16))) float skv[];   // [KV_CHUNK][2C]: phi(k) | v ; reused for the wave partials
  const long long gi = blockIdx.y;      // g*nimg + img
  const int chunk = blockIdx.x;
  const int t = threadIdx.x, wave = t >> 6;
  const int s0 = chunk * KV_CHUNK, ntok = min(L, s0 + KV_CHUNK) - s0;
  const float invL = 1.0f / (float)L;
  const float* base = qkv + (gi * (long long)L + s0) * 3 * C + C;   // k of the chunk's first token
  const int c4 = 2 * C / 4;                                          // float4 per token (k | v)
  // LDS-DMA, 16 B per lane: float4 i of the staged image <- token i / c4, column 4 (i % c4); a wave instruction fills 1 KiB
  // of LDS (one token at C = 128).  KV_CHUNK * c4 is a multiple of 256: nothing waits until all trips are issued.
  for (int it = 0; it < KV_CHUNK * c4 / 256; ++it) {
    const int i = it * 256 + t;
    const int s = min(i / c4, ntok - 1), c = (i % c4) * 4;
    glds16(base + (long long)s * 3 * C + c, (char*)skv + (it * 256 + wave * 64) * 16);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int i = t; i < ntok * (C / 4); i += 256) {   // phi() on the k half, in place, once per element
    const int s = i / (C / 4), c = (i - s * (C / 4)) * 4;
    f32x4 v = *(const f32x4*)(skv + s * 2 * C + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = phi(v[e]);
    *(f32x4*)(skv + s * 2 * C + c) = v;
  }
  __syncthreads();
  kv_chunk_partial<false>(skv, nullptr, ntok, C, part, gi, chunk, nchunk, [invL](float x) { return x * invL; });
}

// block = (256 / H) tokens x H heads of one (g, img), one thread per (token, head)
template <typename T>
__global__ __launch_bounds__(256) void linattn_apply_kernel(const float* __restrict__ qkv, const float* __restrict__ kv,
                                                            T* __restrict__ out, int ldo, int L, int C) {
  extern __shared__ __attribute__((aligned(16))) float skv[];  // [H][MLD]
  const int H = C >> 4;
  const long long gi = blockIdx.y;
  load_block(skv, kv, gi, H);
  __syncthreads();
  const int tpb = 256 / H;
  const int h = threadIdx.x % H;
  const int s = blockIdx.x * tpb + threadIdx.x / H;
  if (s >= L || threadIdx.x >= tpb * H) return;
  const float* qrow = qkv + (gi * L + s) * 3 * C + h * 16;
  float Q[16];
#pragma unroll
  for (int d4 = 0; d4 < 4; ++d4) {
    const f32x4 t4 = *(const f32x4*)(qrow + d4 * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) Q[d4 * 4 + e] = phi(t4[e]);
  }
  const float* K = skv + h * MLD;
  typename Lp<T>::V8 o0, o1;
  linattn_apply_cols<16>(Q, [&](int d, int v) { return K[d * 16 + v]; }, [&](int d) { return K[256 + d]; }, L, 1e-6f,
                         [&](int v, float a) { if (v < 8) o0[v] = (T)a; else o1[v - 8] = (T)a; });
  T* orow = out + (gi * L + s) * ldo + h * 16;
  *(typename Lp<T>::V8*)orow = o0;
  *(typename Lp<T>::V8*)(orow + 8) = o1;
}

// ---- inference with its projections inside (C = 128, 16-bit operands) ------------------------------------------------
// As separate launches a layer writes q | k | v in fp32 (762 MB at 4 x 124 k rows) and reads them straight back, and msg makes the
// same round trip in 16 bit -- although k and v only feed a 16 x 16 sum per head, and q only the apply.  The two kernels below
// compute the projections themselves, as gemm_ln128_kernel does: the group's W rows stay on chip (LDS, chunk-swizzled, or a wave's
// registers), a wave takes the activations of 16 tokens from global memory straight into MFMA B-operand registers and visits the K
// steps in order, so that its accumulators are mk_gemm_grouped's bit for bit; everything after them goes through the inline functions
// the unfused kernels use.
// A wave's accumulators hold 4 consecutive features of a token per lane; the consumers want other layouts (all of a token's k and v
// for the outer product, a head's 16 q per token, a B operand for the merge) -- every hand-over goes through a piece of LDS that
// belongs to the wave alone (DS operations of a wave execute in order: no workgroup barrier).
constexpr int FC = 128;   // the only width these kernels exist for

template <typename T, int ROWS>
__device__ __forceinline__ void w_rows_to_lds(const T* __restrict__ Wg, const int ldw, char* dst, const int tid, const int nthr) {
  for (int i = tid; i < ROWS * 16; i += nthr) {   // 16-byte chunks, a W row's 16 chunks (K = 128) consecutive
    const int c = i & 3, st = (i >> 2) & 3, n = i >> 4;
    const uint4 v = *(const uint4*)(Wg + (long long)n * ldw + st * 32 + c * 8);
    *(uint4*)(dst + ((st * ROWS + n) * 64 + ((c ^ ((n >> 2) & 3)) << 4))) = v;
  }
}
template <typename T, int ROWS>
__device__ __forceinline__ typename Lp<T>::V8 w_frag(const char* w, const int st, const int n, const int q) {
  return *(const typename Lp<T>::V8*)(w + ((st * ROWS + n) * 64 + ((q ^ ((n >> 2) & 3)) << 4)));
}

// k | v projection + the per-chunk partial KV of mk_linattn_kv in one kernel (the unchanged linattn_kv_reduce follows).
//   workgroup = 4 waves walking chunks of KV_CHUNK tokens of one (group, image); wave w owns heads 2w and 2w + 1 for ALL of the
//   chunk's tokens: the 64 rows of qkv_w it needs (k and v of its two heads) stay in its registers as 16 MFMA A fragments -- no W in
//   LDS, no workgroup barrier anywhere.  linattn_kv_partial's wave b sums tokens b, b + 4, ... and the four wave partials are combined
//   as ((0 + 1) + 2) + 3; here the wave takes those four token sets one after the other (block b: 16 B-operand rows = tokens b,
//   b + 4, ...), each into accumulators of its own, and combines the four in the same order.  Per block: 16 MFMAs give k | v of the
//   head pair for the 16 tokens, phi() on k and 1 / L on v, through 4 KiB of staging that belongs to the wave into the outer
//   product (lane = (head of the pair, 2 columns of v, 4 of d)).  (First version: all heads per wave with W_k | W_v in LDS, two heads
//   at a time, partials combined through LDS with two barriers per head pair: 185 us per layer against 344 for the launches it replaces.)
template <typename T>
__global__ __launch_bounds__(256, 2) void linattn_kv_fused_kernel(const T* __restrict__ X, int lda, long long strideX,
                                                                  const T* __restrict__ Wqkv, int ldw, long long strideW,
                                                                  float* __restrict__ part, int nimg, int L, int nchunk) {
  using V8 = typename Lp<T>::V8;
  __shared__ __attribute__((aligned(16))) float stage[4 * 1024];   // [4 waves][16 tokens][64 floats]
  constexpr int H = FC / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long gi = blockIdx.y;   // g * nimg + img
  const int g = (int)(gi / nimg), img = (int)(gi % nimg);
  float* stg = stage + wave * 1024;
  const int r16 = lane & 15, q = lane >> 4;
  const int hp = lane >> 5, vg = (lane >> 2) & 7, dg = lane & 3;
  const float invL = 1.0f / (float)L;
  V8 wf[4][4];   // [K step][k of head 2w, k of head 2w + 1, v of head 2w, v of head 2w + 1]: row r16 of the 16, K chunk q
  {
    const T* Wg = Wqkv + (long long)g * strideW + q * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = FC + (j >> 1) * FC + wave * 32 + (j & 1) * 16 + r16;
#pragma unroll
      for (int st = 0; st < 4; ++st) wf[st][j] = *(const V8*)(Wg + (long long)n * ldw + st * 32);
    }
  }
  const T* xi = X + (long long)g * strideX + (long long)img * L * lda + q * 8;
  auto load_x = [&](int first, V8(&xf)[4]) {   // tokens first + 4 * r16 (clamped: rows past L are never summed)
    const int s = min(first + 4 * r16, L - 1);
#pragma unroll
    for (int st = 0; st < 4; ++st) xf[st] = *(const V8*)(xi + (long long)s * lda + st * 32);
  };
  V8 xf[4], xn[4];
  int chunk = blockIdx.x;
  if (chunk < nchunk) load_x(chunk * KV_CHUNK, xf);
  for (; chunk < nchunk; chunk += gridDim.x) {
    const int ntok = min(L, (chunk + 1) * KV_CHUNK) - chunk * KV_CHUNK;
    float acc[4][4][2], ks[4][4];   // [token set b]
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int a = 0; a < 4; ++a) acc[b][a][0] = acc[b][a][1] = ks[b][a] = 0.f;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      f32x4 kvq[4];   // features 4q .. 4q + 3 of token b + 4 r16
#pragma unroll
      for (int j = 0; j < 4; ++j) kvq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int j = 0; j < 4; ++j) kvq[j] = Lp<T>::mma16(wf[st][j], xf[st], kvq[j]);
      // the next 16 rows travel while these are summed: the chunk's next token set, or the next chunk's first
#pragma unroll
      for (int st = 0; st < 4; ++st) xn[st] = xf[st];
      if (b < 3) load_x(chunk * KV_CHUNK + b + 1, xn);
      else if (chunk + (int)gridDim.x < nchunk) load_x((chunk + gridDim.x) * KV_CHUNK, xn);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          kvq[j][e] = phi(kvq[j][e]);
          kvq[2 + j][e] = kvq[2 + j][e] * invL;   // v / L once per element (the outer product takes it rounded)
        }
      // staged row of a token: 16 chunks of 4 floats, k (2 x 16) | v (2 x 16), chunk c at c ^ slot
#pragma unroll
      for (int j = 0; j < 4; ++j) *(f32x4*)(stg + r16 * 64 + (((j * 4 + q) ^ r16) << 2)) = kvq[j];
      __builtin_amdgcn_wave_barrier();
      auto token = [&](const int t) {
        const f32x4 k4 = *(const f32x4*)(stg + t * 64 + (((hp * 4 + dg) ^ t) << 2));
        const float2 v2 = *(const float2*)(stg + t * 64 + (((8 + hp * 4 + (vg >> 1)) ^ t) << 2) + (vg & 1) * 2);
        const float vs[2] = {v2.x, v2.y};
        kv_outer<2, false>(acc[b], ks[b], k4, vs, 0.f);
      };
      if (ntok == KV_CHUNK) {   // straight-line: the 32 staged reads are in flight together
#pragma unroll
        for (int t = 0; t < 16; ++t) token(t);
      } else {                  // the image's last chunk: tokens b, b + 4, ... < ntok
#pragma unroll 1
        for (int t = 0; b + 4 * t < ntok; ++t) token(t);
      }
      __builtin_amdgcn_wave_barrier();   // (the staged rows are rewritten by the next token set: DS operations execute in order)
#pragma unroll
      for (int st = 0; st < 4; ++st) xf[st] = xn[st];
    }
    float* o = part + (((gi * H + 2 * wave + hp) * nchunk) + chunk) * KVW;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float2 r;
      r.x = ((acc[0][a][0] + acc[1][a][0]) + acc[2][a][0]) + acc[3][a][0];
      r.y = ((acc[0][a][1] + acc[1][a][1]) + acc[2][a][1]) + acc[3][a][1];
      *(float2*)(o + (dg * 4 + a) * 16 + vg * 2) = r;
    }
    if (vg == 0) {
      f32x4 r;
#pragma unroll
      for (int a = 0; a < 4; ++a) r[a] = ((ks[0][a] + ks[1][a]) + ks[2][a]) + ks[3][a];
      *(f32x4*)(o + 256 + dg * 4) = r;
    }
  }
}

// q projection + mk_linattn_apply (+ merge -> norm1, the K = 128 form of mk_gemm_ln128) in one kernel.
//   workgroup = 8 waves of one (group, image): rows 0..C of qkv_w and merge_w in LDS (32 KiB each) + 8 KiB of staging per wave; a
//   lane keeps the 16 x 4 block of its head's KV sum (and Ksum) in registers for the whole image: lane = (token parity, head, 4
//   columns of v).  A wave takes 16 tokens at a time: q accumulators, phi(), staged so that a lane reads the 16 q of its head for
//   every other token, the apply (linattn_apply_cols), msg rounded to T and staged as the B operand of the merge MFMAs (MERGE; else
//   msg is written to `out` and mk_gemm_ln128 follows), LayerNorm in the accumulators as in gemm_ln128_kernel.
//   X and out may be the two column halves of the same rows: neither is __restrict__.
template <typename T, bool MERGE>
__global__ __launch_bounds__(512) void linattn_apply_fused_kernel(const T* X, int lda, long long strideX, const T* __restrict__ Wqkv,
                                                                  int ldw, long long strideW, const float* __restrict__ kv,
                                                                  const T* __restrict__ Wm, int ldwm, long long strideWm,
                                                                  const float* __restrict__ lnw, const float* __restrict__ lnb, float eps,
                                                                  T* out, int ldo, long long strideO, int nimg, int L) {
  using V8 = typename Lp<T>::V8;
  using V4 = typename Lp<T>::V4;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // W_q | merge_w: [4 K steps][128 rows][64 B] each | ln weight, bias | staging [8 waves][8 KiB]
  constexpr int H = FC / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long gi = blockIdx.y;
  const int g = (int)(gi / nimg), img = (int)(gi % nimg);
  char* swm = smem + FC * FC * 2;
  float* slw = (float*)(smem + 2 * FC * FC * 2);
  float* slb = slw + FC;
  w_rows_to_lds<T, FC>(Wqkv + (long long)g * strideW, ldw, smem, tid, 512);
  if (MERGE) {
    w_rows_to_lds<T, FC>(Wm + (long long)g * strideWm, ldwm, swm, tid, 512);
    if (tid < FC) {
      slw[tid] = lnw[g * FC + tid];
      slb[tid] = lnb[g * FC + tid];
    }
  }
  __syncthreads();
  float* stq = (float*)(smem + 2 * FC * FC * 2 + 1024) + wave * 2048;
  const int r16 = lane & 15, q = lane >> 4;
  const int par = lane >> 5, h = (lane >> 2) & 7, vg = lane & 3;
  f32x4 kreg[16], ksum[4];   // KV[d][4 vg .. 4 vg + 3] and Ksum of head h
  {
    const float* kp = kv + (gi * H + h) * KVW;
#pragma unroll
    for (int d = 0; d < 16; ++d) kreg[d] = *(const f32x4*)(kp + d * 16 + vg * 4);
#pragma unroll
    for (int d4 = 0; d4 < 4; ++d4) ksum[d4] = *(const f32x4*)(kp + 256 + d4 * 4);
  }
  const int ntile = (L + 15) >> 4, step = gridDim.x * 8;
  const T* xi = X + (long long)g * strideX + (long long)img * L * lda + q * 8;
  T* oi = out + (long long)g * strideO + (long long)img * L * ldo;
  V8 xf[4];
  auto load_x = [&](int tile) {
    const int s = min(tile * 16 + r16, L - 1);
#pragma unroll
    for (int st = 0; st < 4; ++st) xf[st] = *(const V8*)(xi + (long long)s * lda + st * 32);
  };
  int tile = blockIdx.x * 8 + wave;
  if (tile < ntile) load_x(tile);
  for (; tile < ntile; tile += step) {
    f32x4 acc[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int f = 0; f < 8; ++f) acc[f] = Lp<T>::mma16(w_frag<T, FC>(smem, st, f * 16 + r16, q), xf[st], acc[f]);
    if (tile + step < ntile) load_x(tile + step);
    // phi(q) of token r16, features f * 16 + 4 q .. + 3 -> staged row r16 (32 chunks of 4 floats; chunk c at c ^ r16 ^ (c >> 4) * 2:
    // writes of 16 rows and reads of 8 heads both spread over the banks)
#pragma unroll
    for (int f = 0; f < 8; ++f) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[f][e] = phi(acc[f][e]);
      const int c = f * 4 + q;
      *(f32x4*)(stq + r16 * 128 + ((c ^ r16 ^ ((c >> 4) << 1)) << 2)) = acc[f];
    }
    __builtin_amdgcn_wave_barrier();
    V4 msg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t = 2 * i + par;
      float Q[16];
#pragma unroll
      for (int d4 = 0; d4 < 4; ++d4) {
        const int c = h * 4 + d4;
        const f32x4 t4 = *(const f32x4*)(stq + t * 128 + ((c ^ t ^ ((c >> 4) << 1)) << 2));
#pragma unroll
        for (int e = 0; e < 4; ++e) Q[d4 * 4 + e] = t4[e];
      }
      linattn_apply_cols<4>(Q, [&](int d, int v) { return kreg[d][v]; }, [&](int d) { return ksum[d >> 2][d & 3]; }, L, 1e-6f,
                            [&](int v, float a) { msg[i][v] = (T)a; });
      if constexpr (!MERGE) {
        const int s = tile * 16 + t;
        if (s < L) *(V4*)(oi + (long long)s * ldo + h * 16 + vg * 4) = msg[i];
      }
    }
    if constexpr (MERGE) {
      __builtin_amdgcn_wave_barrier();
      // msg as the merge's B operand: rows of 128 T (16 chunks of 16 B, chunk c at c ^ token), over the q rows (all read by now)
      char* stm = (char*)stq;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int t = 2 * i + par;
        *(V4*)(stm + t * 256 + (((h * 2 + (vg >> 1)) ^ t) << 4) + (vg & 1) * 8) = msg[i];
      }
      __builtin_amdgcn_wave_barrier();
      V8 mf[4];
#pragma unroll
      for (int st = 0; st < 4; ++st) mf[st] = *(const V8*)(stm + r16 * 256 + (((st * 4 + q) ^ r16) << 4));
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int f = 0; f < 8; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int f = 0; f < 8; ++f) acc[f] = Lp<T>::mma16(w_frag<T, FC>(swm, st, f * 16 + r16, q), mf[st], acc[f]);
      const float rstd = ln128_centre(acc, eps);
      const int s = tile * 16 + r16;
      if (s < L) {
#pragma unroll
        for (int f = 0; f < 8; ++f) {
          const int fe = f * 16 + q * 4;
          const f32x4 y = ln128_affine(acc[f], rstd, *(const f32x4*)(slw + fe), *(const f32x4*)(slb + fe));
          V4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (T)y[e];
          *(V4*)(oi + (long long)s * ldo + fe) = o;
        }
      }
    }
  }
}

template <typename T>
hipError_t launch_apply_fused(bool merge, dim3 grid, int lds, hipStream_t st, const void* x, int lda, long long strideX,
                                     const void* qkv_w, int ldw, long long strideW, const float* kv, const void* merge_w, int ldwm,
                                     long long strideWm, const float* ln_w, const float* ln_b, float eps, void* out, int ldo,
                                     long long strideOut, int nimg, int L) {
  static bool done[2] = {false, false};
  const void* fn = merge ? (const void*)linattn_apply_fused_kernel<T, true> : (const void*)linattn_apply_fused_kernel<T, false>;
  if (!done[merge]) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    done[merge] = true;
  }
  if (merge)
    hipLaunchKernelGGL((linattn_apply_fused_kernel<T, true>), grid, dim3(512), lds, st, (const T*)x, lda, strideX, (const T*)qkv_w, ldw,
                       strideW, kv, (const T*)merge_w, ldwm, strideWm, ln_w, ln_b, eps, (T*)out, ldo, strideOut, nimg, L);
  else
    hipLaunchKernelGGL((linattn_apply_fused_kernel<T, false>), grid, dim3(512), lds, st, (const T*)x, lda, strideX, (const T*)qkv_w, ldw,
                       strideW, kv, (const T*)merge_w, ldwm, strideWm, ln_w, ln_b, eps, (T*)out, ldo, strideOut, nimg, L);
  return hipSuccess;
}

// ---- training: fp32 q [N, L, C], k, v [N, S, C] as three strided operands ---------------------------------------------------

// forward, pass over S: stages phi(k) | v / S of one chunk of one image, then the partial M | ks of every head
__global__ __launch_bounds__(256) void attn_train_kv_partial(const float* __restrict__ k, long long ldk, long long sk,
                                                             const float* __restrict__ v, long long ldv, long long sv,
                                                             float* __restrict__ part, int S, int C, int nchunk) {
  extern __shared__ __attribute__((aligned(16))) float st[];   // [KV_CHUNK][2C]
  const long long img = blockIdx.y;
  const int chunk = blockIdx.x, t = threadIdx.x;
  const int s0 = chunk * KV_CHUNK, ntok = min(S, s0 + KV_CHUNK) - s0;
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
  kv_chunk_partial<false>(st, nullptr, ntok, C, part, img, chunk, nchunk, [](float x) { return x; });
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
  float Q[16], o[16];
  load_phi16(q + img * sq + (long long)l * ldq + h * 16, Q);
  const float* M = sM + h * MLD;
  linattn_apply_cols<16>(Q, [&](int d, int v) { return M[d * 16 + v]; }, [&](int d) { return M[256 + d]; }, S, eps,
                         [&](int v, float a) { o[v] = a; });
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
  float* st = sm;                       // [KV_CHUNK][2C]: phi(q) | gnum
  float* sM = sm + KV_CHUNK * 2 * C;    // [H][MLD]
  float* cv = sM + H * MLD;             // [KV_CHUNK][H]: gden
  const long long img = blockIdx.y;
  const int chunk = blockIdx.x, t = threadIdx.x;
  const int l0 = chunk * KV_CHUNK, ntok = min(L, l0 + KV_CHUNK) - l0;
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
    float dot = 0.f;   // gO . out
    const float den = linattn_apply_cols<16>(Q, [&](int d, int v) { return M[d * 16 + v]; }, [&](int d) { return M[256 + d]; }, S, eps,
                                             [&](int v, float o) { dot += G[v] * o; });
    const float r = (float)S / den;
#pragma unroll
    for (int v = 0; v < 16; ++v) gn[v] = G[v] * r;
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
  kv_chunk_partial<true>(st, cv, ntok, C, part, img, chunk, nchunk, [](float x) { return x; });
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

// ---- host side ---------------------------------------------------------------------------------------------------------------

int chunks_of(int ntok) { return (ntok + KV_CHUNK - 1) / KV_CHUNK; }
// the chunk partials of `images` images of ntok tokens each
long long work_floats(long long images, int ntok, int C) { return images * (C / 16) * chunks_of(ntok) * KVW; }
size_t stage_bytes(int C) { return (size_t)KV_CHUNK * 2 * C * sizeof(float); }   // >= the 4 wave partials, 4 (C / 16) KVW floats
size_t block_bytes(int C) { return (size_t)(C / 16) * MLD * sizeof(float); }

void launch_kv_reduce(const float* work, float* kv, int blocks, int nchunk, hipStream_t st) {
  hipLaunchKernelGGL(linattn_kv_reduce, dim3(blocks), dim3(KVW), 0, st, work, kv, nchunk);
}

bool rows_ok(const float* p, long long ld, long long stride, int C) {
  return p && ((uintptr_t)p & 15) == 0 && ld >= C && ld % 4 == 0 && stride >= 0 && stride % 4 == 0;
}
bool dense_ok(const float* p) { return p && ((uintptr_t)p & 15) == 0; }
bool shape_ok(int nimg, int L, int S, int C) { return nimg > 0 && nimg <= 65535 && L > 0 && S > 0 && C > 0 && C % 16 == 0 && C <= 128; }

}  // namespace

extern "C" {

long long mk_linattn_work_floats(int groups, int nimg, int L, int C) { return work_floats((long long)groups * nimg, L, C); }

int mk_linattn_kv(const float* qkv, float* kv, float* work, int groups, int nimg, int L, int C, mk_stream_t stream) {
  MK_CHECK_ARG(qkv && kv && work && groups > 0 && nimg > 0 && L > 0 && C % 16 == 0 && C <= 128, "mk_linattn_kv: bad args (C <= 128)");
  const int nchunk = chunks_of(L);
  hipLaunchKernelGGL(linattn_kv_partial, dim3(nchunk, groups * nimg), dim3(256), stage_bytes(C), (hipStream_t)stream, qkv, work, L, C,
                     nchunk);
  MK_CHECK_LAUNCH();
  launch_kv_reduce(work, kv, groups * nimg * (C / 16), nchunk, (hipStream_t)stream);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_linattn_apply(const float* qkv, const float* kv, void* out, int ldo, int groups, int nimg, int L, int C, int dtype,
                     mk_stream_t stream) {
  const int H = C / 16;
  MK_CHECK_ARG(qkv && kv && out && groups > 0 && nimg > 0 && L > 0 && C > 0 && C % 16 == 0 && C <= 128 && ldo % 8 == 0 && ldo >= C,
               "mk_linattn_apply: bad args (C <= 128, as mk_linattn_kv)");
  const int tpb = 256 / H;
  dim3 grid((L + tpb - 1) / tpb, groups * nimg);
  const size_t lds = block_bytes(C);
  if (dtype == MK_BF16)
    hipLaunchKernelGGL(linattn_apply_kernel<__bf16>, grid, dim3(256), lds, (hipStream_t)stream, qkv, kv, (__bf16*)out, ldo, L,
                       C);
  else if (dtype == MK_F16)
    hipLaunchKernelGGL(linattn_apply_kernel<_Float16>, grid, dim3(256), lds, (hipStream_t)stream, qkv, kv, (_Float16*)out,
                       ldo, L, C);
  else
    hipLaunchKernelGGL(linattn_apply_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, qkv, kv, (float*)out, ldo, L, C);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_linattn_kv_fused(const void* x, int lda, long long strideX, const void* qkv_w, int ldw, long long strideW, float* kv,
                        float* work, int groups, int nimg, int L, int C, int dtype, mk_stream_t stream) {
  MK_CHECK_ARG(x && qkv_w && kv && work, "mk_linattn_kv_fused: null pointer");
  MK_CHECK_ARG(C == FC && (dtype == MK_BF16 || dtype == MK_F16), "mk_linattn_kv_fused: C = 128 and 16-bit operands only");
  MK_CHECK_ARG(groups > 0 && nimg > 0 && L > 0 && lda % 8 == 0 && lda >= C && ldw % 8 == 0 && ldw >= C && strideX % 8 == 0 &&
                   strideW % 8 == 0 && (((uintptr_t)x | (uintptr_t)qkv_w | (uintptr_t)work) & 15) == 0,
               "mk_linattn_kv_fused: bad geometry (rows of 8-element multiples, 16-byte aligned)");
  const int nchunk = chunks_of(L);
  const int gi = groups * nimg;
  // about eight workgroups per CU in all: a wave loads its W fragments once, then walks its workgroup's share of the image's chunks
  int per_img = (8 * mk::gemm::num_cus() + gi - 1) / gi;
  if (per_img > nchunk) per_img = nchunk;
  if (dtype == MK_BF16)
    hipLaunchKernelGGL(linattn_kv_fused_kernel<__bf16>, dim3(per_img, gi), dim3(256), 0, (hipStream_t)stream, (const __bf16*)x, lda,
                       strideX, (const __bf16*)qkv_w, ldw, strideW, work, nimg, L, nchunk);
  else
    hipLaunchKernelGGL(linattn_kv_fused_kernel<_Float16>, dim3(per_img, gi), dim3(256), 0, (hipStream_t)stream, (const _Float16*)x,
                       lda, strideX, (const _Float16*)qkv_w, ldw, strideW, work, nimg, L, nchunk);
  MK_CHECK_LAUNCH();
  launch_kv_reduce(work, kv, gi * (C / 16), nchunk, (hipStream_t)stream);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_linattn_apply_fused(const void* x, int lda, long long strideX, const void* qkv_w, int ldw, long long strideW, const float* kv,
                           const void* merge_w, int ldwm, long long strideWm, const float* ln_w, const float* ln_b, float eps,
                           void* out, int ldo, long long strideOut, int groups, int nimg, int L, int C, int dtype,
                           mk_stream_t stream) {
  MK_CHECK_ARG(x && qkv_w && kv && out, "mk_linattn_apply_fused: null pointer");
  MK_CHECK_ARG(C == FC && (dtype == MK_BF16 || dtype == MK_F16), "mk_linattn_apply_fused: C = 128 and 16-bit operands only");
  MK_CHECK_ARG(!merge_w || (ln_w && ln_b && ldwm % 8 == 0 && ldwm >= C && strideWm % 8 == 0 && ((uintptr_t)merge_w & 15) == 0),
               "mk_linattn_apply_fused: merge_w comes with ln_w, ln_b and 16-byte aligned rows");
  MK_CHECK_ARG(groups > 0 && nimg > 0 && L > 0 && lda % 8 == 0 && lda >= C && ldw % 8 == 0 && ldw >= C && ldo % 4 == 0 && ldo >= C &&
                   strideX % 8 == 0 && strideW % 8 == 0 && strideOut % 4 == 0 && (((uintptr_t)x | (uintptr_t)qkv_w | (uintptr_t)kv) & 15) == 0 &&
                   ((uintptr_t)out & 7) == 0,
               "mk_linattn_apply_fused: bad geometry (rows of 8-element multiples, 16-byte aligned; out 8-byte aligned)");
  const int ntile = (L + 127) / 128;   // 8 waves x 16 tokens
  const int gi = groups * nimg;
  int per_img = (mk::gemm::num_cus() + gi - 1) / gi;   // one workgroup of 8 waves per CU
  if (per_img > ntile) per_img = ntile;
  const int lds = 2 * FC * FC * 2 + 1024 + 8 * 8192;
  const dim3 grid(per_img, gi);
  const hipError_t e = dtype == MK_BF16
      ? launch_apply_fused<__bf16>(merge_w != nullptr, grid, lds, (hipStream_t)stream, x, lda, strideX, qkv_w, ldw, strideW, kv, merge_w,
                                   ldwm, strideWm, ln_w, ln_b, eps, out, ldo, strideOut, nimg, L)
      : launch_apply_fused<_Float16>(merge_w != nullptr, grid, lds, (hipStream_t)stream, x, lda, strideX, qkv_w, ldw, strideW, kv, merge_w,
                                     ldwm, strideWm, ln_w, ln_b, eps, out, ldo, strideOut, nimg, L);
  if (e != hipSuccess) { mk_set_error("mk_linattn_apply_fused: cannot reserve %d B of LDS: %s", lds, hipGetErrorString(e)); return MK_ERR_LAUNCH; }
  MK_CHECK_LAUNCH();
  return MK_OK;
}

long long mk_linattn_train_work_floats(int nimg, int L, int S, int C) {
  if (!shape_ok(nimg, L, S, C)) return 0;
  return work_floats(nimg, L > S ? L : S, C);
}

int mk_linattn_train_fwd(const float* q, long long ldq, long long sq, const float* k, long long ldk, long long sk, const float* v,
                         long long ldv, long long sv, float eps, float* out, float* kv, float* work, int nimg, int L, int S, int C,
                         mk_stream_t stream) {
  MK_CHECK_ARG(shape_ok(nimg, L, S, C), "mk_linattn_train_fwd: bad shape (nimg %d, L %d, S %d, C %d; C %% 16 == 0, C <= 128)", nimg, L, S, C);
  MK_CHECK_ARG(rows_ok(q, ldq, sq, C) && rows_ok(k, ldk, sk, C) && rows_ok(v, ldv, sv, C),
               "mk_linattn_train_fwd: q, k, v must be non-null, 16-byte aligned, with row strides >= C and all strides multiples of 4");
  MK_CHECK_ARG(dense_ok(out) && dense_ok(kv) && dense_ok(work), "mk_linattn_train_fwd: out, kv and work must be non-null and 16-byte aligned");
  const int H = C / 16, nchunk = chunks_of(S);
  hipLaunchKernelGGL(attn_train_kv_partial, dim3(nchunk, nimg), dim3(256), stage_bytes(C), (hipStream_t)stream, k, ldk, sk, v, ldv, sv,
                     work, S, C, nchunk);
  MK_CHECK_LAUNCH();
  launch_kv_reduce(work, kv, nimg * H, nchunk, (hipStream_t)stream);
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
  const int H = C / 16, nchunk = chunks_of(L);
  const size_t lds = stage_bytes(C) + block_bytes(C) + (size_t)KV_CHUNK * H * sizeof(float);
  static bool attr_done = false;   // benign race: the attribute call is idempotent
  if (!attr_done) {
    const int most = (int)(stage_bytes(128) + block_bytes(128) + (size_t)KV_CHUNK * 8 * sizeof(float));
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
  launch_kv_reduce(work, gkv, nimg * H, nchunk, (hipStream_t)stream);
  MK_CHECK_LAUNCH();
  const int tpb = 256 / H;
  hipLaunchKernelGGL(attn_train_bwd_kv, dim3((S + tpb - 1) / tpb, nimg), dim3(256), block_bytes(C), (hipStream_t)stream, k, ldk, sk, v, ldv,
                     sv, gkv, gk, gv, S, C);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

}  // extern "C"
