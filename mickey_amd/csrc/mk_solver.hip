// mickey_amd -- the pose solver of the probabilistic-Procrustes RANSAC on gfx950
// (reference lib/models/MicKey/modules/utils/probabilisticProcrustes.py:183-348).
//
// The reference tiles X/Y 100x for its inner torch.multinomial; the outer one (the exponential-race top-k that picks the
// correspondence sets) is mk_sampler.hip.  Here:
//   * mk_gather_backproject(_kf, _pairs, _bwd): the sampled cells -> 3D correspondences X, Y and their weights.
//   * mk_ransac_hypotheses: a correspondence set (X, Y, w: 56 KB) is staged once in LDS and shared by
//     all its hypotheses; a hypothesis draws its 3 correspondences ~ w without replacement with three uniforms (prefix
//     sums of the set's weights in LDS, binary search with the chosen ones masked out = the top-3 of an exponential race,
//     which the injected-noise path still runs), 3x3 Kabsch via one-sided Jacobi SVD in fp64 (one per lane, no MFMA), soft
//     inlier count by wave64 reduction.
//   * mk_refine_pose: one workgroup per pair: arg-max, <= 4 masked-Kabsch refits with the reference's
//     per-pair early exit, final confidence.  No host synchronisation anywhere.
//   * mk_train_ransac_masks / mk_reinforce_scatter: the training-time RANSAC of loss/loss_class.py (8-point hypotheses,
//     refinement of every hypothesis, REINFORCE bookkeeping); its differentiable tail is mk_train_tail.hip.
// The rigid-fit arithmetic itself (Jacobi sweeps, Procrustes moments, residuals) is mk_procrustes.hpp, shared with the tail.
// Noise can be INJECTED (fp32 Exp(1) tensors / explicit indices) so that tests are bit-comparable
// with torch; the product path uses Philox4x32-10 (mk_philox.hpp).
#include "mk_common.hpp"

#pragma clang fp contract(off)  // keep dist, sigmoid, key arithmetic un-fused: comparable with ATen

// (after the pragma: the shared arithmetic compiles un-fused here -- see the head of mk_procrustes.hpp)
#include "mk_philox.hpp"
#include "mk_procrustes.hpp"

namespace {
using namespace mk;

// ---- gather + back-projection -----------------------------------------------------------------------
__device__ __forceinline__ void inv3(const float* K, float* o) {
  const float a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
  const float A = e * i - f * h, Bc = -(d * i - f * g), Cc = d * h - e * g;
  const float det = a * A + b * Bc + c * Cc;
  const float id = 1.0f / det;
  o[0] = A * id; o[1] = -(b * i - c * h) * id; o[2] = (b * f - c * e) * id;
  o[3] = Bc * id; o[4] = (a * i - c * g) * id; o[5] = -(a * f - c * d) * id;
  o[6] = Cc * id; o[7] = -(a * h - b * g) * id; o[8] = (a * e - b * d) * id;
}

// MAP (mk_common.hpp: pair_rows): pair b reads row b0 of kps0 / dep0 and row b1 of kps1 / dep1 (keyframe mode: operand 0 through
// idx0; pair-list mode: a map on each side; chosen on the host by with_row_map, mk_common.hpp); K0 / K1 stay per pair
template <int MAP>
__global__ __launch_bounds__(256) void gather_backproject_kernel(const int* __restrict__ idx, const float* __restrict__ fs,
                                                                 const float* __restrict__ kps0, const float* __restrict__ dep0,
                                                                 const float* __restrict__ kps1, const float* __restrict__ dep1,
                                                                 const float* __restrict__ K0, const float* __restrict__ K1,
                                                                 float* __restrict__ X, float* __restrict__ Y,
                                                                 float* __restrict__ wts, float* __restrict__ corr,
                                                                 int rows_per_pair, int k, int n0, int n1,
                                                                 const int* __restrict__ idx0, int N0, const int* __restrict__ idx1,
                                                                 int N1) {
  const int r = blockIdx.y, b = r / rows_per_pair;
  int b0, b1;
  if (!pair_rows<MAP>(idx0, N0, idx1, N1, b, b0, b1)) return;
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= k) return;
  float Ki0[9], Ki1[9];
  inv3(K0 + b * 9, Ki0);
  inv3(K1 + b * 9, Ki1);
  const int c = idx[(long long)r * k + s];
  const int i = c / n1, j = c - i * n1;
  const float u0 = kps0[((long long)b0 * 2 + 0) * n0 + i], v0 = kps0[((long long)b0 * 2 + 1) * n0 + i], d0 = dep0[(long long)b0 * n0 + i];
  const float u1 = kps1[((long long)b1 * 2 + 0) * n1 + j], v1 = kps1[((long long)b1 * 2 + 1) * n1 + j], d1 = dep1[(long long)b1 * n1 + j];
  const long long o = (long long)r * k + s;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    X[o * 3 + a] = d0 * (Ki0[a * 3 + 0] * u0 + Ki0[a * 3 + 1] * v0 + Ki0[a * 3 + 2]);
    Y[o * 3 + a] = d1 * (Ki1[a * 3 + 0] * u1 + Ki1[a * 3 + 1] * v1 + Ki1[a * 3 + 2]);
  }
  wts[o] = fs[(long long)b * n0 * n1 + c];
  float* cr = corr + o * 6;
  cr[0] = u0; cr[1] = v0; cr[2] = u1; cr[3] = v1; cr[4] = d0; cr[5] = d1;
}

// Backward of the above w.r.t. the keypoints and depths (training: reference loss_class.py:139-146 under autograd; the
// intrinsics are detached).  X_a = d (Ki[a,0] u + Ki[a,1] v + Ki[a,2]):  dL/du = d sum_a gX_a Ki[a,0], dL/dv = d sum_a gX_a Ki[a,1],
// dL/dd = sum_a gX_a (Ki[a,:] . [u, v, 1]).  A keypoint is drawn by many cells of many rows: fp32 atomic adds into zeroed
// outputs (what torch's index backward does on a GPU too).
__global__ __launch_bounds__(256) void gather_backproject_bwd_kernel(const int* __restrict__ idx, const float* __restrict__ corr,
                                                                     const float* __restrict__ gX, const float* __restrict__ gY,
                                                                     const float* __restrict__ K0, const float* __restrict__ K1,
                                                                     float* __restrict__ gkps0, float* __restrict__ gdep0,
                                                                     float* __restrict__ gkps1, float* __restrict__ gdep1,
                                                                     int rows_per_pair, int k, int n0, int n1) {
  const int r = blockIdx.y, b = r / rows_per_pair;
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= k) return;
  float Ki0[9], Ki1[9];
  inv3(K0 + b * 9, Ki0);
  inv3(K1 + b * 9, Ki1);
  const long long o = (long long)r * k + s;
  const int c = idx[o];
  const int i = c / n1, j = c - i * n1;
  const float* cr = corr + o * 6;
  const float u0 = cr[0], v0 = cr[1], u1 = cr[2], v1 = cr[3], d0 = cr[4], d1 = cr[5];
  float gu0 = 0.f, gv0 = 0.f, gd0 = 0.f, gu1 = 0.f, gv1 = 0.f, gd1 = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float gx = gX[o * 3 + a], gy = gY[o * 3 + a];
    gu0 += gx * Ki0[a * 3 + 0];
    gv0 += gx * Ki0[a * 3 + 1];
    gd0 += gx * (Ki0[a * 3 + 0] * u0 + Ki0[a * 3 + 1] * v0 + Ki0[a * 3 + 2]);
    gu1 += gy * Ki1[a * 3 + 0];
    gv1 += gy * Ki1[a * 3 + 1];
    gd1 += gy * (Ki1[a * 3 + 0] * u1 + Ki1[a * 3 + 1] * v1 + Ki1[a * 3 + 2]);
  }
  atomicAdd(gkps0 + ((long long)b * 2 + 0) * n0 + i, d0 * gu0);
  atomicAdd(gkps0 + ((long long)b * 2 + 1) * n0 + i, d0 * gv0);
  atomicAdd(gdep0 + (long long)b * n0 + i, gd0);
  atomicAdd(gkps1 + ((long long)b * 2 + 0) * n1 + j, d1 * gu1);
  atomicAdd(gkps1 + ((long long)b * 2 + 1) * n1 + j, d1 * gv1);
  atomicAdd(gdep1 + (long long)b * n1 + j, gd1);
}

// ---- 3x3 Kabsch: R = V diag(1,1,det(V U^T)) U^T for H = U S V^T (reference loss/solvers.py:45-50) ----
// One-sided Jacobi on the columns of H (no H^T H: keeps fp32-level relative accuracy of the small
// singular directions), fp64, then the two leading singular pairs + right-handed completion, which
// equals the reflection-fixed Kabsch rotation and is finite for degenerate (collinear) input.
struct KabschFloor { static __device__ constexpr double value() { return 1e-30; } };
__device__ void kabsch_rotation(const double Hin[9], double R[9]) {
  double G[9], V[9], S[3], u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
  int ord[3];
  jacobi_sweeps<12>(Hin, G, V, KabschFloor());
  leading_pair(G, ord, S, u1, u2);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    v1[r] = V[r * 3 + ord[0]];
    v2[r] = V[r * 3 + ord[1]];
  }
  cross3(u1, u2, u3);
  cross3(v1, v2, v3);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) R[a * 3 + b] = v1[a] * u1[b] + v2[a] * u2[b] + v3[a] * u3[b];
}

// ---- hypotheses: block = (set r, slice of its hypotheses); wave = a few hypotheses, their SVDs one per lane ---
__global__ __launch_bounds__(256) void hypotheses_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                         const float* __restrict__ wts, const float* __restrict__ noise3,
                                                         const int* __restrict__ idx3_in, unsigned k0, unsigned k1,
                                                         unsigned off_lo, unsigned off_hi,
                                                         const unsigned long long* __restrict__ offp, float th_soft,
                                                         float* __restrict__ Rh, float* __restrict__ th,
                                                         float* __restrict__ score, int* __restrict__ idx3, int it_ransac, int k,
                                                         int nsplit, long long set_base) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // X[k*3] | Y[k*3] | w[k] | cdf[k] | scan scratch[256]
  add_device_offset(off_lo, off_hi, offp);
  float* sX = lds;
  float* sY = lds + (size_t)k * 3;
  float* sW = lds + (size_t)k * 6;
  float* sC = lds + (size_t)k * 7;   // inclusive prefix sums of the weights (the on-device 3-sample draws through it)
  float* sS = lds + (size_t)k * 8;
  const int r = blockIdx.x / nsplit, part = blockIdx.x % nsplit;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  stage_set(X, Y, wts, r, k, sX, sY, sW);
  __syncthreads();
  const bool cdf_draw = !idx3_in && !noise3;
  if (cdf_draw) {   // block scan: thread t owns the run [t * run, (t + 1) * run)
    const int run = (k + 255) / 256, j0 = threadIdx.x * run;
    float acc = 0.f;
    for (int j = j0; j < min(k, j0 + run); ++j) acc += fmaxf(sW[j], 0.f);
    sS[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {   // Hillis-Steele over the 256 run totals
      const float v = threadIdx.x >= o ? sS[threadIdx.x - o] : 0.f;
      __syncthreads();
      sS[threadIdx.x] += v;
      __syncthreads();
    }
    float c = threadIdx.x ? sS[threadIdx.x - 1] : 0.f;
    for (int j = j0; j < min(k, j0 + run); ++j) {
      c += fmaxf(sW[j], 0.f);
      sC[j] = c;
    }
    __syncthreads();
  }
  const int per = (it_ransac + nsplit - 1) / nsplit;
  const int h0 = part * per, h1 = min(it_ransac, h0 + per);
  const float beta = 5.0f / th_soft;
  // A wave owns the hypotheses h0 + wave, + 4, ...  Three phases per pass of up to HYP_PASS of them:
  //   1. selection (wave-cooperative arg-max over the k matches) and the 3 x 3 cross-covariance, parked in lane i;
  //   2. the fp64 Jacobi SVD of ALL parked hypotheses at once, one per lane (computed redundantly by 64 lanes it was most of
  //      this kernel's time: divisions and square roots in fp64 at a fraction of the fp32 rate, hypothesis after hypothesis);
  //   3. soft-inlier scoring, wave-cooperative again, R and t broadcast from lane i.
  // Every hypothesis sees exactly the arithmetic it saw before: the results are bit-identical.
  constexpr int HYP_PASS = 8;
  for (int hb = h0 + wave; hb < h1; hb += 4 * HYP_PASS) {
    double myH[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    float myam[3] = {0.f, 0.f, 0.f}, mybm[3] = {0.f, 0.f, 0.f};
    int mysel[3] = {0, 0, 0};
    // On-device draws: lane i draws the triple of ITS hypothesis (hb + 4 i) by sequential sampling without replacement
    // through the prefix sums -- the same (Plackett-Luce) distribution as the top-3 of the exponential race, order included,
    // from 3 uniforms instead of k Exp(1) draws (the race over 2048 matches was two thirds of this kernel: 8 Philox calls,
    // 32 logarithms and 32 divisions per lane and hypothesis).  Injected noise / indices keep the race (torch-comparable).
    int draw3[3] = {0, 0, 0};
    if (cdf_draw && lane < HYP_PASS && hb + 4 * lane < h1) {
      const long long gh = (long long)r * it_ransac + hb + 4 * lane + set_base * it_ransac;   // GLOBAL hypothesis index
      const U4 rnd = philox4x32(k0, k1, U4{0x3c6ef372u, (unsigned)gh, (unsigned)(gh >> 32) ^ off_hi ^ 0x5bd1e995u, off_lo});
      const unsigned rr[3] = {rnd.x, rnd.y, rnd.z};
      int ex[2] = {-1, -1};        // chosen so far, ascending
      float exw[2] = {0.f, 0.f};   // their weights
      float rem = sC[k - 1];
      for (int d = 0; d < 3; ++d) {
        const float u = ((float)(rr[d] >> 8) + 0.5f) * 5.9604644775390625e-8f;   // (0, 1) on a 2^-24 grid
        const float target = u * rem;
        // smallest j with F'(j) > target, F'(j) = cdf[j] - (weights of the chosen indices <= j)
        int lo = 0, hi = k - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          float f = sC[mid];
          if (ex[0] >= 0 && ex[0] <= mid) f -= exw[0];
          if (ex[1] >= 0 && ex[1] <= mid) f -= exw[1];
          if (f > target) hi = mid; else lo = mid + 1;
        }
        // round-off next to a chosen index / zero-weight runs: step to the next index that can be drawn; if nothing is
        // left (fewer than three positive weights) the lowest index not yet chosen, as the race's tie rule does
        int j = lo;
        for (int tries = 0; tries < k && (j == ex[0] || j == ex[1] || !(sW[j] > 0.f)); ++tries) j = j + 1 < k ? j + 1 : 0;
        if (j == ex[0] || j == ex[1] || !(sW[j] > 0.f)) {
          j = 0;
          while (j == ex[0] || j == ex[1]) ++j;
        }
        draw3[d] = j;
        const float wj = fmaxf(sW[j], 0.f);
        rem = fmaxf(rem - wj, 0.f);
        if (ex[0] < 0) { ex[0] = j; exw[0] = wj; }
        else if (j < ex[0]) { ex[1] = ex[0]; exw[1] = exw[0]; ex[0] = j; exw[0] = wj; }
        else { ex[1] = j; exw[1] = wj; }
      }
    }
    for (int i = 0; i < HYP_PASS; ++i) {
      const int h = hb + 4 * i;
      if (h >= h1) break;
      const long long hyp = (long long)r * it_ransac + h;
      int sel[3];
      if (cdf_draw) {
        sel[0] = __shfl(draw3[0], i, 64);
        sel[1] = __shfl(draw3[1], i, 64);
        sel[2] = __shfl(draw3[2], i, 64);
      } else if (idx3_in) {
        sel[0] = idx3_in[hyp * 3 + 0];
        sel[1] = idx3_in[hyp * 3 + 1];
        sel[2] = idx3_in[hyp * 3 + 2];
      } else {
        // per-lane top-3 of key = w / e, then 3 wave arg-max rounds
        float bk[3] = {-1.f, -1.f, -1.f};
        int bi[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
        for (int base = lane * 4; base < k; base += 256) {
          float e[4];
          if (noise3) {
  #pragma unroll
            for (int q = 0; q < 4; ++q) e[q] = base + q < k ? noise3[hyp * k + base + q] : 1.f;
          } else {
            const long long gh = hyp + set_base * it_ransac;   // GLOBAL hypothesis index: draws do not depend on how a batch is split
            const U4 rnd = philox4x32(k0, k1, U4{(unsigned)(base >> 2), (unsigned)gh, (unsigned)(gh >> 32) ^ off_hi ^ 0x5bd1e995u, off_lo});
            e[0] = exp1(rnd.x); e[1] = exp1(rnd.y); e[2] = exp1(rnd.z); e[3] = exp1(rnd.w);
          }
  #pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int j = base + q;
            if (j >= k) continue;
            const float key = sW[j] / e[q];
            if (key > bk[2]) {  // strict: earlier (lower) index wins ties
              if (key > bk[0]) { bk[2] = bk[1]; bi[2] = bi[1]; bk[1] = bk[0]; bi[1] = bi[0]; bk[0] = key; bi[0] = j; }
              else if (key > bk[1]) { bk[2] = bk[1]; bi[2] = bi[1]; bk[1] = key; bi[1] = j; }
              else { bk[2] = key; bi[2] = j; }
            }
          }
        }
  #pragma unroll
        for (int round = 0; round < 3; ++round) {
          float v = bk[0];
          int ix = bi[0];
          wave_argmax(v, ix);
          sel[round] = ix;
          if (bi[0] == ix) { bk[0] = bk[1]; bi[0] = bi[1]; bk[1] = bk[2]; bi[1] = bi[2]; bk[2] = -1.f; bi[2] = 0x7fffffff; }
        }
      }
      // means and cross-covariance of the 3 pairs (reference loss/solvers.py:31-39,45-52)
      float am[3], bm[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        am[a] = (sX[sel[0] * 3 + a] + sX[sel[1] * 3 + a] + sX[sel[2] * 3 + a]) / 3.0f;
        bm[a] = (sY[sel[0] * 3 + a] + sY[sel[1] * 3 + a] + sY[sel[2] * 3 + a]) / 3.0f;
      }
      const bool mine = lane == i;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float sm = 0.f;
#pragma unroll
          for (int pnt = 0; pnt < 3; ++pnt) sm += (sX[sel[pnt] * 3 + a] - am[a]) * (sY[sel[pnt] * 3 + c] - bm[c]);
          if (mine) myH[a * 3 + c] = (double)sm;
        }
        if (mine) {
          myam[a] = am[a];
          mybm[a] = bm[a];
          mysel[a] = sel[a];
        }
      }
    }
    double Rd[9];
    kabsch_rotation(myH, Rd);
    float myR[9], myt[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) myR[q] = (float)Rd[q];
    fit_translation(myR, myam, mybm, myt);
    for (int i = 0; i < HYP_PASS; ++i) {
      const int h = hb + 4 * i;
      if (h >= h1) break;
      const long long hyp = (long long)r * it_ransac + h;
      float Rf[9], tf[3];
      int sel[3];
#pragma unroll
      for (int q = 0; q < 9; ++q) Rf[q] = __shfl(myR[q], i, 64);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        tf[a] = __shfl(myt[a], i, 64);
        sel[a] = __shfl(mysel[a], i, 64);
      }
      float sc = 0.f;
      for (int jj = lane; jj < k; jj += 64) sc += soft_inlier(beta, th_soft, pt_dist(Rf, tf, sX + jj * 3, sY + jj * 3), ExpLibm());
      sc = wave_sum(sc);
      if (lane < 9) Rh[hyp * 9 + lane] = Rf[lane];
      if (lane < 3) { th[hyp * 3 + lane] = tf[lane]; idx3[hyp * 3 + lane] = sel[lane]; }
      if (lane == 0) score[hyp] = sc;
    }
  }
}

// ---- arg-max + refinement: one workgroup per pair -----------------------------------------------------
constexpr int RT = 512;
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0;
  for (int i = 0; i < RT / 64; ++i) s += red[i];
  return s;
}

__global__ __launch_bounds__(RT) void refine_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                    const float* __restrict__ Rh, const float* __restrict__ th,
                                                    const float* __restrict__ score, float th_in, int num_ref, int min_inl,
                                                    float* __restrict__ Ro, float* __restrict__ to, float* __restrict__ conf,
                                                    int* __restrict__ best, unsigned char* __restrict__ mask,
                                                    int* __restrict__ rounds, int* __restrict__ invalid, int it_matches,
                                                    int it_ransac, int k) {
  __shared__ double red[RT / 64];
  __shared__ float sv[RT / 64];
  __shared__ int si[RT / 64];
  __shared__ float sR[9], st[3];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HP = it_matches * it_ransac;
  // non-finite hypothesis anywhere in the batch -> the reference returns the zero pose for all pairs
  bool bad = false;
  for (int i = tid; i < HP * 9; i += RT) bad |= !isfinite(Rh[(long long)b * HP * 9 + i]);
  for (int i = tid; i < HP * 3; i += RT) bad |= !isfinite(th[(long long)b * HP * 3 + i]);
  if (bad) atomicOr(invalid, 1);
  // arg-max (first index among equal maxima)
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < HP; i += RT) {
    const float v = score[(long long)b * HP + i];
    if (v > bv) { bv = v; bi = i; }
  }
  wave_argmax(bv, bi);
  if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < RT / 64; ++i)
      if (sv[i] > bv || (sv[i] == bv && si[i] < bi)) { bv = sv[i]; bi = si[i]; }
    if (bi == 0x7fffffff) bi = 0;  // all-NaN scores
    si[0] = bi;
    for (int i = 0; i < 9; ++i) sR[i] = Rh[((long long)b * HP + bi) * 9 + i];
    for (int i = 0; i < 3; ++i) st[i] = th[((long long)b * HP + bi) * 3 + i];
  }
  __syncthreads();
  const int hb = si[0];
  const long long set = (long long)b * it_matches + hb / it_ransac;
  const float* Xb = X + set * k * 3;
  const float* Yb = Y + set * k * 3;
  float best_cnt = (float)min_inl;
  int nround = 0;
  float R[9], t[3];
  auto load_pose = [&] {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = sR[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = st[i];
  };
  for (int it = 0; it < num_ref; ++it) {
    load_pose();
    // masked Procrustes over the inliers of (R, t): centroids with w / (sum|w| + 1e-16), covariance with the RAW 0/1 mask
    // (solvers.py:14-26); the fit ends (block-uniformly) unless the inlier count grew
    double C, am[3], bm[3], H[9];
    const bool more = procrustes_moments<float>(
        Xb, Yb,
        [&](auto&& f) {
          for (int j = tid; j < k; j += RT)
            if (th_in - pt_dist(R, t, Xb + j * 3, Yb + j * 3) >= 0.f) f(j, 1.0);
        },
        [&](double v) { return block_sum_d(v, red); }, [&](double c) { return c >= (double)min_inl && c > (double)best_cnt; }, C, am,
        bm, H);
    if (!more) break;
    best_cnt = (float)C;
    ++nround;
    __syncthreads();
    if (tid == 0) {
      double Rd[9];
      kabsch_rotation(H, Rd);
      for (int i = 0; i < 9; ++i) sR[i] = (float)Rd[i];
      fit_translation(sR, am, bm, st);
    }
    __syncthreads();
  }
  __syncthreads();
  load_pose();
  const float beta = 5.0f / th_in;
  double cs = 0;
  for (int j = tid; j < k; j += RT) {
    const float d = pt_dist(R, t, Xb + j * 3, Yb + j * 3);
    cs += (double)soft_inlier(beta, th_in, d, ExpLibm());
    mask[(long long)b * k + j] = (th_in - d) >= 0.f ? 1 : 0;
  }
  const double ctot = block_sum_d(cs, red);
  if (tid < 9) Ro[b * 9 + tid] = R[tid];
  if (tid < 3) to[b * 3 + tid] = t[tid];
  if (tid == 0) { conf[b] = (float)ctot; best[b] = hb; rounds[b] = nround; }
}

// ---- training-time RANSAC (reference loss/loss_class.py:141-184) -------------------------------
// One workgroup per sampled match set (row r: S matches X, Y, w staged in LDS once), one wave per hypothesis.  A hypothesis
// draws NUM_CORR matches without replacement ~ w (exponential race: top-NUM_CORR of w / Exp(1), Philox in registers or
// injected noise / indices), then runs the reference's refinement state machine:
//     cur = sample, fin = sample, pre = NUM_CORR
//     repeat NUM_REF_STEPS: (R, t) = masked Procrustes(cur); ref = {|R x + t - y| <= th}; stop unless |ref| > pre;
//                           pre = |ref|, fin = cur, cur = ref
// and emits fin as a 0/1 float mask [S] -- the input of the differentiable Procrustes the loss is built on.  Match j of a
// row lives in lane j % 64, slot j / 64 (S <= 1024): the three sets are 16-bit masks per lane, no memory traffic.
constexpr int TR_SLOTS = 16;

__global__ __launch_bounds__(256) void train_refine_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                           const float* __restrict__ wts, const float* __restrict__ noise,
                                                           const int* __restrict__ idx_in, unsigned k0, unsigned k1,
                                                           unsigned off_lo, unsigned off_hi,
                                                           const unsigned long long* __restrict__ offp, float th_ref,
                                                           int num_ref, int nc, float* __restrict__ fin_mask,
                                                           int* __restrict__ idx_out, int* __restrict__ rounds_out,
                                                           int it_ransac, int S, long long set_base) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // X[S*3] | Y[S*3] | w[S]
  add_device_offset(off_lo, off_hi, offp);
  float* sX = lds;
  float* sY = lds + (size_t)S * 3;
  float* sW = lds + (size_t)S * 6;
  const int r = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  stage_set(X, Y, wts, r, S, sX, sY, sW);
  __syncthreads();
  const int nq = (S + 63) >> 6;
  for (int h = wave; h < it_ransac; h += 4) {
    const long long hyp = (long long)r * it_ransac + h;
    unsigned cur = 0;
    if (idx_in) {
      for (int c = 0; c < nc; ++c) {
        const int j = idx_in[hyp * nc + c];
        if ((j & 63) == lane) cur |= 1u << (j >> 6);
        if (lane == 0) idx_out[hyp * nc + c] = j;
      }
    } else {
      float key[TR_SLOTS];
#pragma unroll
      for (int q4 = 0; q4 < TR_SLOTS / 4; ++q4) {
        float e[4] = {1.f, 1.f, 1.f, 1.f};
        if (q4 * 4 < nq) {
          if (noise) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int j = (q4 * 4 + u) * 64 + lane;
              if (j < S) e[u] = noise[hyp * S + j];
            }
          } else {
            const long long gh = hyp + set_base * it_ransac;   // GLOBAL hypothesis index (sharding-invariant draws)
            const U4 rnd = philox4x32(k0, k1, U4{(unsigned)(q4 * 64 + lane), (unsigned)gh, (unsigned)(gh >> 32) ^ off_hi ^ 0x2545f491u, off_lo});
            e[0] = exp1(rnd.x); e[1] = exp1(rnd.y); e[2] = exp1(rnd.z); e[3] = exp1(rnd.w);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = (q4 * 4 + u) * 64 + lane;
          key[q4 * 4 + u] = j < S ? sW[j] / e[u] : -1.f;
        }
      }
      for (int c = 0; c < nc; ++c) {
        float v = -1.f;
        int ix = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < TR_SLOTS; ++q)
          if (!((cur >> q) & 1u) && key[q] > v) { v = key[q]; ix = q * 64 + lane; }   // ascending j within a lane: first wins ties
        wave_argmax(v, ix);
        if (ix != 0x7fffffff && (ix & 63) == lane) cur |= 1u << (ix >> 6);
        if (lane == 0) idx_out[hyp * nc + c] = ix == 0x7fffffff ? 0 : ix;
      }
    }
    unsigned fin = cur;
    int pre = nc, nround = 0;
    for (int it = 0; it < num_ref; ++it) {
      // masked Procrustes over cur: centroids with w / (sum|w| + 1e-16), covariance with the RAW 0/1 mask (solvers.py:14-26)
      double C, am[3], bm[3], H[9], Rd[9];
      procrustes_moments<float>(
          sX, sY,
          [&](auto&& f) {
#pragma unroll
            for (int q = 0; q < TR_SLOTS; ++q)
              if ((cur >> q) & 1u) f(q * 64 + lane, 1.0);
          },
          [](double v) { return wave_sum_d(v); }, [](double) { return true; }, C, am, bm, H);
      kabsch_rotation(H, Rd);
      float Rf[9], tf[3];
#pragma unroll
      for (int i = 0; i < 9; ++i) Rf[i] = (float)Rd[i];
      fit_translation(Rf, am, bm, tf);
      unsigned ref = 0;
      int rl = 0;
#pragma unroll
      for (int q = 0; q < TR_SLOTS; ++q) {
        const int j = q * 64 + lane;
        if (j < S && th_ref - pt_dist(Rf, tf, sX + j * 3, sY + j * 3) >= 0.f) { ref |= 1u << q; ++rl; }
      }
      const int cnt = (int)wave_sum((float)rl);
      if (!(cnt > pre)) break;   // wave-uniform
      pre = cnt;
      fin = cur;
      cur = ref;
      ++nround;
    }
#pragma unroll
    for (int q = 0; q < TR_SLOTS; ++q) {
      const int j = q * 64 + lane;
      if (j < S) fin_mask[hyp * S + j] = (fin >> q) & 1u ? 1.f : 0.f;
    }
    if (lane == 0) rounds_out[hyp] = nround;
  }
}

// REINFORCE bookkeeping (loss_class.py:251-261): gradients[b, c] += loss_value[row], gradients_b[b, c] += 1 for the S
// sampled cells c of every row of pair b, ROW AFTER ROW like the reference's python loop (a cell drawn by several rows
// receives its fp32 additions in the same order: bit-identical sums).  Cells within a row are distinct (sampling without
// replacement), so a row is a plain read-modify-write; one workgroup per pair, a barrier between rows.
__global__ __launch_bounds__(512) void reinforce_scatter_kernel(const int* __restrict__ idx, const float* __restrict__ loss_value,
                                                                float* __restrict__ grads, float* __restrict__ grads_b,
                                                                int it_matches, int S, long long ncell) {
  const int b = blockIdx.x;
  float* g = grads + (long long)b * ncell;
  float* gb = grads_b + (long long)b * ncell;
  for (int r = 0; r < it_matches; ++r) {
    const long long row = (long long)b * it_matches + r;
    const float lv = loss_value[row];
    for (int s = threadIdx.x; s < S; s += 512) {
      const int c = idx[row * S + s];
      g[c] += lv;
      gb[c] += 1.0f;
    }
    __syncthreads();
  }
}

__global__ void finalize_kernel(float* R, float* t, float* conf, const int* invalid, int B) {
  if (*invalid == 0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * 9) R[i] = 0.f;
  if (i < B * 3) t[i] = 0.f;
  if (i < B) conf[i] = 0.f;
}

}  // namespace

extern "C" {

int mk_gather_backproject(const int* idx, const float* final_scores, const float* kps0, const float* depth0, const float* kps1,
                          const float* depth1, const float* K0, const float* K1, float* X, float* Y, float* wts, float* corr,
                          int B, int rows_per_pair, int k, int n0, int n1, mk_stream_t stream) {
  return mk_gather_backproject_kf(idx, final_scores, kps0, depth0, kps1, depth1, K0, K1, X, Y, wts, corr, B, rows_per_pair, k, n0, n1,
                                  nullptr, B, stream);
}

int mk_gather_backproject_kf(const int* idx, const float* final_scores, const float* kps0, const float* depth0, const float* kps1,
                             const float* depth1, const float* K0, const float* K1, float* X, float* Y, float* wts, float* corr,
                             int B, int rows_per_pair, int k, int n0, int n1, const int* kf_index, int K, mk_stream_t stream) {
  MK_CHECK_ARG(idx && final_scores && kps0 && depth0 && kps1 && depth1 && K0 && K1 && X && Y && wts && corr,
               "mk_gather_backproject: null pointer");
  MK_CHECK_ARG(B > 0 && rows_per_pair > 0 && k > 0 && n0 > 0 && n1 > 0, "mk_gather_backproject: bad sizes");
  MK_CHECK_ARG(kf_index ? (K > 0 && K <= B) : K == B, "mk_gather_backproject_kf: need 0 < K <= B with a keyframe map, K == B without");
  return mk_gather_backproject_pairs(idx, final_scores, kps0, depth0, kps1, depth1, K0, K1, X, Y, wts, corr, B, rows_per_pair, k, n0, n1,
                                     kf_index, nullptr, K, B, stream);
}

int mk_gather_backproject_pairs(const int* idx, const float* final_scores, const float* kps0, const float* depth0, const float* kps1,
                                const float* depth1, const float* K0, const float* K1, float* X, float* Y, float* wts, float* corr,
                                int B, int rows_per_pair, int k, int n0, int n1, const int* idx0, const int* idx1, int N0, int N1,
                                mk_stream_t stream) {
  MK_CHECK_ARG(idx && final_scores && kps0 && depth0 && kps1 && depth1 && K0 && K1 && X && Y && wts && corr,
               "mk_gather_backproject_pairs: null pointer");
  MK_CHECK_ARG(B > 0 && rows_per_pair > 0 && k > 0 && n0 > 0 && n1 > 0, "mk_gather_backproject_pairs: bad sizes");
  const RowMaps rm{idx0, N0, idx1, N1};
  if (const int rc = check_row_maps("mk_gather_backproject_pairs", rm, B)) return rc;
  const dim3 g((k + 255) / 256, B * rows_per_pair);
  hipStream_t st = (hipStream_t)stream;
  with_row_map(rm, [&](auto M) {
    hipLaunchKernelGGL(gather_backproject_kernel<decltype(M)::value>, g, dim3(256), 0, st, idx, final_scores, kps0, depth0, kps1, depth1,
                       K0, K1, X, Y, wts, corr, rows_per_pair, k, n0, n1, idx0, N0, idx1, N1);
  });
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_gather_backproject_bwd(const int* idx, const float* corr, const float* gX, const float* gY, const float* K0, const float* K1,
                              float* gkps0, float* gdepth0, float* gkps1, float* gdepth1, int B, int rows_per_pair, int k, int n0,
                              int n1, mk_stream_t stream) {
  MK_CHECK_ARG(idx && corr && gX && gY && K0 && K1 && gkps0 && gdepth0 && gkps1 && gdepth1, "mk_gather_backproject_bwd: null pointer");
  MK_CHECK_ARG(B > 0 && rows_per_pair > 0 && k > 0 && n0 > 0 && n1 > 0, "mk_gather_backproject_bwd: bad sizes");
  hipLaunchKernelGGL(gather_backproject_bwd_kernel, dim3((k + 255) / 256, B * rows_per_pair), dim3(256), 0, (hipStream_t)stream, idx,
                     corr, gX, gY, K0, K1, gkps0, gdepth0, gkps1, gdepth1, rows_per_pair, k, n0, n1);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_ransac_hypotheses(const float* X, const float* Y, const float* wts, const float* noise3, const int* idx3_in,
                         unsigned long long seed, unsigned long long offset, const unsigned long long* offset_dev, float th_soft,
                         float* Rh, float* th, float* score, int* idx3, int nsets, int it_ransac, int k, long long set_base,
                         mk_stream_t stream) {
  MK_CHECK_ARG(X && Y && wts && Rh && th && score && idx3, "mk_ransac_hypotheses: null pointer");
  MK_CHECK_ARG(nsets > 0 && it_ransac > 0 && k >= 3 && (size_t)k * 32 + 1024 <= 150 * 1024, "mk_ransac_hypotheses: bad sizes (k <= 4768)");
  // blocks per correspondence set: 4 (25 hypotheses per block, 6 - 7 per wave) when the sets alone fill the part; with few sets
  // (one pair: 20) as many as keep every wave at >= one hypothesis and the launch at ~2 blocks per CU -- a hypothesis' arithmetic and
  // draws do not depend on the block it is computed in (keyed by its global index): bit-identical for any split
  int nsplit = it_ransac >= 16 ? 4 : 1;
  if (it_ransac >= 16) nsplit = max(4, min((it_ransac + 3) / 4, (2 * mk::gemm::num_cus() + nsets - 1) / nsets));
  const size_t lds = ((size_t)k * 8 + 256) * sizeof(float);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)hypotheses_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { mk_set_error("mk_ransac_hypotheses: cannot reserve %zu B of LDS", lds); return MK_ERR_LAUNCH; }
  }
  hipLaunchKernelGGL(hypotheses_kernel, dim3(nsets * nsplit), dim3(256), lds, (hipStream_t)stream, X, Y, wts, noise3, idx3_in,
                     (unsigned)seed, (unsigned)(seed >> 32), (unsigned)offset, (unsigned)(offset >> 32), offset_dev, th_soft, Rh, th,
                     score, idx3, it_ransac, k, nsplit, set_base);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_refine_pose(const float* X, const float* Y, const float* Rh, const float* th, const float* score, float th_inlier,
                   int num_ref, int min_inliers, float* R, float* t, float* conf, int* best, unsigned char* inl_mask, int* rounds,
                   int* invalid, int B, int it_matches, int it_ransac, int k, mk_stream_t stream) {
  MK_CHECK_ARG(X && Y && Rh && th && score && R && t && conf && best && inl_mask && rounds && invalid,
               "mk_refine_pose: null pointer");
  MK_CHECK_ARG(B > 0 && it_matches > 0 && it_ransac > 0 && k > 0 && num_ref >= 0, "mk_refine_pose: bad sizes");
  hipLaunchKernelGGL(refine_kernel, dim3(B), dim3(RT), 0, (hipStream_t)stream, X, Y, Rh, th, score, th_inlier, num_ref,
                     min_inliers, R, t, conf, best, inl_mask, rounds, invalid, it_matches, it_ransac, k);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_pose_finalize(float* R, float* t, float* conf, const int* invalid, int B, mk_stream_t stream) {
  MK_CHECK_ARG(R && t && conf && invalid && B > 0, "mk_pose_finalize: bad args");
  hipLaunchKernelGGL(finalize_kernel, dim3((B * 9 + 255) / 256), dim3(256), 0, (hipStream_t)stream, R, t, conf, invalid, B);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_train_ransac_masks(const float* X, const float* Y, const float* wts, const float* noise, const int* idx_in,
                          unsigned long long seed, unsigned long long offset, const unsigned long long* offset_dev, float th_ref,
                          int num_ref, int num_corr, float* final_mask, int* idx_out, int* rounds, int nsets, int it_ransac,
                          int S, long long set_base, mk_stream_t stream) {
  MK_CHECK_ARG(X && Y && wts && final_mask && idx_out && rounds, "mk_train_ransac_masks: null pointer");
  MK_CHECK_ARG(nsets > 0 && it_ransac > 0 && S > 0 && S <= 64 * TR_SLOTS && num_corr >= 3 && num_corr <= S && num_ref >= 0,
               "mk_train_ransac_masks: bad sizes (3 <= num_corr <= S <= %d)", 64 * TR_SLOTS);
  const size_t lds = (size_t)S * 7 * sizeof(float);
  hipLaunchKernelGGL(train_refine_kernel, dim3(nsets), dim3(256), lds, (hipStream_t)stream, X, Y, wts, noise, idx_in,
                     (unsigned)seed, (unsigned)(seed >> 32), (unsigned)offset, (unsigned)(offset >> 32), offset_dev, th_ref,
                     num_ref, num_corr, final_mask, idx_out, rounds, it_ransac, S, set_base);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_reinforce_scatter(const int* idx, const float* loss_value, float* gradients, float* gradients_b, int B, int it_matches,
                         int S, long long ncell, mk_stream_t stream) {
  MK_CHECK_ARG(idx && loss_value && gradients && gradients_b, "mk_reinforce_scatter: null pointer");
  MK_CHECK_ARG(B > 0 && it_matches > 0 && S > 0 && ncell > 0 && ncell < (1LL << 31), "mk_reinforce_scatter: bad sizes");
  hipLaunchKernelGGL(reinforce_scatter_kernel, dim3(B), dim3(512), 0, (hipStream_t)stream, idx, loss_value, gradients,
                     gradients_b, it_matches, S, ncell);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

}  // extern "C"
