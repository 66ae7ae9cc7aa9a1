// mickey_amd -- the rigid-fit (Procrustes / Kabsch) arithmetic of the pose solver, stated once for the inference kernels
// (mk_solver.hip: hypotheses, refinement, training-time RANSAC masks) and for the differentiable tail (mk_train_tail.hip).
//
// FLOATING-POINT CONTRACTION: this header carries NO `#pragma clang fp contract` of its own, on purpose.  mk_solver.hip
// compiles everything after its `#pragma clang fp contract(off)` un-fused (comparable with ATen) and includes this header
// AFTER that pragma; mk_train_tail.hip has no such pragma and fuses a * b + c into an fma.  Every function below therefore
// compiles in the mode of the file that includes it, as the hand-kept copies it replaces did.  A pragma here, or an include
// moved in front of the solver's pragma, changes result bits.
//
// What the two users deliberately keep different is a parameter here, not a copy: the Jacobi sweep count and skip floor
// (jacobi_sweeps), the precision of the 1 / sum|w| normalisation (procrustes_moments) and the finishing stage on top of the
// sweeps (kabsch_rotation / svd3 stay in their files).  The tail's t = bbar - R abar, its residuals and its __expf soft-inlier
// term stay spelled out in mk_train_tail.hip: under contraction the form of these fp32 expressions decides which product is
// fused, and routing them through fit_translation / residual / soft_inlier changed result bits.
#pragma once
#include "mk_common.hpp"

namespace mk {

// ---- small fp64 3x3 helpers (row-major) ------------------------------------------------------------------------------
__device__ __forceinline__ double det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// C = op(A) op(B) in fp64, op = transpose where TA / TB; every element is the sum over k = 0, 1, 2 in that order, then cast to T
template <bool TA, bool TB, typename T>
__device__ __forceinline__ void mul3(const double* A, const double* B, T* C) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      C[a * 3 + c] = (T)((TA ? A[a] : A[a * 3]) * (TB ? B[c * 3] : B[c]) + (TA ? A[3 + a] : A[a * 3 + 1]) * (TB ? B[c * 3 + 1] : B[3 + c]) +
                         (TA ? A[6 + a] : A[a * 3 + 2]) * (TB ? B[c * 3 + 2] : B[6 + c]));
}

// ---- one-sided Jacobi on the columns of G (no H^T H: keeps fp32-level relative accuracy of the small singular directions) ---
// On exit G = H V has orthogonal columns (= U S, unordered) and V holds the accumulated rotations.  At most SWEEPS sweeps; a
// pair of columns whose inner product is at most Floor::value() (or negligible beside their norms) is left alone.
template <int SWEEPS, typename Floor>
__device__ __forceinline__ void jacobi_sweeps(const double H[9], double G[9], double V[9], Floor) {
#pragma unroll
  for (int i = 0; i < 9; ++i) { G[i] = H[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double al = 0, be = 0, ga = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        al += G[r * 3 + p] * G[r * 3 + p];
        be += G[r * 3 + q] * G[r * 3 + q];
        ga += G[r * 3 + p] * G[r * 3 + q];
      }
      if (fabs(ga) <= Floor::value() || ga * ga <= 1e-32 * al * be) continue;
      off += fabs(ga);
      const double zeta = (be - al) / (2.0 * ga);
      const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double gp = G[r * 3 + p], gq = G[r * 3 + q];
        G[r * 3 + p] = cs * gp - sn * gq;
        G[r * 3 + q] = sn * gp + cs * gq;
        const double vp = V[r * 3 + p], vq = V[r * 3 + q];
        V[r * 3 + p] = cs * vp - sn * vq;
        V[r * 3 + q] = sn * vp + cs * vq;
      }
    }
    if (off == 0.0) break;
  }
}

// Columns of G = U S ordered by norm (ord: largest first; S: their norms) and the two leading left singular vectors: u1 is
// the normalised largest column (e_x if it vanishes), u2 the second column Gram-Schmidt'ed against u1 and normalised; if that
// vanishes (rank one) any unit vector perpendicular to u1.  Finite for every input.
__device__ __forceinline__ void leading_pair(const double G[9], int ord[3], double S[3], double u1[3], double u2[3]) {
  double nrm[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) nrm[c] = G[c] * G[c] + G[3 + c] * G[3 + c] + G[6 + c] * G[6 + c];
  int o0 = 0, o1 = 1, o2 = 2;
  if (nrm[o0] < nrm[o1]) { const int t = o0; o0 = o1; o1 = t; }
  if (nrm[o0] < nrm[o2]) { const int t = o0; o0 = o2; o2 = t; }
  if (nrm[o1] < nrm[o2]) { const int t = o1; o1 = o2; o2 = t; }
  ord[0] = o0; ord[1] = o1; ord[2] = o2;
#pragma unroll
  for (int c = 0; c < 3; ++c) S[c] = sqrt(nrm[ord[c]]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    u1[r] = S[0] > 1e-300 ? G[r * 3 + o0] / S[0] : (r == 0 ? 1.0 : 0.0);
    u2[r] = G[r * 3 + o1];
  }
  double d12 = dot3(u1, u2);
#pragma unroll
  for (int r = 0; r < 3; ++r) u2[r] -= d12 * u1[r];
  double n2 = sqrt(dot3(u2, u2));
  if (!(n2 > 1e-12 * S[0]) || !(n2 > 1e-300)) {
    const int ax = fabs(u1[0]) <= fabs(u1[1]) && fabs(u1[0]) <= fabs(u1[2]) ? 0 : (fabs(u1[1]) <= fabs(u1[2]) ? 1 : 2);
    double e[3] = {0, 0, 0};
    e[ax] = 1.0;
    d12 = u1[ax];
#pragma unroll
    for (int r = 0; r < 3; ++r) u2[r] = e[r] - d12 * u1[r];
    n2 = sqrt(dot3(u2, u2));
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) u2[r] /= n2;
}

// ---- residual and soft inlier (reference training_utils.py:55-61) -------------------------------------------------------
// e = R x + t - y; returns d = sqrt(|e|^2 + 1e-6)
__device__ __forceinline__ float residual(const float* R, const float* t, const float* x, const float* y, float e[3]) {
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    e[a] = (R[a * 3 + 0] * x[0] + R[a * 3 + 1] * x[1] + R[a * 3 + 2] * x[2]) + t[a] - y[a];
    s += e[a] * e[a];
  }
  return sqrtf(s + 1e-6f);
}
__device__ __forceinline__ float pt_dist(const float* R, const float* t, const float* x, const float* y) {
  float e[3];
  return residual(R, t, x, y, e);
}
struct ExpLibm { __device__ __forceinline__ float operator()(float x) const { return expf(x); } };
// sigmoid(beta (th - d)); the exponential is a parameter (libm expf in the solver kernels)
template <typename Exp>
__device__ __forceinline__ float soft_inlier(float beta, float th, float d, Exp ex) { return 1.0f / (1.0f + ex(-beta * (th - d))); }

// t = bbar - R abar in fp32 (centroids in fp32 or fp64)
template <typename T>
__device__ __forceinline__ void fit_translation(const float* R, const T* am, const T* bm, float* t) {
#pragma unroll
  for (int a = 0; a < 3; ++a) t[a] = (float)bm[a] - ((float)am[0] * R[a * 3 + 0] + (float)am[1] * R[a * 3 + 1] + (float)am[2] * R[a * 3 + 2]);
}

// ---- weighted Procrustes moments (reference loss/solvers.py:14-26) ------------------------------------------------------
// each(f) calls f(j, w) for every match j that THIS lane owns with weight w != 0 (a double; the 0/1 masks pass the constant
// 1.0, which folds away); sum(v) adds a double over all lanes that share the fit (wave_sum_d, or block_sum_d for a fit that a
// whole workgroup shares).  sw = sum |w|; accept(sw) may end the fit there (false is returned, nothing else is computed);
// centroids am, bm = sum w x / (sw + 1e-16) with the reciprocal in Norm's precision (fp32 in the solver kernels, as the
// reference's float pipeline; fp64 in the training tail); H = sum w (x - am)(y - bm)^T with the RAW weights.  Every lane gets
// the results.
__device__ __forceinline__ double inv_sum_w(double sw, float) { return (double)(1.0f / ((float)sw + 1e-16f)); }
__device__ __forceinline__ double inv_sum_w(double sw, double) { return 1.0 / (sw + 1e-16); }

template <typename Norm, typename Each, typename Sum, typename Accept>
__device__ __forceinline__ bool procrustes_moments(const float* X, const float* Y, Each each, Sum sum, Accept accept, double& sw,
                                                   double am[3], double bm[3], double H[9]) {
  double c = 0.0, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
  each([&](int j, double w) {
    c += fabs(w);
#pragma unroll
    for (int a = 0; a < 3; ++a) { sa[a] += w * X[j * 3 + a]; sb[a] += w * Y[j * 3 + a]; }
  });
  sw = sum(c);
  if (!accept(sw)) return false;
  const double inv = inv_sum_w(sw, Norm());
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    am[a] = sum(sa[a]) * inv;
    bm[a] = sum(sb[a]) * inv;
  }
  double hl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  each([&](int j, double w) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c2 = 0; c2 < 3; ++c2) hl[a * 3 + c2] += w * ((double)X[j * 3 + a] - am[a]) * ((double)Y[j * 3 + c2] - bm[c2]);
  });
#pragma unroll
  for (int i = 0; i < 9; ++i) H[i] = sum(hl[i]);
  return true;
}

// ---- wave arg-max of a (value, index) pair: the lowest index wins ties; every lane gets the winner -------------------------
__device__ __forceinline__ void wave_argmax(float& v, int& ix) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(ix, o, 64);
    if (v2 > v || (v2 == v && i2 < ix)) { v = v2; ix = i2; }
  }
}

// ---- a match set's X | Y (| w) into LDS, by all 256 threads of the workgroup (the caller synchronises) ---------------------
__device__ __forceinline__ void stage_set(const float* X, const float* Y, long long set, int n, float* sX,
                                          float* sY) {
  const float *Xs = X + set * n * 3, *Ys = Y + set * n * 3;
  for (int i = threadIdx.x; i < n * 3; i += 256) {
    sX[i] = Xs[i];
    sY[i] = Ys[i];
  }
}
__device__ __forceinline__ void stage_set(const float* X, const float* Y, const float* w,
                                          long long set, int n, float* sX, float* sY, float* sW) {
  stage_set(X, Y, set, n, sX, sY);
  for (int i = threadIdx.x; i < n; i += 256) sW[i] = w[set * n + i];
}

}  // namespace mk
