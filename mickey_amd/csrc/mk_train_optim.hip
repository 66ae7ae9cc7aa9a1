// mickey_amd -- the tail of a training step (reference lib/models/MicKey/model.py:104-145): the finite checks of the gradients, the
// global L2 norm and its clip (torch.nn.utils.clip_grad_norm_), the skip of a step that met a NaN or an Inf, and the Adam update
// (torch.optim.Adam.step), as three launches over a table of tensors.  fp32 data on the vector ALU, the sums of squares and the
// bias corrections in fp64.  No atomics, no host synchronisation, every sum in an order fixed by the element counts: results are
// bit-identical from run to run.
//
// Layout of every kernel: the tensors are cut into chunks of kChunk elements, a chunk never spans two tensors, and the chunk map
// names for every workgroup its row of the table and the chunk's index inside that tensor.  A workgroup is 256 lanes; lane t owns
// the element quads t, t + 256, ... of the chunk: 16-byte loads and stores when every pointer the kernel follows for that tensor
// is 16-byte aligned (a decision per tensor, hence wave-uniform), four dword accesses of the same quad otherwise -- the same
// elements in the same lanes, so the sums do not depend on which path ran.  A workgroup reads and writes nothing but its own
// chunk, its own step cell and its own partial: nothing crosses workgroups inside a launch.
#include "mk_common.hpp"

namespace {
using namespace mk;

constexpr int kThreads = 256;
constexpr int kChunk = 4096;                          // elements of a chunk (mk_optim_chunk_elems): four quads per lane
constexpr int kQuads = kChunk / (4 * kThreads);
constexpr int kReduceThreads = 1024;
typedef __attribute__((ext_vector_type(2))) double f64x2;
static_assert(sizeof(mk_optim_row) == 96, "the table's row is 12 eight-byte words (mickey_hip.h, train_optim.py)");

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the chunk of this workgroup: its row, its index inside the tensor, its first element and its element count (0: nothing to do --
// a map entry that names no row or lies past the tensor's end is skipped, never followed)
struct Chunk {
  mk_optim_row row;
  int index, n;
  long long off;
};
__device__ __forceinline__ Chunk chunk_of(const mk_optim_row* __restrict__ table, int rows, const int* __restrict__ map) {
  Chunk c;
  c.n = 0;
  const int t = map[2 * (long long)blockIdx.x];
  c.index = map[2 * (long long)blockIdx.x + 1];
  if ((unsigned)t >= (unsigned)rows || c.index < 0) return c;
  c.row = table[t];
  c.off = (long long)c.index * kChunk;
  if (c.off >= c.row.numel) return c;
  const long long left = c.row.numel - c.off;
  c.n = left < kChunk ? (int)left : kChunk;
  return c;
}

// elements e .. e + 3 of a chunk of n (those past n read as zero and are not stored)
__device__ __forceinline__ f32x4 load_quad(const float* p, int e, int n, bool vec) {
  if (vec && e + 4 <= n) return *(const f32x4*)(p + e);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (e + k < n) v[k] = p[e + k];
  return v;
}
__device__ __forceinline__ void store_quad(float* p, int e, int n, bool vec, f32x4 v) {
  if (vec && e + 4 <= n) {
    *(f32x4*)(p + e) = v;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (e + k < n) p[e + k] = v[k];
}

// the sum over the workgroup's WAVES waves, in a fixed order: the butterfly of each wave, then the waves in wave order (valid in thread 0)
template <int WAVES>
__device__ __forceinline__ double block_sum(double s, double* red) {
  s = wave_sum_d(s);
  __syncthreads();   // (the previous use of red is over)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) t += red[w];
  return t;
}

// ---- launch 1: partials[chunk] = { s, s where the row counts towards the norm else 0 }, s = the sum of g^2 over the chunk in
// double.  The square of an fp32 value cannot overflow a double, so s is non-finite exactly when the chunk holds a NaN or an Inf:
// it is the finite check as well. -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void optim_grad_stats_kernel(const mk_optim_row* __restrict__ table, int rows,
                                                                    const int* __restrict__ map, f64x2* __restrict__ partials) {
  __shared__ double red[4];
  const Chunk c = chunk_of(table, rows, map);
  double s = 0.0;
  if (c.n > 0) {
    const float* g = c.row.g + c.off;
    const bool vec = aligned16(g);
    f32x4 v[kQuads];
    if (vec && c.n == kChunk) {   // a full chunk: every load is issued before the first sum
#pragma unroll
      for (int i = 0; i < kQuads; ++i) v[i] = *(const f32x4*)(g + (i * kThreads + (int)threadIdx.x) * 4);
    } else {
#pragma unroll
      for (int i = 0; i < kQuads; ++i) v[i] = load_quad(g, (i * kThreads + (int)threadIdx.x) * 4, c.n, vec);   // (zeros past the end)
    }
#pragma unroll
    for (int i = 0; i < kQuads; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) s = fma((double)v[i][k], (double)v[i][k], s);
  }
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = f64x2{s, c.n > 0 && (c.row.flags & MK_OPTIM_NORM) ? s : 0.0};
}

// ---- launch 2 (one workgroup of kReduceThreads): the partials added in chunk order -- thread t adds its run of consecutive
// chunks, then the workgroup's fixed-order sum -- both columns at once: all chunks (finite: ok) and the chunks of the rows that
// count towards the norm.  state = { ok, total_norm, clip_coef, 0 }. --------------------------------------------------------------
__global__ __launch_bounds__(kReduceThreads) void optim_reduce_kernel(const f64x2* __restrict__ partials, int chunks, float max_norm,
                                                                      float* __restrict__ state) {
  __shared__ double red[kReduceThreads / 64];
  const int per = (chunks + kReduceThreads - 1) / kReduceThreads;
  const int k0 = (int)threadIdx.x * per < chunks ? (int)threadIdx.x * per : chunks;
  const int k1 = k0 + per < chunks ? k0 + per : chunks;
  double all = 0.0, counted = 0.0;
#pragma unroll 4
  for (int k = k0; k < k1; ++k) {
    const f64x2 v = partials[k];
    all += v[0];
    counted += v[1];
  }
  all = block_sum<kReduceThreads / 64>(all, red);
  counted = block_sum<kReduceThreads / 64>(counted, red);
  if (threadIdx.x == 0) {
    const bool ok = all - all == 0.0;   // (false for a NaN and for an Inf)
    const float total = (float)sqrt(counted);
    float coef = 1.0f;
    if (max_norm >= 0.f) {
      coef = max_norm / (total + 1e-6f);   // torch/nn/utils/clip_grad.py, in fp32 as there
      coef = coef < 1.0f ? coef : 1.0f;
    }
    *(f32x4*)state = f32x4{ok ? 1.0f : 0.0f, total, coef, 0.0f};
  }
}

// ---- launch 3: the Adam update of one chunk.  state[0] == 0: nothing is touched.  Every workgroup owns the step cell of its
// chunk (row.step[index]; all cells of a tensor hold the same count), so that no workgroup reads a cell another one writes. ---------
__global__ __launch_bounds__(kThreads) void optim_adam_kernel(const mk_optim_row* __restrict__ table, int rows,
                                                              const int* __restrict__ map, const float* __restrict__ state) {
  if (state[0] == 0.f) return;
  const float coef = state[2];
  const Chunk c = chunk_of(table, rows, map);
  if (c.n == 0 || !(c.row.flags & MK_OPTIM_PARAM)) return;
  float* cell = c.row.step + c.index;
  const float t = *cell + 1.0f;
  __syncthreads();   // (every lane has read the cell)
  if (threadIdx.x == 0) *cell = t;
  // once per workgroup, in double (torch/optim/adam.py takes them from Python floats)
  const double bc1 = 1.0 - pow(c.row.beta1, (double)t), bc2 = 1.0 - pow(c.row.beta2, (double)t);
  const float step_size = (float)(c.row.lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  const float b1 = (float)c.row.beta1, b2 = (float)c.row.beta2, ob1 = (float)(1.0 - c.row.beta1), ob2 = (float)(1.0 - c.row.beta2);
  const float eps = (float)c.row.eps, wd = (float)c.row.weight_decay;
  float *p = c.row.p + c.off, *g = c.row.g + c.off, *m = c.row.m + c.off, *v = c.row.v + c.off;
  const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);
  const bool clip = coef < 1.0f;
#pragma unroll
  for (int i = 0; i < kQuads; ++i) {
    const int e = (i * kThreads + (int)threadIdx.x) * 4;
    if (e >= c.n) continue;
    f32x4 pv = load_quad(p, e, c.n, vec), gv = load_quad(g, e, c.n, vec), mv = load_quad(m, e, c.n, vec), vv = load_quad(v, e, c.n, vec);
    if (clip) {
      gv *= coef;
      store_quad(g, e, c.n, vec, gv);
    }
    if (wd != 0.f) gv += wd * pv;
    mv = b1 * mv + ob1 * gv;
    vv = b2 * vv + ob2 * (gv * gv);
#pragma unroll
    for (int k = 0; k < 4; ++k) pv[k] -= step_size * (mv[k] / (sqrtf(vv[k]) / bc2_sqrt + eps));
    store_quad(m, e, c.n, vec, mv);
    store_quad(v, e, c.n, vec, vv);
    store_quad(p, e, c.n, vec, pv);
  }
}

bool table_ok(const void* table, int rows, const int* map, int chunks) {
  return table && ((uintptr_t)table & 7) == 0 && rows > 0 && map && ((uintptr_t)map & 3) == 0 && chunks > 0;
}

}  // namespace

extern "C" {

int mk_optim_chunk_elems(void) { return kChunk; }

long long mk_optim_chunks(long long numel) { return numel > 0 ? (numel + kChunk - 1) / kChunk : 0; }

int mk_optim_grad_stats(const mk_optim_row* table, int rows, const int* chunk_map, int chunks, double* partials, mk_stream_t stream) {
  MK_CHECK_ARG(table_ok(table, rows, chunk_map, chunks), "mk_optim_grad_stats: needs an 8-byte aligned table of rows >= 1 rows and a chunk map of chunks >= 1 entries");
  MK_CHECK_ARG(partials && ((uintptr_t)partials & 15) == 0, "mk_optim_grad_stats: partials must be 16-byte aligned");
  hipLaunchKernelGGL(optim_grad_stats_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, (hipStream_t)stream, table, rows, chunk_map,
                     (f64x2*)partials);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_optim_reduce(const double* partials, int chunks, float max_norm, float* state, mk_stream_t stream) {
  MK_CHECK_ARG(partials && ((uintptr_t)partials & 15) == 0 && chunks > 0, "mk_optim_reduce: needs 16-byte aligned partials of chunks >= 1 chunks");
  MK_CHECK_ARG(state && ((uintptr_t)state & 15) == 0, "mk_optim_reduce: state must be 16-byte aligned");
  MK_CHECK_ARG(max_norm == max_norm && max_norm <= 3.4e38f, "mk_optim_reduce: max_norm must be a finite number (negative: no clipping)");
  hipLaunchKernelGGL(optim_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, (hipStream_t)stream, (const f64x2*)partials, chunks, max_norm, state);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

int mk_optim_adam(const mk_optim_row* table, int rows, const int* chunk_map, int chunks, const float* state, mk_stream_t stream) {
  MK_CHECK_ARG(table_ok(table, rows, chunk_map, chunks), "mk_optim_adam: needs an 8-byte aligned table of rows >= 1 rows and a chunk map of chunks >= 1 entries");
  MK_CHECK_ARG(state && ((uintptr_t)state & 15) == 0, "mk_optim_adam: state must be 16-byte aligned");
  hipLaunchKernelGGL(optim_adam_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, (hipStream_t)stream, table, rows, chunk_map, state);
  MK_CHECK_LAUNCH();
  return MK_OK;
}

}  // extern "C"
