// table_sum.h — sums over a list of rows, one column at a time in a fixed order (device code only): ONE column body,
// its three folds and the two drivers that walk the columns.  A kernel is its own prologue, which fills `sel` (the rows
// in the order they are added, in LDS), and one call of a driver: selected_mean(_burst)_kernel (reduce.hip),
// anticge_sum_kernel (anticge.hip), weighted_sum_kernel (weighted_sum.hip).  A burst form of another fold is one more
// instantiation of table_sum_burst and a threshold to measure.
#pragma once
#include "bm_common.h"

namespace bm {

constexpr int kTableBlock = 256;  // lanes per workgroup of the plain driver
// A fold: start(x_0) of row 0 as loaded when kFromFirstRow (m >= 1), else start(0); fold(k, x_k, acc) for the other k; finish.
// (((0 + x_0) + x_1) + ...) / fm, one IEEE division; fm is NaN when the index table holds a negative index.
struct MeanFold {
  static constexpr bool kFromFirstRow = false;
  float fm;
  __device__ __forceinline__ float start(float) const { return 0.0f; }
  __device__ __forceinline__ float fold(int, float x, float acc) const { return acc + x; }
  __device__ __forceinline__ float finish(float acc) const { return acc / fm; }
};
// `attack = g_(0).clone()`, then one `add_` per selected row, g_(0) first: the row of rank 0 AS LOADED (0 + x would
// lose the sign of -0), read once and doubled iff a row is selected at all.
struct AnticgeFold {
  static constexpr bool kFromFirstRow = true;
  bool twice;
  __device__ __forceinline__ float start(float x) const { return twice ? x + x : x; }
  __device__ __forceinline__ float fold(int, float x, float acc) const { return acc + x; }
  __device__ __forceinline__ float finish(float acc) const { return acc; }
};
// acc = init, then acc = fmaf(w_k, x_k, acc); init is 0, or NaN with m = 0 when a weight is NaN (no row is read).
struct WeightedFold {
  static constexpr bool kFromFirstRow = false;
  const float* wt;
  float init;
  __device__ __forceinline__ float start(float) const { return init; }
  __device__ __forceinline__ float fold(int k, float x, float acc) const { return __builtin_fmaf(wt[k], x, acc); }
  __device__ __forceinline__ float finish(float acc) const { return acc; }
};
struct NoObserver { __device__ __forceinline__ void operator()(float) const {} };

// The column body: column group v (VEC columns) of every row, streamed.
template <int VEC, class Fold>
__device__ __forceinline__ void table_columns(const float* const* sel, int m, int64_t v, const Fold& f, float (&acc)[VEC]) {
  int k = 0;
  for (int c = 0; c < VEC; ++c) acc[c] = 0.0f;
  if constexpr (Fold::kFromFirstRow) load_stream<VEC>(sel[k++] + v * VEC, acc);
  for (int c = 0; c < VEC; ++c) acc[c] = f.start(acc[c]);
#pragma unroll 8
  for (; k < m; ++k) {
    float t[VEC];
    load_stream<VEC>(sel[k] + v * VEC, t);
    for (int c = 0; c < VEC; ++c) acc[c] = f.fold(k, t[c], acc[c]);
  }
  for (int c = 0; c < VEC; ++c) acc[c] = f.finish(acc[c]);
}

// Its scalar twin over the d % VEC trailing columns: one lane each, in the last workgroup (no second launch; none at VEC = 1).
template <int VEC, class Fold, class Observe>
__device__ __forceinline__ void table_sum_tail(const float* const* sel, int m, int64_t nvec, int tail,
                                               float* __restrict__ out, const Fold& f, Observe&& observe) {
  if (VEC > 1 && blockIdx.x == gridDim.x - 1 && (int)threadIdx.x < tail) {
    const int64_t j = nvec * VEC + threadIdx.x;
    int k = 0;
    float acc = 0.0f;
    if constexpr (Fold::kFromFirstRow) acc = sel[k++][j];
    acc = f.start(acc);
    for (; k < m; ++k) acc = f.fold(k, sel[k][j], acc);
    out[j] = acc = f.finish(acc);
    observe(acc);
  }
}

// The plain driver: blocks of kTableBlock column groups, grid-stride, one non-temporal store per group; observe(x) sees
// every result of a lane: block by block, c = 0 .. VEC-1, then the tail.  Never returns early (a block reduction may follow).
template <int VEC, class Fold, class Observe = NoObserver>
__device__ __forceinline__ void table_sum_plain(const float* const* sel, int m, int64_t nvec, int tail,
                                                float* __restrict__ out, const Fold& f, Observe&& observe = Observe{}) {
  const int64_t nblk = (nvec + kTableBlock - 1) / kTableBlock;
  for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    const int64_t v = b * kTableBlock + threadIdx.x;
    if (v >= nvec) continue;
    float acc[VEC];
    table_columns<VEC>(sel, m, v, f, acc);
    store_stream<VEC>(out + v * VEC, acc);
    for (int c = 0; c < VEC; ++c) observe(acc[c]);
  }
  table_sum_tail<VEC>(sel, m, nvec, tail, out, f, observe);
}

// The burst driver for long rows of 16-byte columns: one workgroup of THREADS lanes per CU, column groups interleaved
// across the CUs, the results of SLOTS iterations staged in LDS, a barrier, then written back to back — the recipe of
// colwise_burst_kernel (colwise_kernels.h), where the why is written down.  Same body, same bits.  nvec < 2^30.
template <int THREADS, int SLOTS, class Fold>
__device__ __forceinline__ void table_sum_burst(const float* const* sel, int m, int64_t nvec, int tail,
                                                float* __restrict__ out, const Fold& f) {
  using V = typename VecLoad<4>::T;
  __shared__ V stage[SLOTS * THREADS];
  const uint32_t tid = threadIdx.x, nv = (uint32_t)nvec, span = gridDim.x * THREADS;
  const uint32_t iters = (nv + span - 1) / span, first = blockIdx.x * THREADS + tid;
  for (uint32_t p0 = 0; p0 < iters; p0 += SLOTS) {
    const uint32_t p1 = (p0 + SLOTS < iters) ? p0 + SLOTS : iters;
    for (uint32_t it = p0; it < p1; ++it) {
      const uint32_t v = it * span + first;
      if (v < nv) {
        float acc[4];
        table_columns<4>(sel, m, (int64_t)v, f, acc);
        stage[(it - p0) * THREADS + tid] = V{acc[0], acc[1], acc[2], acc[3]};
      }
    }
    __syncthreads();  // what makes the stores below a burst
    for (uint32_t it = p0; it < p1; ++it) {
      const uint32_t v = it * span + first;
      if (v < nv) __builtin_nontemporal_store(stage[(it - p0) * THREADS + tid], reinterpret_cast<V*>(out) + v);
    }
  }
  table_sum_tail<4>(sel, m, nvec, tail, out, f, NoObserver{});
}

}  // namespace bm
