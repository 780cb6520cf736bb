// mix_kernels.h — device code of row mixing (contract: include/bm_gar.h, bm_mix_rows): output row r of a column is
//     acc = +0;  for j = 0 .. N-1 ascending, bit j of mask_r set:  acc = acc + x_j;   y_r = acc / popcount(mask_r)
// on the N register-resident values of the column (static indices, as colwise_kernel keeps them), the masks wave-uniform.
// Shared by bm_mix_rows (mix_rows.hip: y_r is stored as it is formed) and bm_colwise_mixed (colwise_mixed_*.hip: the N
// mixed values stay in registers and go to column_rule).
//
// One VALU operation per (row, output row) pair and column.  A row outside the mask must not be READ — NaN or inf
// there may not reach y_r — yet a lane predicate per pair would be N * n_out of them.  Instead the pair's bit becomes a
// wave-uniform scalar operand:
//   every loaded value of the wave finite (a ballot, once per column group): w = bit ? 1.0f : 0.0f and
//     acc = fmaf(w, x, acc), which is exactly acc + x or acc for finite x (acc is never -0: it starts at +0 and a sum
//     that cancels gives +0);
//   else: keep = bit ? ~0u : 0u and acc = acc + float(bits(x) & keep), two operations, the excluded value replaced by +0.
// The mask of an output row is re-read from LDS per column group behind an empty asm: without it the compiler hoists the
// N * n_out scalar weights out of the column loop and spills them (the comment above trimmed_sum, colwise_kernels.h,
// records what that cost once).
#pragma once
#include "colwise_kernels.h"

namespace bm {

// What a workgroup keeps per output row: the mask (bits >= N cleared), popcount as a float, its reciprocal.
struct MixEntry {
  uint32_t lo, hi;
  float count, rcount;
};

// masks: DEVICE, n_out of them.  Every lane of the workgroup must call; ends with a barrier.
template <int N>
__device__ __forceinline__ void mix_prologue(const uint64_t* __restrict__ masks, int n_out, MixEntry* entries) {
  const int tid = threadIdx.x;
  if (tid < n_out) {
    constexpr uint64_t kRows = N >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << (N & 63)) - 1);
    const uint64_t m = masks[tid] & kRows;
    const float count = (float)__builtin_popcountll(m);
    entries[tid] = MixEntry{(uint32_t)m, (uint32_t)(m >> 32), count, 1.0f / count};
  }
  __syncthreads();
}

// The entry of output row r as the column loop uses it: the mask in scalar registers, opaque to loop-invariant motion.
__device__ __forceinline__ MixEntry mix_entry(const MixEntry* entries, int r) {
  MixEntry e = entries[r];
  e.lo = __builtin_amdgcn_readfirstlane(e.lo);
  e.hi = __builtin_amdgcn_readfirstlane(e.hi);
  asm volatile("" : "+s"(e.lo), "+s"(e.hi));
  return e;
}

template <int N, int VEC>
__device__ __forceinline__ bool all_finite(const float (&x)[VEC][N]) {
  bool odd = false;
#pragma unroll
  for (int c = 0; c < VEC; ++c)
#pragma unroll
    for (int j = 0; j < N; ++j) odd |= !(__builtin_fabsf(x[c][j]) < __builtin_inff());
  return __builtin_amdgcn_ballot_w64(odd) == 0ull;  // wave-uniform
}

// The sequential sum of the rows in the mask, then the division: y[c] for the VEC columns of the lane.
template <int N, int VEC, bool FINITE>
__device__ __forceinline__ void mix_one(const float (&x)[VEC][N], const MixEntry& e, float (&y)[VEC]) {
  float acc[VEC];
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc[c] = 0.0f;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool in = (((j < 32 ? e.lo : e.hi) >> (j & 31)) & 1u) != 0u;
    if constexpr (FINITE) {
      const float w = in ? 1.0f : 0.0f;
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] = __builtin_fmaf(w, x[c][j], acc[c]);
    } else {
      const uint32_t keep = in ? 0xffffffffu : 0u;
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] = acc[c] + __uint_as_float(__float_as_uint(x[c][j]) & keep);
    }
  }
  // acc / count, one IEEE division: div_small_int gives its bits for a quotient in the normal range (and for 0 and
  // inf); an empty mask (0 / 0), a NaN or a sum small enough for a subnormal quotient takes the division itself
  bool plain = false;
#pragma unroll
  for (int c = 0; c < VEC; ++c) {
    const float a = __builtin_fabsf(acc[c]);
    plain |= !(a >= 0x1p-100f || a == 0.0f);
  }
  if (e.count == 0.0f || __builtin_amdgcn_ballot_w64(plain) != 0ull) {  // wave-uniform, rarely taken
#pragma unroll
    for (int c = 0; c < VEC; ++c) y[c] = acc[c] / e.count;
  } else {
#pragma unroll
    for (int c = 0; c < VEC; ++c) y[c] = div_small_int(acc[c], e.count, e.rcount);
  }
}

// Column group g of every row: VEC columns by one vector load per row, or — the group behind the last whole vector,
// g == nvec — the `tail` trailing columns one by one, the others 0.
template <int N, int VEC>
__device__ __forceinline__ void mix_load(const RowTable& rows, uint32_t g, uint32_t nvec, int tail, float (&x)[VEC][N]) {
  const uint32_t off = g * (uint32_t)(VEC * sizeof(float));
  if (g < nvec) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float t[VEC];
      load_stream_off<VEC>(rows.p[i], off, t);
#pragma unroll
      for (int c = 0; c < VEC; ++c) x[c][i] = t[c];
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(rows.p[i]) + off);
#pragma unroll
      for (int c = 0; c < VEC; ++c) x[c][i] = c < tail ? p[c] : 0.0f;
    }
  }
}

template <int VEC>
__device__ __forceinline__ void mix_store(float* base, uint32_t g, uint32_t nvec, int tail, const float (&y)[VEC]) {
  const uint32_t off = g * (uint32_t)(VEC * sizeof(float));
  if (g < nvec) {
    store_stream_off<VEC>(base, off, y);
  } else {
    float* p = reinterpret_cast<float*>(reinterpret_cast<char*>(base) + off);
#pragma unroll
    for (int c = 0; c < VEC; ++c)
      if (c < tail) p[c] = y[c];
  }
}

// ---------------------------------------------------------------------------------------------------
// bm_mix_rows: the loop over the output rows is a RUN-TIME loop (code linear in N), y_r stored as it is formed.
// ---------------------------------------------------------------------------------------------------
struct OutTable {
  float* p[BM_MAX_ROWS];
  OutTable advanced(int64_t by) const {
    OutTable t = *this;
    advance(t.p, by);
    return t;
  }
};

template <int N, int VEC>
__global__ __launch_bounds__(kColBlock) void mix_rows_kernel(RowTable rows, OutTable outs,
                                                             const uint64_t* __restrict__ masks, int n_out, int64_t nvec,
                                                             int tail) {
  __shared__ MixEntry entries[BM_MAX_ROWS];
  __shared__ float* dst[BM_MAX_ROWS];
  if ((int)threadIdx.x < n_out) dst[threadIdx.x] = outs.p[threadIdx.x];
  mix_prologue<N>(masks, n_out, entries);
  // nvec * VEC * 4 <= 2^31 (the host cuts longer rows into pieces): 32-bit byte offsets
  const uint32_t nv = (uint32_t)nvec, groups = nv + (tail > 0 ? 1u : 0u);
  const uint32_t stride = gridDim.x * kColBlock;
  for (uint32_t g = blockIdx.x * kColBlock + threadIdx.x; g < groups; g += stride) {
    float x[VEC][N];
    mix_load<N, VEC>(rows, g, nv, tail, x);
    if (all_finite<N, VEC>(x)) {
      for (int r = 0; r < n_out; ++r) {
        float y[VEC];
        mix_one<N, VEC, true>(x, mix_entry(entries, r), y);
        mix_store<VEC>(dst[r], g, nv, tail, y);
      }
    } else {
      for (int r = 0; r < n_out; ++r) {
        float y[VEC];
        mix_one<N, VEC, false>(x, mix_entry(entries, r), y);
        mix_store<VEC>(dst[r], g, nv, tail, y);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// bm_colwise_mixed: y_0 .. y_{N-1} formed in registers (static indices: the loop over r is unrolled) and handed to the
// rule.  No intermediate row is written: 4 d (N + 1) bytes.
// ---------------------------------------------------------------------------------------------------
template <int N, int VEC, bool FINITE, int R>
__device__ __forceinline__ void mix_into(const float (&x)[VEC][N], const MixEntry* entries, float (&y)[VEC][N]) {
  float t[VEC];
  mix_one<N, VEC, FINITE>(x, mix_entry(entries, R), t);
#pragma unroll
  for (int c = 0; c < VEC; ++c) y[c][R] = t[c];
}

// (a fold, not a loop: at the larger row counts the N * N pairs exceed the unroller's budget, and a loop it leaves rolled
//  indexes y at run time — the column lands in scratch)
template <int N, int VEC, bool FINITE, size_t... R>
__device__ __forceinline__ void mix_all_impl(const float (&x)[VEC][N], const MixEntry* entries, float (&y)[VEC][N],
                                             std::index_sequence<R...>) {
  (mix_into<N, VEC, FINITE, (int)R>(x, entries, y), ...);
}

template <int N, int VEC, bool FINITE>
__device__ __forceinline__ void mix_all(const float (&x)[VEC][N], const MixEntry* entries, float (&y)[VEC][N]) {
  mix_all_impl<N, VEC, FINITE>(x, entries, y, std::make_index_sequence<N>{});
}

template <int N, int OP, int VEC>
__global__ __launch_bounds__(kColBlock) void colwise_mixed_kernel(RowTable rows, const uint64_t* __restrict__ masks,
                                                                  int64_t nvec, int tail, int f, float inv_keep,
                                                                  float* __restrict__ out) {
  __shared__ MixEntry entries[BM_MAX_ROWS];
  mix_prologue<N>(masks, N, entries);
  const uint32_t nv = (uint32_t)nvec, groups = nv + (tail > 0 ? 1u : 0u);
  const uint32_t stride = gridDim.x * kColBlock;
  for (uint32_t g = blockIdx.x * kColBlock + threadIdx.x; g < groups; g += stride) {
    float x[VEC][N], y[VEC][N];
    mix_load<N, VEC>(rows, g, nv, tail, x);
    if (all_finite<N, VEC>(x))
      mix_all<N, VEC, true>(x, entries, y);
    else
      mix_all<N, VEC, false>(x, entries, y);
    float r[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) r[c] = column_rule<N, OP>(y[c], f, inv_keep, nullptr);
    mix_store<VEC>(out, g, nv, tail, r);
  }
}

}  // namespace bm
