// colwise_bucketed_dispatch.h — device code and launch logic of bm_colwise_bucketed (contract: include/bm_gar.h), shared
// by colwise_bucketed_{median,trmean}_s{2,3}.hip: one rule and one bucket size each, so that the instances compile side
// by side.  The mixing is mix_kernels.h's as it stands (mix_prologue, mix_entry, mix_one, all_finite, mix_load, mix_store:
// the bits of bm_mix_rows); what is new is that the NOUT < N mixed values of a column stay in registers and go to
// column_rule<NOUT, OP>: the stack is read once and d floats are written, 4 d (N + 1) bytes, where bm_mix_rows followed by
// bm_colwise moves 4 d (N + 2 NOUT + 1).
#pragma once
#include "mix_kernels.h"

namespace bm {

// The fused form exists for the bucket counts of s = 2 and s = 3, NOUT = ceil(N / 2) and ceil(N / 3), for
// 2 .. bucketed_max_rows(s) rows; any other shape has no instance and the caller runs bm_mix_rows and bm_colwise
// (gars.bucketing).  Decided per bucket size by measurement against that composition (profiles/bucketing_timings.txt,
// d = 11.2 M, the composition's own repeated series apart by at most 0.006): fused / composed = 0.50-0.60 at 11 rows,
// 0.50-0.56 at 25, 0.57-0.59 at 36, 0.70-0.76 at 44; at 51 rows s = 3 still wins (0.71-0.73: 51 * 17 pairs per column)
// and s = 2 does not (1.00-1.03: 51 * 26).  s = 2 keeps its instances up to 44 rows, the largest count measured at which
// it wins (45 .. 50 were not measured); s = 3 up to 51, the largest count measured at all.
constexpr int kBucketedMaxRows = 51;    // the largest row count with any instance: s = 3's
constexpr int kBucketedMaxRowsS2 = 44;  // s = 2's
constexpr int bucketed_max_rows(int s) { return s == 2 ? kBucketedMaxRowsS2 : kBucketedMaxRows; }

constexpr int bucketed_n_out(int n, int s) { return (n + s - 1) / s; }

// x and y are both live: (N + NOUT) * VEC registers.  Four columns per lane while that is at most 96 values (68 at 11
// rows, s = 2), two up to 25 rows (2 * 38 = 76 values: under 128 VGPRs, four waves per SIMD; four columns would be 152),
// two beyond as well: 124 VGPRs at 36 rows, 151 at 44 (s = 2), 153 at 51 (s = 3), no spill.
template <int N, int NOUT>
constexpr int bucketed_max_vec() {
  return (N + NOUT) * 4 <= 96 ? 4 : 2;
}

template <int N, int NOUT, int VEC, bool FINITE, int R>
__device__ __forceinline__ void bucket_into(const float (&x)[VEC][N], const MixEntry* entries, float (&y)[VEC][NOUT]) {
  float t[VEC];
  mix_one<N, VEC, FINITE>(x, mix_entry(entries, R), t);
#pragma unroll
  for (int c = 0; c < VEC; ++c) y[c][R] = t[c];
}

// (a fold, not a loop, for the reason given at mix_all: y must keep static indices)
template <int N, int NOUT, int VEC, bool FINITE, size_t... R>
__device__ __forceinline__ void bucket_all_impl(const float (&x)[VEC][N], const MixEntry* entries, float (&y)[VEC][NOUT],
                                                std::index_sequence<R...>) {
  (bucket_into<N, NOUT, VEC, FINITE, (int)R>(x, entries, y), ...);
}

template <int N, int NOUT, int VEC, bool FINITE>
__device__ __forceinline__ void bucket_all(const float (&x)[VEC][N], const MixEntry* entries, float (&y)[VEC][NOUT]) {
  bucket_all_impl<N, NOUT, VEC, FINITE>(x, entries, y, std::make_index_sequence<NOUT>{});
}

template <int N, int NOUT, int OP, int VEC>
__global__ __launch_bounds__(kColBlock) void colwise_bucketed_kernel(RowTable rows, const uint64_t* __restrict__ masks,
                                                                     int64_t nvec, int tail, int f, float inv_keep,
                                                                     float* __restrict__ out) {
  static_assert(NOUT >= 1 && NOUT <= N && N <= BM_MAX_ROWS, "a bucketed instance mixes N rows into at most N");
  __shared__ MixEntry entries[BM_MAX_ROWS];
  mix_prologue<N>(masks, NOUT, entries);
  // nvec * VEC * 4 <= 2^31 (the host cuts longer rows into pieces): 32-bit byte offsets
  const uint32_t nv = (uint32_t)nvec, groups = nv + (tail > 0 ? 1u : 0u);
  const uint32_t stride = gridDim.x * kColBlock;
  for (uint32_t g = blockIdx.x * kColBlock + threadIdx.x; g < groups; g += stride) {
    float x[VEC][N], y[VEC][NOUT];
    mix_load<N, VEC>(rows, g, nv, tail, x);
    if (all_finite<N, VEC>(x))
      bucket_all<N, NOUT, VEC, true>(x, entries, y);
    else
      bucket_all<N, NOUT, VEC, false>(x, entries, y);
    float r[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) r[c] = column_rule<NOUT, OP>(y[c], f, inv_keep, nullptr);
    mix_store<VEC>(out, g, nv, tail, r);
  }
}

template <int N, int NOUT, int OP>
static int launch_bucketed_n(const float* const* rows_host, const uint64_t* masks, int64_t d_all, int f, float* out_all,
                             hipStream_t stream) {
  const int keep = (OP == BM_OP_TRMEAN) ? (NOUT - 2 * f) : (NOUT - f);
  const float inv_keep = 1.0f / (float)(keep > 0 ? keep : 1);
  RowTable tab{};
  for (int i = 0; i < N; ++i) tab.p[i] = rows_host[i];
  const int64_t piece = tuning().wsum_piece > 0 ? (int64_t)tuning().wsum_piece : kMaxColsPerLaunch;
  return for_pieces(d_all, [&](int64_t lo, int64_t d) {
    const RowTable t = tab.advanced(lo);
    float* const o = out_all + lo;
    const int vec = Alignment().of(t.p, N).of(o).vec();
    return for_body_and_tail<bucketed_max_vec<N, NOUT>()>(Tail::kRides, vec, d, kColBlock, caps_of(kColMaxBlocks), [&](auto width, const Span& sp) {
      hipLaunchKernelGGL((colwise_bucketed_kernel<N, NOUT, OP, decltype(width)::value>), dim3(sp.grid), dim3(kColBlock), 0,
                         stream, t, masks, sp.count, sp.tail, f, inv_keep, o);
      BM_LAUNCH_CHECK();
      return 0;
    });
  }, piece);
}

// The instance of N rows in buckets of S, NOUT = ceil(N / S).  At N = 2 and 4 the bucket counts of S = 2 and S = 3 are one
// number: the instance belongs to S = 2 alone, so that no kernel is made in two translation units.
template <int N, int S, int OP>
static int launch_bucketed(int n_out, const float* const* rows, const uint64_t* masks, int64_t d, int f, float* out,
                           hipStream_t stream) {
  constexpr int NOUT = bucketed_n_out(N, S);
  if constexpr (S == 3 && NOUT == bucketed_n_out(N, 2)) {
    return BM_EINVAL;
  } else {
    if (n_out != NOUT) return BM_EINVAL;
    return launch_bucketed_n<N, NOUT, OP>(rows, masks, d, f, out, stream);
  }
}

template <int OP, int S, int LO, int... Ns>
static int bucketed_dispatch_n(std::integer_sequence<int, Ns...>, const float* const* rows, int n, const uint64_t* masks,
                               int n_out, int64_t d, int f, float* out, hipStream_t stream) {
  int rc = BM_EINVAL;
  ((n == Ns + LO ? (rc = launch_bucketed<Ns + LO, S, OP>(n_out, rows, masks, d, f, out, stream), 0) : 0), ...);
  return rc;
}

// the rule OP on the means of buckets of S for any n = LO .. HI; BM_EINVAL where n_out is not ceil(n / S)
template <int OP, int S, int LO, int HI>
static int colwise_bucketed_dispatch(const float* const* rows, int n, const uint64_t* masks, int n_out, int64_t d, int f,
                                     float* out, hipStream_t stream) {
  return bucketed_dispatch_n<OP, S, LO>(std::make_integer_sequence<int, HI - LO + 1>{}, rows, n, masks, n_out, d, f, out,
                                        stream);
}

}  // namespace bm
