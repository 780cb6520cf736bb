// colwise_mixed_dispatch.h — launch logic of bm_colwise_mixed (contract: include/bm_gar.h; device code: mix_kernels.h),
// shared by colwise_mixed_median.hip and colwise_mixed_trmean.hip: one rule each, n = 1 .. kMixedMaxRows rows, so that
// the instances (N * N unrolled pairs each) compile side by side.
#pragma once
#include "mix_kernels.h"

namespace bm {

// The fused form exists up to this row count: beyond it the mixed rows are written and the plain rule reads them
// (gars.nnm).  Decided by measurement against that composition (profiles/nnm_timings.txt, d = 11.2 M): fused / composed
// = 0.37-0.38 at 11 rows, 0.56-0.59 at 25, 0.73-0.79 at 36, but 1.00-1.15 at 38, 40, 45 and 51 rows, at two columns per
// lane and at one alike — the N * N pairs per column outgrow what the saved 2 N row passes cost.
constexpr int kMixedMaxRows = 36;
// x and y are both live: 2 * N * VEC registers.  Two columns per lane: 118 VGPRs at 25 rows (four waves per SIMD), 163
// at 36 (three).
constexpr int kMixedMaxVec = 2;

template <int N, int OP>
static int launch_mixed_n(const float* const* rows_host, const uint64_t* masks, int64_t d_all, int f, float* out_all,
                          hipStream_t stream) {
  const int keep = (OP == BM_OP_TRMEAN) ? (N - 2 * f) : (N - f);
  const float inv_keep = 1.0f / (float)(keep > 0 ? keep : 1);
  RowTable tab{};
  for (int i = 0; i < N; ++i) tab.p[i] = rows_host[i];
  const int64_t piece = tuning().wsum_piece > 0 ? (int64_t)tuning().wsum_piece : kMaxColsPerLaunch;
  return for_pieces(d_all, [&](int64_t lo, int64_t d) {
    const RowTable t = tab.advanced(lo);
    float* const o = out_all + lo;
    const int vec = Alignment().of(t.p, N).of(o).vec();
    return for_body_and_tail<kMixedMaxVec>(Tail::kRides, vec, d, kColBlock, caps_of(kColMaxBlocks), [&](auto width, const Span& sp) {
      hipLaunchKernelGGL((colwise_mixed_kernel<N, OP, decltype(width)::value>), dim3(sp.grid), dim3(kColBlock), 0, stream,
                         t, masks, sp.count, sp.tail, f, inv_keep, o);
      BM_LAUNCH_CHECK();
      return 0;
    });
  }, piece);
}

template <int OP, int LO, int... Ns>
static int mixed_dispatch_n(std::integer_sequence<int, Ns...>, const float* const* rows, int n, const uint64_t* masks,
                            int64_t d, int f, float* out, hipStream_t stream) {
  int rc = BM_EINVAL;
  ((n == Ns + LO ? (rc = launch_mixed_n<Ns + LO, OP>(rows, masks, d, f, out, stream), 0) : 0), ...);
  return rc;
}

// the rule OP on the mixed rows for any n = LO .. HI
template <int OP, int LO, int HI>
static int colwise_mixed_dispatch(const float* const* rows, int n, const uint64_t* masks, int64_t d, int f, float* out,
                                  hipStream_t stream) {
  return mixed_dispatch_n<OP, LO>(std::make_integer_sequence<int, HI - LO + 1>{}, rows, n, masks, d, f, out, stream);
}

}  // namespace bm
