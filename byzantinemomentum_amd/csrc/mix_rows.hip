// mix_rows.hip — bm_mix_rows: n_out averages over subsets of the n rows from ONE read of the rows (nearest-neighbour
// mixing with the masks of bm_nnm_masks_device, bucketing with one mask per bucket).  A lane loads the N values of its
// VEC columns once, forms y_0 .. y_{n_out-1} one after the other (mix_kernels.h) and stores each as it is formed:
// 4 d (n + n_out) bytes.
#include "mix_kernels.h"

namespace bm {

// Registers: N * VEC values of the lane's columns stay live through the loop over the output rows.
template <int N>
constexpr int mix_max_vec() {
  return N <= 28 ? 4 : 2;
}

template <int N>
static int launch_mix_n(const float* const* rows_host, const uint64_t* masks, int n_out, int64_t d_all,
                        float* const* out_host, hipStream_t stream) {
  RowTable tab{};
  OutTable out{};
  for (int i = 0; i < N; ++i) tab.p[i] = rows_host[i];
  for (int r = 0; r < n_out; ++r) out.p[r] = out_host[r];
  // pieces of 2^29 columns (BM_WSUM_PIECE: a smaller piece, so that a test walks several at a small d); the width of a
  // piece follows the alignment of its own first column
  const int64_t piece = tuning().wsum_piece > 0 ? (int64_t)tuning().wsum_piece : kMaxColsPerLaunch;
  return for_pieces(d_all, [&](int64_t lo, int64_t d) {
    const RowTable t = tab.advanced(lo);
    const OutTable o = out.advanced(lo);
    const int vec = Alignment().of(t.p, N).of(o.p, n_out).vec();
    // (the d % VEC trailing columns are one more column group of the same launch)
    return for_body_and_tail<mix_max_vec<N>()>(Tail::kRides, vec, d, kColBlock, caps_of(kColMaxBlocks), [&](auto width, const Span& sp) {
      hipLaunchKernelGGL((mix_rows_kernel<N, decltype(width)::value>), dim3(sp.grid), dim3(kColBlock), 0, stream, t, o,
                         masks, n_out, sp.count, sp.tail);
      BM_LAUNCH_CHECK();
      return 0;
    });
  }, piece);
}

template <int... Ns>
static int mix_dispatch(std::integer_sequence<int, Ns...>, const float* const* rows, int n, const uint64_t* masks,
                        int n_out, int64_t d, float* const* out_rows, hipStream_t stream) {
  int rc = BM_EINVAL;
  ((n == Ns + 1 ? (rc = launch_mix_n<Ns + 1>(rows, masks, n_out, d, out_rows, stream), 0) : 0), ...);
  return rc;
}

static bool overlap(const float* a, const float* b, int64_t d) { return a < b + d && b < a + d; }

}  // namespace bm

extern "C" int bm_mix_rows(const float* const* rows, int n, const uint64_t* masks_dev, int n_out, int64_t d,
                           float* const* out_rows, void* stream) {
  using namespace bm;
  if (rows == nullptr || masks_dev == nullptr || out_rows == nullptr || n < 1 || n > BM_MAX_ROWS || n_out < 1 ||
      n_out > BM_MAX_ROWS || d < 0)
    return BM_EINVAL;
  if (d == 0) return 0;
  for (int i = 0; i < n; ++i)
    if (rows[i] == nullptr) return BM_EINVAL;
  // inputs may be one pointer several times; an output is written while the inputs of other columns are still being
  // read, so it may touch neither an input nor another output
  for (int r = 0; r < n_out; ++r) {
    if (out_rows[r] == nullptr) return BM_EINVAL;
    for (int i = 0; i < n; ++i)
      if (overlap(out_rows[r], rows[i], d)) return BM_EINVAL;
    for (int s = 0; s < r; ++s)
      if (overlap(out_rows[r], out_rows[s], d)) return BM_EINVAL;
  }
  return mix_dispatch(std::make_integer_sequence<int, BM_MAX_ROWS>{}, rows, n, masks_dev, n_out, d, out_rows,
                      static_cast<hipStream_t>(stream));
}
