// weighted_sum.hip — out = sum_i w_i rows[i], the weights read from DEVICE memory: the last leg of the geometric median
// and of centered clipping (bm_center_weights_device leaves the weights where this kernel reads them).  ONE streaming
// pass over the rows that carry weight; per coordinate acc = 0, then acc = fmaf(w_i, x_i, acc) in index order
// (WeightedFold under the plain driver of table_sum.h; no burst form yet).
#include "table_sum.h"

namespace bm {

constexpr int kWsumMaxBlocks = 256 * 32;

// first[i] = the lowest index whose pointer is rows[i]: rows that are one pointer (the f copies of a Byzantine vector,
// attacks/identical.py:86) form one group, read once.  By value, next to the RowTable.
struct RowGroups {
  uint8_t first[BM_MAX_ROWS];
};

// The active rows of a launch, decided once per workgroup (as selected_mean_prologue, reduce.hip, builds its sel[]):
// the weight of a group is the sum of its members' fp64 weights in index order, rounded to fp32; a group whose fp32
// weight is exactly 0 is dropped (never read: an excluded NaN row cannot poison the sum); a NaN weight poisons the
// launch.  Returns the number of active groups, -1 when poisoned.  Every lane of the workgroup must call.
__device__ __forceinline__ int weighted_sum_prologue(const RowTable& rows, const RowGroups& groups,
                                                     const double* __restrict__ weights, int n, const float** sel,
                                                     float* wt, double* wd, int* count) {
  const int tid = threadIdx.x;
  if (tid < BM_MAX_ROWS) wd[tid] = tid < n ? weights[tid] : 0.0;
  __syncthreads();
  if (tid < 64) {  // wave 0: lane i is row i
    const bool lead = tid < n && groups.first[tid] == tid;
    float g = 0.0f;
    if (lead) {
      double s = 0.0;
      for (int j = tid; j < n; ++j) s += (groups.first[j] == tid) ? wd[j] : 0.0;
      g = (float)s;
    }
    const bool active = lead && g != 0.0f;  // (a NaN group weight is active, and poisons below)
    const bool bad = (tid < n && wd[tid] != wd[tid]) || (lead && g != g);
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(active);
    const unsigned long long poison = __builtin_amdgcn_ballot_w64(bad);
    if (active) {
      const int pos = __builtin_popcountll(mask & ((1ull << tid) - 1ull));
      sel[pos] = rows.p[tid];
      wt[pos] = g;
    }
    if (tid == 0) *count = poison != 0ull ? -1 : __builtin_popcountll(mask);
  }
  __syncthreads();
  return *count;
}

template <int VEC>
__global__ __launch_bounds__(kTableBlock) void weighted_sum_kernel(RowTable rows, RowGroups groups,
                                                                   const double* __restrict__ weights, int n,
                                                                   int64_t nvec, float* __restrict__ out, int tail) {
  __shared__ const float* sel[BM_MAX_ROWS];
  __shared__ float wt[BM_MAX_ROWS];
  __shared__ double wd[BM_MAX_ROWS];
  __shared__ int count;
  const int found = weighted_sum_prologue(rows, groups, weights, n, sel, wt, wd, &count);
  const int m = found < 0 ? 0 : found;
  const float init = found < 0 ? __builtin_nanf("") : 0.0f;  // a NaN weight: NaN everywhere, no row read
  table_sum_plain<VEC>(sel, m, nvec, tail, out, WeightedFold{wt, init});
}

}  // namespace bm

extern "C" int bm_weighted_sum(const float* const* rows, int n, const double* weights_dev, int64_t d, float* out,
                               void* stream) {
  using namespace bm;
  if (rows == nullptr || weights_dev == nullptr || (out == nullptr && d > 0) || n < 1 || n > BM_MAX_ROWS || d < 0)
    return BM_EINVAL;
  if (d == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  RowTable tab{};
  RowGroups grp{};
  for (int i = 0; i < n; ++i) {
    tab.p[i] = rows[i];
    int first = i;
    for (int j = 0; j < i; ++j)
      if (rows[j] == rows[i]) {
        first = j;
        break;
      }
    grp.first[i] = (uint8_t)first;
  }
  // pieces of 2^29 columns (BM_WSUM_PIECE: a smaller piece, so that a test walks several at a small d); the width of
  // a piece follows the alignment of its own first column
  const int64_t piece = tuning().wsum_piece > 0 ? (int64_t)tuning().wsum_piece : kMaxColsPerLaunch;
  return for_pieces(d, [&](int64_t lo, int64_t dp) {
    const RowTable t = tab.advanced(lo);
    float* const o = out + lo;
    const int vec = Alignment().of(t.p, n).of(o).vec();
    // (the dp % VEC trailing columns ride in the last workgroup of the body's launch: no launch of their own)
    return for_body_and_tail<4>(Tail::kRidesNarrowed, vec, dp, kTableBlock, caps_of(kWsumMaxBlocks), [&](auto width, const Span& sp) {
      hipLaunchKernelGGL(weighted_sum_kernel<decltype(width)::value>, dim3(sp.grid), dim3(kTableBlock), 0, s, t, grp,
                         weights_dev, n, sp.count, o, sp.tail);
      BM_LAUNCH_CHECK();
      return 0;
    });
  }, piece);
}
