// anticge.hip — the reference's `anticge` attack (attacks/anticge.py:49-78) as one short chain on the device.
//
// Replaces (reference, PyTorch):
//   sorted(((byznorm(grad), grad) for grad in grads), key=...)     anticge.py:37-47   h x norm().item()
//   attack = normed[0][1].clone(); for ...: attack.add_(grad)      anticge.py:70-72   one pass per row
//   attnorm = attack.norm().item(); attack.mul_(-maxnorm/attnorm)  anticge.py:74-76   a host round trip, two passes
// bm_anticge_sum: rank the rows from their squared norms (one workgroup), then ONE pass over the selected rows that
// writes their sum S in the reference's order of additions and leaves |S|^2 (fp64, fixed reduction tree, no float
// atomics); bm_anticge_scale: S *= -nextafter(norm_(maxpos), 0) / |S| from the two scalars where they are.  Nothing
// synchronises with the host; under sharding the caller all-reduces ONE double between the two calls.
#include "rank_body.h"
#include "table_sum.h"

namespace bm {

constexpr int kAcgScaleBlock = 256;  // lanes per workgroup of the scaling kernel (the sum: kTableBlock, table_sum.h)
constexpr int kAcgMaxBlocks = 256 * 32;  // workgroups of the plain form per piece of the pass
constexpr Caps kAcgCaps = caps_of(kAcgMaxBlocks);  // one fp64 partial per workgroup: at most kAcgCaps.sets() per piece
constexpr int kAcgScaleBlocks = 2048;

// The rows by increasing squared norm (non-finite as +inf, ties to the lower index: anticge.py:44-47 with Python's
// stable sort) and the squared norm of the row of rank `maxpos`, the first one the attack leaves out.
__global__ __launch_bounds__(64) void anticge_rank_kernel(const double* __restrict__ row_sq, int h, int maxpos,
                                                          int32_t* __restrict__ order, int32_t* __restrict__ order_out,
                                                          double* __restrict__ scal_out) {
  __shared__ double keys[BM_MAX_ROWS];
  __shared__ int32_t ranked[BM_MAX_ROWS];
  const int i = threadIdx.x;
  double key = i < h ? row_sq[i] : 0.0;
  if (!(__builtin_fabs(key) < __builtin_inf())) key = __builtin_inf();
  stable_argsort_body(key, h, keys, ranked);
  __syncthreads();
  order[i] = i < h ? ranked[i] : 0;
  if (order_out != nullptr) order_out[i] = i < h ? ranked[i] : 0;
  if (i == 0) scal_out[1] = keys[ranked[maxpos]];
}

// sum_out = ((g_(0) + g_(0)) + g_(1)) + ... + g_(maxpos-1), sequential fp32 per coordinate: `attack = g_(0).clone()`
// followed by one `attack.add_(g)` per selected row, g_(0) first (anticge.py:70-72; with maxpos = 0 the clone alone).
// One fp64 partial of sum_j S_j^2 per workgroup: every product exact in fp64, lanes and waves through the fixed tree.
template <int VEC>
__global__ __launch_bounds__(kTableBlock) void anticge_sum_kernel(RowTable rows, const int32_t* __restrict__ order,
                                                                int maxpos, int64_t nvec, float* __restrict__ out,
                                                                int tail, double* __restrict__ partial) {
  __shared__ const float* sel[BM_MAX_ROWS];
  __shared__ double red[kTableBlock / 64];
  const int m = maxpos > 0 ? maxpos : 1;  // rows read
  if ((int)threadIdx.x < m) sel[threadIdx.x] = rows.p[load_index_coherent(order + threadIdx.x) & (BM_MAX_ROWS - 1)];
  __syncthreads();
  double wide = 0.0;
  table_sum_plain<VEC>(sel, m, nvec, tail, out, AnticgeFold{maxpos > 0}, [&](float x) { wide += (double)x * (double)x; });
  const double r = block_reduce_sum<kTableBlock>(wide, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// one wave: lane l adds the partials l, l + 64, ... in launch order, then the fixed shuffle tree
__global__ __launch_bounds__(64) void anticge_finish_kernel(const double* __restrict__ partial, int nparts,
                                                            double* __restrict__ scal_out) {
  const int lane = threadIdx.x;
  double tot = 0.0;
  for (int b = lane; b < nparts; b += 64) tot += partial[b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
  if (lane == 0) scal_out[0] = tot;
}

// The multiplier of anticge.py:68,74-76 from scal = { |S|^2, |g_(maxpos)|^2 }: both norms are the fp32 numbers
// `.norm().item()` hands to Python, `nextafter(norm, 0)` and the quotient are taken in double, and `mul_` with a Python
// scalar rounds it to fp32 once.  A norm of S that is not > 0 (zero, NaN) leaves S as it is.
__device__ __forceinline__ bool anticge_multiplier(const double* __restrict__ scal, float* mult) {
  const float attnorm = (float)sqrt(scal[0]);
  if (!(attnorm > 0.0f)) return false;
  const float byznorm = (float)sqrt(scal[1]);
  const double norm = (__builtin_fabsf(byznorm) < __builtin_inff()) ? (double)byznorm : __builtin_inf();
  *mult = (float)(-nextafter(norm, 0.0) / (double)attnorm);
  return true;
}

template <int VEC>
__global__ __launch_bounds__(kAcgScaleBlock) void anticge_scale_kernel(float* __restrict__ vec, int64_t nvec,
                                                                  const double* __restrict__ scal) {
  float mult;
  if (!anticge_multiplier(scal, &mult)) return;
  using T = typename VecLoad<VEC>::T;
  const int64_t stride = (int64_t)gridDim.x * kAcgScaleBlock;
  for (int64_t v = (int64_t)blockIdx.x * kAcgScaleBlock + threadIdx.x; v < nvec; v += stride) {
    T x = *reinterpret_cast<const T*>(vec + v * VEC);
    if constexpr (VEC == 1) {
      x = x * mult;
    } else {
#pragma unroll
      for (int c = 0; c < VEC; ++c) x[c] = x[c] * mult;
    }
    *reinterpret_cast<T*>(vec + v * VEC) = x;
  }
}

// workspace: the ranking (BM_MAX_ROWS int32), then one fp64 partial per workgroup of every piece of the pass
constexpr int64_t kAcgOrderBytes = BM_MAX_ROWS * (int64_t)sizeof(int32_t);

}  // namespace bm

extern "C" int64_t bm_anticge_workspace_bytes(int64_t d) {
  using namespace bm;
  if (d < 0) return BM_EINVAL;
  const int64_t pieces = piece_count(d) > 0 ? piece_count(d) : 1;
  return kAcgOrderBytes + pieces * kAcgCaps.sets() * (int64_t)sizeof(double);
}

extern "C" int bm_anticge_sum(const float* const* rows, int h, int64_t d, int f_decl, const double* row_sq,
                              float* sum_out, int32_t* order_out, double* scal_out, void* ws, void* stream) {
  using namespace bm;
  if (rows == nullptr || row_sq == nullptr || scal_out == nullptr || ws == nullptr || h < 1 || h > BM_MAX_ROWS ||
      f_decl < 1 || f_decl > h || d < 0 || (d > 0 && sum_out == nullptr))
    return BM_EINVAL;
  for (int i = 0; i < h && d > 0; ++i)
    if (rows[i] == nullptr) return BM_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int maxpos = h - f_decl;
  int32_t* order = static_cast<int32_t*>(ws);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(ws) + kAcgOrderBytes);
  hipLaunchKernelGGL(anticge_rank_kernel, dim3(1), dim3(64), 0, s, row_sq, h, maxpos, order, order_out, scal_out);
  BM_LAUNCH_CHECK();
  RowTable tab{};
  for (int i = 0; i < h; ++i) tab.p[i] = rows[i];
  const int vec = Alignment().of(rows, h).of(sum_out).vec();
  int nparts = 0;
  // (the d % VEC trailing columns ride in the last workgroup of a piece's launch: no launch, no partial of their own)
  const int rc = for_pieces(d, [&](int64_t lo, int64_t dp) {
    return for_body_and_tail<4>(Tail::kRidesNarrowed, vec, dp, kTableBlock, kAcgCaps, [&](auto width, const Span& sp) {
      hipLaunchKernelGGL(anticge_sum_kernel<decltype(width)::value>, dim3(sp.grid), dim3(kTableBlock), 0, s,
                         tab.advanced(lo), order, maxpos, sp.count, sum_out + lo, sp.tail, partial + sp.part);
      BM_LAUNCH_CHECK();
      return 0;
    }, &nparts);
  });
  if (rc != 0) return rc;
  // d == 0 (an empty shard): no partial at all, the finish kernel writes zero and every rank reaches its collective
  hipLaunchKernelGGL(anticge_finish_kernel, dim3(1), dim3(64), 0, s, partial, nparts, scal_out);
  BM_LAUNCH_CHECK();
  return 0;
}

extern "C" int bm_anticge_scale(float* vec, int64_t d, const double* scal, void* stream) {
  using namespace bm;
  if (scal == nullptr || d < 0 || (d > 0 && vec == nullptr)) return BM_EINVAL;
  if (d == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return for_body_and_tail<4>(Tail::kOwnLaunch, Alignment().of(vec).vec(), d, kAcgScaleBlock, caps_of(kAcgScaleBlocks),
                              [&](auto width, const Span& sp) {
    hipLaunchKernelGGL(anticge_scale_kernel<decltype(width)::value>, dim3(sp.grid), dim3(kAcgScaleBlock), 0, s,
                       vec + sp.first, sp.count, scal);
    BM_LAUNCH_CHECK();
    return 0;
  });
}
