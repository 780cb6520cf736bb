// mixdist.hip — bm_mixed_sqdist_device and bm_mix_weights_device: the distances between mixed rows and the weights of the
// original rows where bm_pairwise_sqdist / bm_nnm_masks_device / bm_center_weights_device / bm_krum_rank left their
// inputs, each in ONE workgroup, so that
//     distances -> masks -> mixed distances -> rule on scalars -> weights -> bm_weighted_sum
// are launches on one stream with no copy, no synchronisation and no n x d scratch.  The arithmetic is mixdist_core.h's,
// the one the host forms (mixdist.cpp) walk: same bits.
//
// A device form cannot return BM_EINVAL for what only the device holds: a mask with a bit at or above n_in makes every
// entry of the output NaN instead (the host forms refuse it).
#include "bm_common.h"
#include "mixdist_core.h"

namespace bm {

constexpr int kMixBlock = 1024;             // at most 4 entries of Q and 4 of the output per lane, 64 additions each
constexpr int kMixLd = BM_MAX_ROWS + 1;     // odd row length, as in nnm.hip

static inline size_t mixdist_lds_bytes(int n_in) { return (size_t)2 * n_in * kMixLd * sizeof(double); }  // D, then Q

__global__ __launch_bounds__(kMixBlock) void mixed_sqdist_kernel(const double* __restrict__ sq, int n_in,
                                                                 const uint64_t* __restrict__ masks, int n_out,
                                                                 double* __restrict__ out) {
  extern __shared__ double mix_lds[];
  __shared__ uint64_t M[BM_MAX_ROWS];
  __shared__ double diag[BM_MAX_ROWS];
  __shared__ int bad;
  double* D = mix_lds;
  double* Q = mix_lds + n_in * kMixLd;
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  __syncthreads();
  if (tid < n_out) {
    const uint64_t m = masks[tid];
    M[tid] = m;
    if (!mixdist_mask_ok(m, n_in)) bad = 1;
  }
  for (int p = tid; p < n_in * n_in; p += kMixBlock) {
    const int i = p / n_in, j = p - i * n_in;
    D[i * kMixLd + j] = sq[p];
  }
  __syncthreads();
  if (bad) {
    for (int p = tid; p < n_out * n_out; p += kMixBlock) out[p] = __builtin_nan("");
    return;
  }
  // Q_ib: the lanes of a wave share i and walk b, so a read of D is one address for the wave
  for (int p = tid; p < n_in * n_out; p += kMixBlock) {
    const int i = p / n_out, b = p - i * n_out;
    Q[i * kMixLd + b] = mixdist_q(D, kMixLd, n_in, i, M[b]);
  }
  __syncthreads();
  if (tid < n_out) diag[tid] = mixdist_p(Q, kMixLd, n_in, M[tid], tid);
  __syncthreads();
  for (int p = tid; p < n_out * n_out; p += kMixBlock) {
    const int a = p / n_out, b = p - a * n_out;
    if (a == b) {
      out[p] = M[a] == 0 ? __builtin_nan("") : 0.0;
    } else if (a < b) {
      const int x = mixdist_first(M[a], M[b]) ? a : b, y = a + b - x;
      const double v = mixdist_entry(mixdist_p(Q, kMixLd, n_in, M[x], y), diag[x], diag[y], M[x], M[y]);
      out[p] = v;
      out[b * n_out + a] = v;
    }
  }
}

__global__ __launch_bounds__(BM_MAX_ROWS) void mix_weights_kernel(const uint64_t* __restrict__ masks, int n_in, int n_out,
                                                                  const double* __restrict__ w_mixed,
                                                                  const int32_t* __restrict__ sel, int m,
                                                                  double* __restrict__ w_out) {
  __shared__ uint64_t M[BM_MAX_ROWS];
  __shared__ double W[BM_MAX_ROWS];
  __shared__ int32_t S[BM_MAX_ROWS];
  const int tid = threadIdx.x;  // one lane per mixed row, then one per original row
  M[tid] = tid < n_out ? masks[tid] : 0;
  S[tid] = (sel != nullptr && tid < m) ? sel[tid] : 0;
  __syncthreads();
  bool ok = true;
  for (int r = 0; r < n_out; ++r) ok = ok && mixdist_mask_ok(M[r], n_in);
  if (sel != nullptr) {
    ok = ok && mixw_sel_ok(S, m, n_out);
    W[tid] = (tid < n_out && ok) ? mixw_from_sel(S, m, tid) : 0.0;
  } else {
    W[tid] = tid < n_out ? w_mixed[tid] : 0.0;
  }
  __syncthreads();
  ok = ok && mixw_rows_ok(W, M, n_out);
  w_out[tid] = tid >= n_in ? 0.0 : ok ? mixw_entry(W, M, n_out, tid) : __builtin_nan("");
}

}  // namespace bm

extern "C" int bm_mixed_sqdist_device(const double* sq_dev, int n_in, const uint64_t* masks_dev, int n_out, double* out_dev,
                                      void* stream) {
  using namespace bm;
  if (sq_dev == nullptr || masks_dev == nullptr || out_dev == nullptr || !mixdist_args_ok(n_in, n_out)) return BM_EINVAL;
  const size_t lds = mixdist_lds_bytes(n_in);
  if (const int rc = lds_opt_in(reinterpret_cast<const void*>(mixed_sqdist_kernel), lds,
                                BM_MAX_ROWS * (sizeof(uint64_t) + sizeof(double)) + sizeof(int)))
    return rc;
  hipLaunchKernelGGL(mixed_sqdist_kernel, dim3(1), dim3(kMixBlock), lds, static_cast<hipStream_t>(stream), sq_dev, n_in,
                     masks_dev, n_out, out_dev);
  BM_LAUNCH_CHECK();
  return 0;
}

extern "C" int bm_mix_weights_device(const uint64_t* masks_dev, int n_in, int n_out, const double* w_mixed_dev,
                                     const int32_t* sel_dev, int m, double* w_out_dev, void* stream) {
  using namespace bm;
  if (masks_dev == nullptr || w_out_dev == nullptr || !mixw_args_ok(n_in, n_out, w_mixed_dev, sel_dev, m)) return BM_EINVAL;
  hipLaunchKernelGGL(mix_weights_kernel, dim3(1), dim3(BM_MAX_ROWS), 0, static_cast<hipStream_t>(stream), masks_dev, n_in,
                     n_out, w_mixed_dev, sel_dev, m, w_out_dev);
  BM_LAUNCH_CHECK();
  return 0;
}
