// center.hip — bm_center_weights_device: the weights of the geometric median / centered clipping from the N x N
// squared distances where bm_pairwise_sqdist left them, in ONE workgroup (one wave: lane i is point i), so that
//     distances -> weights -> bm_weighted_sum
// are launches on one stream with no copy and no synchronisation between them (a HIP graph records them).  The
// iteration is center_core.h's, the one the host form (center.cpp) runs: same weights, bit for bit
// (tests/test_gpu_center_weights.py).
#include "bm_common.h"
#include "center_core.h"

namespace bm {

constexpr int kCenterBlock = 64;
constexpr int kCenterLd = BM_MAX_ROWS + 1;  // odd row length: lane i walking row i meets no bank conflict

// Lane i handles point i; the phases meet at a workgroup barrier (one wave: it orders the LDS traffic and costs
// nothing else); a sum over the points is the butterfly of search_core.h over the lanes, every lane ending with the same bits.
struct WavePar {
  int lane;
  __device__ int begin() const { return lane; }
  __device__ int end() const { return lane + 1; }
  __device__ void sync() const { __syncthreads(); }
  __device__ double sum(const double (&slots)[BM_MAX_ROWS]) const {
    __syncthreads();
    double v = slots[lane];
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = v + __shfl_xor(v, s, 64);
    return v;
  }
};

__global__ __launch_bounds__(kCenterBlock) void center_weights_kernel(const double* __restrict__ sq, int n, int has_start,
                                                                      int mode, double param, int iters, double tol,
                                                                      double* __restrict__ weights_out,
                                                                      double* __restrict__ info_out) {
  __shared__ double D[BM_MAX_ROWS * kCenterLd];
  __shared__ CenterState st;
  const int N = n + (has_start ? 1 : 0), lane = threadIdx.x;
  for (int p = lane; p < N * N; p += kCenterBlock) {
    const int i = p / N, j = p - i * N;
    D[i * kCenterLd + j] = sq[p];
  }
  __syncthreads();
  WavePar par{lane};
  center_run(D, kCenterLd, n, has_start, mode, param, iters, tol, st, info_out, par);
  weights_out[lane] = st.c[lane];
}

}  // namespace bm

extern "C" int bm_center_weights_device(const double* sq_dev, int n, int has_start, int mode, double param, int iters,
                                        double tol, double* weights_out_dev, double* info_out_dev, void* stream) {
  using namespace bm;
  if (sq_dev == nullptr || weights_out_dev == nullptr || info_out_dev == nullptr ||
      !center_args_ok(n, has_start, mode, param, iters, tol))
    return BM_EINVAL;
  hipLaunchKernelGGL(center_weights_kernel, dim3(1), dim3(kCenterBlock), 0, static_cast<hipStream_t>(stream), sq_dev, n,
                     has_start ? 1 : 0, mode, param, iters, tol, weights_out_dev, info_out_dev);
  BM_LAUNCH_CHECK();
  return 0;
}
