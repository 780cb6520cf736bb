// spectral.hip — bm_spectral_weights_device: the weights of CAF / DnC from the n x n squared distances where
// bm_pairwise_sqdist left them, in ONE workgroup, so that
//     distances -> weights -> bm_weighted_sum
// are launches on one stream with no copy and no synchronisation between them (a HIP graph records them).  The
// evaluation is spectral_core.h's, the one the host form (spectral.cpp) runs: same weights, bit for bit
// (tests/test_gpu_spectral.py).
//
// A call runs (power_iters + 2) x rounds row-dot sweeps, 70-300 at the defaults, so the sweep is what counts.  LANES
// waves share it: lane i of every wave is row i, wave l adds chain l of the row (the terms j = l, l + LANES, ...), the
// chains meet in LDS and every wave adds them in index order.  Everything else — the sums over the rows, the
// reweighting — every wave computes for itself on its own copy of the state: the same bits in every wave, so the waves
// take the same branches and meet at the same barriers, and the only traffic between waves is the chains.
#include "bm_common.h"
#include "spectral_core.h"

namespace bm {

constexpr int kSpectralLd = BM_MAX_ROWS + 1;  // odd row length: lane i walking row i meets no bank conflict

template <int LANES>
struct WavesPar {
  int lane, wave;
  double* part;  // [2][LANES][BM_MAX_ROWS]: the chains of a sweep; sweeps alternate between the two halves
  int half;
  __device__ int begin() const { return lane; }
  __device__ int end() const { return lane + 1; }
  __device__ bool writes() const { return wave == 0; }
  __device__ void sync() const { __syncthreads(); }
  __device__ double sum(const double (&slots)[BM_MAX_ROWS]) const {
    double v = slots[lane];
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = v + __shfl_xor(v, s, 64);
    return v;
  }
  __device__ void sum2(const double (&a)[BM_MAX_ROWS], const double (&b)[BM_MAX_ROWS], double& sa, double& sb) const {
    double va = a[lane], vb = b[lane];
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      va = va + __shfl_xor(va, s, 64);
      vb = vb + __shfl_xor(vb, s, 64);
    }
    sa = va;
    sb = vb;
  }
  __device__ double max(const double (&slots)[BM_MAX_ROWS]) const {
    double v = slots[lane];
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const double o = __shfl_xor(v, s, 64);
      v = o > v ? o : v;
    }
    return v;
  }
  // (the callers have passed a barrier since `w` was written)
  __device__ void dots(const double* w, const double* D, int ld, int N, double* out) {
    const double p = lane < N ? spectral_partial_dot<LANES>(w, D + lane * ld, N, wave) : 0.0;
    if (LANES == 1) {
      out[lane] = p;
      return;
    }
    // A wave that is one sweep ahead writes the other half; it cannot be two ahead: this barrier stands in between.
    double* mine = part + half * LANES * BM_MAX_ROWS;
    mine[wave * BM_MAX_ROWS + lane] = p;
    __syncthreads();
    double s = mine[lane];
#pragma unroll
    for (int l = 1; l < LANES; ++l) s = s + mine[l * BM_MAX_ROWS + lane];
    out[lane] = s;
    half ^= 1;
  }
};

template <int LANES>
__global__ __launch_bounds__(64 * LANES) void spectral_weights_kernel(const double* __restrict__ sq, int n, int mode,
                                                                      int count, int power_iters,
                                                                      double* __restrict__ weights_out,
                                                                      double* __restrict__ info_out) {
  __shared__ double D[BM_MAX_ROWS * kSpectralLd];
  __shared__ SpectralState st[LANES];
  __shared__ double part[2 * LANES * BM_MAX_ROWS];
  for (int p = threadIdx.x; p < n * n; p += 64 * LANES) {
    const int i = p / n, j = p - i * n;
    D[i * kSpectralLd + j] = sq[p];
  }
  __syncthreads();
  WavesPar<LANES> par{(int)(threadIdx.x & 63), (int)(threadIdx.x >> 6), part, 0};
  spectral_run(D, kSpectralLd, n, mode, count, power_iters, st[par.wave], info_out, par);
  if (par.wave == 0) weights_out[par.lane] = st[0].best[par.lane];
}

}  // namespace bm

extern "C" int bm_spectral_weights_device(const double* sq_dev, int n, int mode, int count, int power_iters,
                                          double* weights_out_dev, double* info_out_dev, void* stream) {
  using namespace bm;
  if (sq_dev == nullptr || weights_out_dev == nullptr || info_out_dev == nullptr ||
      !spectral_args_ok(n, mode, count, power_iters))
    return BM_EINVAL;
  if (tuning().spectral_lanes == 1)
    hipLaunchKernelGGL(spectral_weights_kernel<1>, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), sq_dev, n,
                       mode, count, power_iters, weights_out_dev, info_out_dev);
  else
    hipLaunchKernelGGL(spectral_weights_kernel<kSpectralLanes>, dim3(1), dim3(64 * kSpectralLanes), 0,
                       static_cast<hipStream_t>(stream), sq_dev, n, mode, count, power_iters, weights_out_dev,
                       info_out_dev);
  BM_LAUNCH_CHECK();
  return 0;
}
