// bucket_masks.hip — bm_bucket_masks_device: the bucket masks of bucketing drawn ON THE DEVICE from a counter that lives
// in device memory, in ONE wavefront, so that
//     masks -> bm_mix_rows / bm_colwise_bucketed
// are launches on one stream and a recorded graph draws the NEXT permutation at every replay with no host involvement.
// The definition is bucket_core.h's, the one the host form (bucket_masks.cpp) runs: same masks, bit for bit.
#include "bm_common.h"
#include "bucket_core.h"

namespace bm {

constexpr int kBucketBlock = 64;  // one wavefront: lane b answers for bucket b

__global__ __launch_bounds__(kBucketBlock) void bucket_masks_kernel(int n, int s, uint64_t seed,
                                                                    uint64_t* __restrict__ counter,
                                                                    uint64_t* __restrict__ masks) {
  __shared__ uint8_t perm[BM_MAX_ROWS];
  const int tid = threadIdx.x;
  const uint64_t c = counter[0];  // every lane reads it BEFORE the one store below (the barrier orders them)
  // the n - 1 swaps depend on one another: one lane walks them (at most 63)
  if (tid == 0) bucket_permutation(n, seed, c, perm);
  __syncthreads();
  masks[tid] = bucket_mask(perm, n, s, tid);  // BM_MAX_ROWS masks: zeros beyond ceil(n / s)
  // no atomic: launches on one stream are ordered, and one counter word belongs to one stream of launches
  if (tid == 0) counter[0] = c + 1;
}

}  // namespace bm

extern "C" int bm_bucket_masks_device(int n, int s, uint64_t seed, uint64_t* counter_dev, uint64_t* masks_dev,
                                      void* stream) {
  using namespace bm;
  if (counter_dev == nullptr || masks_dev == nullptr || !bucket_args_ok(n, s)) return BM_EINVAL;
  hipLaunchKernelGGL(bucket_masks_kernel, dim3(1), dim3(kBucketBlock), 0, static_cast<hipStream_t>(stream), n, s, seed,
                     counter_dev, masks_dev);
  BM_LAUNCH_CHECK();
  return 0;
}
