// bucket_masks.cpp — bm_bucket_masks: the bucket masks of bucketing from (n, s, seed, counter) ON THE HOST (pure host
// code: no kernel, no HIP call).  The definition is bucket_core.h's, the one the device form (bucket_masks.hip) runs: the
// two are compared bit for bit.
#include <cstdint>

#include "bucket_core.h"

extern "C" int bm_bucket_masks(int n, int s, uint64_t seed, uint64_t counter, uint64_t* masks_host) {
  using namespace bm;
  if (masks_host == nullptr || !bucket_args_ok(n, s)) return BM_EINVAL;
  uint8_t perm[BM_MAX_ROWS];
  bucket_permutation(n, seed, counter, perm);
  for (int b = 0; b < BM_MAX_ROWS; ++b) masks_host[b] = bucket_mask(perm, n, s, b);
  return 0;
}
