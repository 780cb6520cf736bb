// bucket_core.h — the bucket masks of bucketing (Karimireddy, He, Jaggi, ICLR 2022) from a counter, shared by the host
// form (bucket_masks.cpp, bm_bucket_masks) and the device form (bucket_masks.hip, bm_bucket_masks_device).
//
// The permutation is a function of (n, seed, counter) alone, uint64 and wrapping throughout (include/bm_gar.h):
//     mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
//     u_i    = mix(seed + 0x9E3779B97F4A7C15 * (64 * counter + i))                       i = 1 .. n-1
//     perm   = (0 .. n-1);  for i = n-1 down to 1:  j = u_i mod (i + 1);  swap(perm[i], perm[j])
//     bucket b = { perm[b s] .. perm[min(n, b s + s) - 1] },  b < ceil(n / s)
// ONE definition for both sides — integers only, so the two forms cannot differ; gars.bucket_permutation is the same
// in Python integers.  No state: every rank of a sharded run, and every replay of a recorded graph (whose counter
// lives in device memory), draws its permutation without a collective and without the host.
#pragma once
#include "bm_common.h"

namespace bm {

__host__ __device__ inline uint64_t bucket_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// u_i of the definition
__host__ __device__ inline uint64_t bucket_draw(uint64_t seed, uint64_t counter, int i) {
  return bucket_mix(seed + 0x9E3779B97F4A7C15ull * (64ull * counter + (uint64_t)i));
}

// perm: n bytes (the caller's: a stack array on the host, LDS on the device)
__host__ __device__ inline void bucket_permutation(int n, uint64_t seed, uint64_t counter, uint8_t* perm) {
  for (int i = 0; i < n; ++i) perm[i] = (uint8_t)i;
  for (int i = n - 1; i >= 1; --i) {
    const int j = (int)(bucket_draw(seed, counter, i) % (uint64_t)(i + 1));
    const uint8_t t = perm[i];
    perm[i] = perm[j];
    perm[j] = t;
  }
}

// masks[b] of the definition; 0 for b >= ceil(n / s)
__host__ __device__ inline uint64_t bucket_mask(const uint8_t* perm, int n, int s, int b) {
  uint64_t m = 0;
  const int64_t lo = (int64_t)b * s;
  for (int64_t p = lo; p < lo + s && p < n; ++p) m |= (uint64_t)1 << perm[p];
  return m;
}

// Arguments both entry points refuse before doing anything.
inline bool bucket_args_ok(int n, int s) { return n >= 1 && n <= BM_MAX_ROWS && s >= 1 && s <= n; }

}  // namespace bm
