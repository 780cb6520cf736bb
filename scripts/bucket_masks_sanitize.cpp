// bucket_masks_sanitize.cpp — a stand-alone CPU program (its own main) that drives the HOST form of the bucket masks,
// bm_bucket_masks (csrc/bucket_masks.cpp over csrc/bucket_core.h), under AddressSanitizer and UBSan.  Host code only: no
// kernel is launched and no HIP call is made.  From the repository root:
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Iinclude scripts/bucket_masks_sanitize.cpp \
//         byzantinemomentum_amd/csrc/bucket_masks.cpp -o /tmp/bucket_masks_sanitize && /tmp/bucket_masks_sanitize
//
// The masks live in a heap buffer of exactly BM_MAX_ROWS words, so that a write one word outside is reported.  Covers
// n = 1 .. 64 with every s = 1 .. n, seeds and counters at the ends of the 64-bit range, and every refused argument;
// checks that every result is a partition of 0 .. n-1 into buckets of s, s, ..., n mod s and pins the anchors of the
// contract.  Prints the number of calls and "no report" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/bm_gar.h"

namespace {

int calls = 0;

void fail(const char* what, int n, int s) {
  std::printf("FAILED: %s at n = %d, s = %d\n", what, n, s);
  std::exit(1);
}

void check(int n, int s, uint64_t seed, uint64_t counter) {
  std::vector<uint64_t> masks(BM_MAX_ROWS, ~(uint64_t)0);
  if (bm_bucket_masks(n, s, seed, counter, masks.data()) != 0) fail("refused", n, s);
  ++calls;
  const int n_out = (n + s - 1) / s;
  uint64_t all = 0;
  for (int b = 0; b < BM_MAX_ROWS; ++b) {
    const int want = b < n_out ? (b * s + s <= n ? s : n - b * s) : 0;
    if (__builtin_popcountll(masks[b]) != want) fail("bucket size", n, s);
    if (all & masks[b]) fail("overlap", n, s);
    all |= masks[b];
  }
  if (all != (n == 64 ? ~(uint64_t)0 : (((uint64_t)1 << n) - 1))) fail("not a partition", n, s);
}

}  // namespace

int main() {
  const uint64_t ends[] = {0, 1, 0x9E3779B97F4A7C15ull, (uint64_t)1 << 63, ~(uint64_t)0};
  for (int n = 1; n <= BM_MAX_ROWS; ++n)
    for (int s = 1; s <= n; ++s)
      for (uint64_t seed : ends)
        for (uint64_t counter : ends) check(n, s, seed, counter);
  std::vector<uint64_t> masks(BM_MAX_ROWS);
  const uint64_t anchor[6] = {0x60, 0x9, 0x410, 0x6, 0x300, 0x80};
  if (bm_bucket_masks(11, 2, 0, 0, masks.data()) != 0) fail("anchor refused", 11, 2);
  for (int b = 0; b < 6; ++b)
    if (masks[b] != anchor[b]) fail("anchor", 11, 2);
  const int bad[][2] = {{0, 1}, {65, 1}, {-1, 1}, {11, 0}, {11, 12}, {11, -1}};
  for (const auto& a : bad)
    if (bm_bucket_masks(a[0], a[1], 0, 0, masks.data()) != BM_EINVAL) fail("not refused", a[0], a[1]);
  if (bm_bucket_masks(11, 2, 0, 0, nullptr) != BM_EINVAL) fail("null not refused", 11, 2);
  std::printf("%d calls, no report\n", calls);
  return 0;
}
