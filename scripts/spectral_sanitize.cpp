// spectral_sanitize.cpp — a stand-alone CPU program (its own main) that drives the HOST form of the spectral filters,
// bm_spectral_weights (csrc/spectral.cpp over csrc/spectral_core.h), under AddressSanitizer and UBSan.  Host code only:
// no kernel is launched and no HIP call is made.  From the repository root:
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined scripts/spectral_sanitize.cpp byzantinemomentum_amd/csrc/spectral.cpp \
//         byzantinemomentum_amd/csrc/api.cpp -o /tmp/spectral_sanitize && /tmp/spectral_sanitize
//
// Every matrix lives in a heap buffer of exactly n * n doubles, the outputs in buffers of exactly 64 and 4, so that a
// read or write one element outside is reported.  Prints the number of calls and "no report" at the end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/bm_gar.h"

namespace {

unsigned long long state = 88172645463325252ull;
double uniform() {  // xorshift64: the same matrices on every run
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return (double)(state >> 11) / 9007199254740992.0;
}

// squared distances of n random points in `dim` dimensions, the last `copies` being one far point
std::vector<double> distances(int n, int dim, int copies) {
  std::vector<double> x((size_t)n * dim);
  for (auto& v : x) v = uniform() - 0.5;
  for (int i = n - copies; i < n; ++i)
    for (int c = 0; c < dim; ++c) x[(size_t)i * dim + c] = x[(size_t)(n - 1) * dim + c] + (i == n - 1 ? 20.0 : 0.0);
  for (int i = n - copies; i < n - 1; ++i)
    for (int c = 0; c < dim; ++c) x[(size_t)i * dim + c] = x[(size_t)(n - 1) * dim + c];
  std::vector<double> sq((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int c = 0; c < dim; ++c) {
        const double e = x[(size_t)i * dim + c] - x[(size_t)j * dim + c];
        s += e * e;
      }
      sq[(size_t)i * n + j] = s;
    }
  return sq;
}

long calls = 0;

int call(const std::vector<double>& sq, int n, int mode, int count, int iters) {
  double* m = (double*)malloc(sizeof(double) * (size_t)n * n);  // exactly n * n
  for (size_t p = 0; p < (size_t)n * n; ++p) m[p] = sq[p];
  double* w = (double*)malloc(sizeof(double) * 64);
  double* info = (double*)malloc(sizeof(double) * 4);
  const int code = bm_spectral_weights(m, n, mode, count, iters, w, info);
  ++calls;
  int bad = 0;
  if (code == 0) {
    double total = 0.0;
    bool nan = false;
    for (int i = 0; i < 64; ++i) {
      if (i >= n && w[i] != 0.0) bad = 1;
      if (std::isnan(w[i])) nan = true;
      total += w[i];
    }
    if (!nan && std::fabs(total - 1.0) > 1e-12) bad = 1;  // (an infinite distance between usable rows may give NaN)
  }
  free(m);
  free(w);
  free(info);
  if (bad) {
    std::printf("wrong weights: n = %d mode = %d count = %d iters = %d\n", n, mode, count, iters);
    std::exit(1);
  }
  return code;
}

}  // namespace

int main() {
  const int iters[] = {1, 16, 256};
  for (int n = 1; n <= 64; ++n) {
    for (int copies : {0, 1, 3}) {
      if (copies >= n) continue;
      std::vector<double> sq = distances(n, 9, copies);
      for (int T : iters) {
        for (int f : {0, 1, (n - 1) / 2}) {
          if (2 * f < n) call(sq, n, BM_SPECTRAL_CAF, f, T);
          if (f < n) call(sq, n, BM_SPECTRAL_DNC, f, T);
        }
        call(sq, n, BM_SPECTRAL_DNC, n - 1, T);
      }
      // NaN rows: a minority, a majority, all; an infinite and a negative entry
      for (int bad : {1, n / 3, n / 2 + 1, n}) {
        if (bad > n || bad < 1) continue;
        std::vector<double> nan = sq;
        for (int i = n - bad; i < n; ++i)
          for (int j = 0; j < n; ++j) nan[(size_t)i * n + j] = nan[(size_t)j * n + i] = NAN;
        call(nan, n, BM_SPECTRAL_CAF, (n - 1) / 2, 16);
        call(nan, n, BM_SPECTRAL_DNC, n - 1, 16);
      }
      if (n >= 3) {
        std::vector<double> odd = sq;
        odd[1] = odd[(size_t)n] = INFINITY;
        odd[2] = odd[(size_t)2 * n] = -1.0;
        call(odd, n, BM_SPECTRAL_CAF, (n - 1) / 2, 16);
        call(odd, n, BM_SPECTRAL_DNC, 1, 16);
      }
    }
    std::vector<double> zero((size_t)n * n, 0.0);  // all rows equal: degenerate
    call(zero, n, BM_SPECTRAL_CAF, (n - 1) / 2, 16);
    call(zero, n, BM_SPECTRAL_DNC, n - 1, 16);
  }
  // refused arguments: nothing is read or written
  std::vector<double> sq = distances(11, 9, 2);
  double out[64], info[4];
  int refused = 0;
  refused += bm_spectral_weights(sq.data(), 11, BM_SPECTRAL_CAF, 6, 16, out, info) == BM_EINVAL;
  refused += bm_spectral_weights(sq.data(), 11, BM_SPECTRAL_DNC, 11, 16, out, info) == BM_EINVAL;
  refused += bm_spectral_weights(sq.data(), 11, BM_SPECTRAL_CAF, -1, 16, out, info) == BM_EINVAL;
  refused += bm_spectral_weights(sq.data(), 11, BM_SPECTRAL_CAF, 2, 0, out, info) == BM_EINVAL;
  refused += bm_spectral_weights(sq.data(), 11, BM_SPECTRAL_CAF, 2, 257, out, info) == BM_EINVAL;
  refused += bm_spectral_weights(sq.data(), 11, 2, 2, 16, out, info) == BM_EINVAL;
  refused += bm_spectral_weights(sq.data(), 0, BM_SPECTRAL_CAF, 0, 16, out, info) == BM_EINVAL;
  refused += bm_spectral_weights(sq.data(), 65, BM_SPECTRAL_CAF, 2, 16, out, info) == BM_EINVAL;
  refused += bm_spectral_weights(nullptr, 11, BM_SPECTRAL_CAF, 2, 16, out, info) == BM_EINVAL;
  refused += bm_spectral_weights(sq.data(), 11, BM_SPECTRAL_CAF, 2, 16, nullptr, info) == BM_EINVAL;
  refused += bm_spectral_weights(sq.data(), 11, BM_SPECTRAL_CAF, 2, 16, out, nullptr) == BM_EINVAL;
  if (refused != 11) {
    std::printf("a bad argument was accepted (%d of 11 refused)\n", refused);
    return 1;
  }
  std::printf("%ld calls, 11 refusals: no report\n", calls);
  return 0;
}
