// minmax_sanitize.cpp — a stand-alone CPU program (its own main) that drives the HOST form of the Min-Max / Min-Sum
// factor, bm_minmax_factor (csrc/minmax.cpp over csrc/minmax_core.h), under AddressSanitizer and UBSan.  Host code
// only: no kernel is launched and no HIP call is made.  From the repository root:
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined scripts/minmax_sanitize.cpp byzantinemomentum_amd/csrc/minmax.cpp \
//         -o /tmp/minmax_sanitize && /tmp/minmax_sanitize
//
// Every matrix lives in a heap buffer of exactly h * h doubles, the scalars in one of exactly BM_PERTURB_SLOTS, the
// output in one of exactly 6, so that a read or write one element outside is reported.  Covers h = 2 .. 64, both modes,
// three directions, the degenerate inputs and every refused argument; checks tightness of every factor on the
// vectors.  Prints the number of calls and "no report" at the end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/bm_gar.h"

namespace {

unsigned long long state = 88172645463325252ull;
double uniform() {  // xorshift64: the same stacks on every run
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return (double)(state >> 11) / 9007199254740992.0;
}

int calls = 0;

void fail(const char* what, int h, int mode) {
  std::printf("FAILED: %s (h = %d, mode = %d)\n", what, h, mode);
  std::exit(1);
}

struct Stack {
  int h, dim;
  std::vector<double> x, avg, p;
  double* sq;    // exactly h * h
  double* scal;  // exactly BM_PERTURB_SLOTS
  Stack(int h_, int dim_, int kind) : h(h_), dim(dim_), x((size_t)h_ * dim_), avg(dim_), p(dim_) {
    for (auto& v : x) v = uniform() - 0.3;
    for (int c = 0; c < dim; ++c) {
      double s = 0.0, q = 0.0;
      for (int i = 0; i < h; ++i) s += x[(size_t)i * dim + c];
      avg[c] = s / h;
      for (int i = 0; i < h; ++i) q += (x[(size_t)i * dim + c] - avg[c]) * (x[(size_t)i * dim + c] - avg[c]);
      p[c] = kind == BM_PERTURB_UNIT ? -avg[c] : (kind == BM_PERTURB_STD ? -std::sqrt(q / (h - 1)) : (avg[c] > 0 ? -1.0 : (avg[c] < 0 ? 1.0 : 0.0)));
    }
    sq = new double[(size_t)h * h];
    scal = new double[BM_PERTURB_SLOTS]();
    for (int i = 0; i < h; ++i)
      for (int j = 0; j < h; ++j) {
        double s = 0.0;
        for (int c = 0; c < dim; ++c) {
          const double df = x[(size_t)i * dim + c] - x[(size_t)j * dim + c];
          s += df * df;
        }
        sq[i * h + j] = s;
      }
    for (int i = 0; i < h; ++i) {
      double b = 0.0;
      for (int c = 0; c < dim; ++c) b += p[c] * (avg[c] - x[(size_t)i * dim + c]);
      scal[i] = b;
    }
    for (int c = 0; c < dim; ++c) {
      scal[BM_MAX_ROWS] += p[c] * p[c];
      scal[BM_MAX_ROWS + 1] += avg[c] * avg[c];
    }
  }
  ~Stack() {
    delete[] sq;
    delete[] scal;
  }
  // the constraint of the attack at the factor g: (value, bound)
  void constraint(double g, int mode, double* value, double* bound) const {
    double vmax = 0.0, vsum = 0.0, R = 0.0, S = 0.0;
    for (int i = 0; i < h; ++i) {
      double d2 = 0.0, row = 0.0;
      for (int c = 0; c < dim; ++c) {
        const double df = avg[c] + g * p[c] - x[(size_t)i * dim + c];
        d2 += df * df;
      }
      vmax = d2 > vmax ? d2 : vmax;
      vsum += d2;
      for (int j = 0; j < h; ++j) {
        row += sq[i * h + j];
        R = sq[i * h + j] > R ? sq[i * h + j] : R;
      }
      S = row > S ? row : S;
    }
    *value = mode == BM_MINMAX ? vmax : vsum;
    *bound = mode == BM_MINMAX ? R : S;
  }
};

void expect_degenerate(const double* sq, const double* scal, int h, int mode, const char* what) {
  double* out = new double[6];
  ++calls;
  if (bm_minmax_factor(sq, scal, h, mode, out) != 0) fail("a degenerate input was refused", h, mode);
  if (out[5] != 1.0 || out[0] != 0.0 || std::signbit(out[0]) || out[2] != -1.0) fail(what, h, mode);
  delete[] out;
}

}  // namespace

int main() {
  for (int h = 2; h <= BM_MAX_ROWS; ++h)
    for (int kind = 0; kind < 3; ++kind) {
      Stack st(h, 5 + (h % 7), kind);
      for (int mode = 0; mode < 2; ++mode) {
        double* out = new double[6];
        ++calls;
        if (bm_minmax_factor(st.sq, st.scal, h, mode, out) != 0) fail("refused", h, mode);
        if (out[5] != 0.0 || !(out[0] > 0.0)) fail("a plain stack came out degenerate", h, mode);
        if (mode == BM_MINMAX ? !(out[2] >= 0.0 && out[2] < h) : out[2] != -1.0) fail("binding row", h, mode);
        double value, bound, beyond;
        st.constraint(out[0], mode, &value, &bound);
        if (!(value <= bound * (1 + 1e-9))) fail("the factor breaks the constraint", h, mode);
        st.constraint(out[0] * (1 + 1e-6), mode, &beyond, &bound);
        if (!(beyond > bound)) fail("the factor is not the largest", h, mode);
        if (std::fabs(out[1] - bound) > 1e-12 * bound) fail("bound", h, mode);
        delete[] out;
        // the degenerate inputs, each on a fresh copy of exactly the same sizes
        double* sq = new double[(size_t)h * h];
        double* scal = new double[BM_PERTURB_SLOTS];
        auto reset = [&]() {
          for (int i = 0; i < h * h; ++i) sq[i] = st.sq[i];
          for (int i = 0; i < BM_PERTURB_SLOTS; ++i) scal[i] = st.scal[i];
        };
        reset();
        scal[BM_MAX_ROWS] = 0.0;
        expect_degenerate(sq, scal, h, mode, "P = 0");
        scal[BM_MAX_ROWS] = -1.0;
        expect_degenerate(sq, scal, h, mode, "P < 0");
        scal[BM_MAX_ROWS] = INFINITY;
        expect_degenerate(sq, scal, h, mode, "P infinite");
        reset();
        scal[h - 1] = NAN;
        expect_degenerate(sq, scal, h, mode, "a NaN scalar");
        reset();
        sq[1] = sq[h] = INFINITY;
        expect_degenerate(sq, scal, h, mode, "an infinite distance");
        reset();
        for (int j = 0; j < h; ++j) sq[(h - 1) * h + j] = sq[j * h + h - 1] = NAN;
        expect_degenerate(sq, scal, h, mode, "a NaN row");
        reset();
        for (int i = 0; i < h * h; ++i) sq[i] = 0.0;  // all rows equal: b_i = 0 then
        for (int i = 0; i < h; ++i) scal[i] = 0.0;
        double* out0 = new double[6];
        ++calls;
        if (bm_minmax_factor(sq, scal, h, mode, out0) != 0 || out0[0] != 0.0 || out0[5] != 0.0) fail("equal rows", h, mode);
        delete[] out0;
        delete[] sq;
        delete[] scal;
      }
    }
  // every refused argument
  double* sq = new double[4]();
  double* scal = new double[BM_PERTURB_SLOTS]();
  double* out = new double[6]();
  const int refused[] = {
      bm_minmax_factor(nullptr, scal, 2, BM_MINMAX, out), bm_minmax_factor(sq, nullptr, 2, BM_MINMAX, out),
      bm_minmax_factor(sq, scal, 2, BM_MINMAX, nullptr),  bm_minmax_factor(sq, scal, 1, BM_MINMAX, out),
      bm_minmax_factor(sq, scal, 0, BM_MINSUM, out),      bm_minmax_factor(sq, scal, -3, BM_MINSUM, out),
      bm_minmax_factor(sq, scal, BM_MAX_ROWS + 1, BM_MINMAX, out), bm_minmax_factor(sq, scal, 2, 2, out),
      bm_minmax_factor(sq, scal, 2, -1, out)};
  for (int rc : refused) {
    ++calls;
    if (rc != BM_EINVAL) fail("a bad argument was accepted", 0, 0);
  }
  delete[] sq;
  delete[] scal;
  delete[] out;
  std::printf("%d calls of bm_minmax_factor, no report\n", calls);
  return 0;
}
