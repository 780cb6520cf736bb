// nnm_core.h — the neighbour masks of nearest-neighbour mixing (Allouah et al., "Fixing by Mixing", AISTATS 2023) from the
// n x n fp64 squared distances, shared by the host form (nnm.cpp, bm_nnm_masks) and the device form (nnm.hip,
// bm_nnm_masks_device).
//
// N_i = { i } + the k - 1 = n - f - 1 OTHER rows of smallest D[i][j]: row i itself whatever D[i][i] holds, ties to the
// lower index, NaN keys last and in index order among themselves (+inf before NaN) — the stable order of the selection
// kernels (rank_body.h).  Bit j of masks[i] is set iff j is in N_i.
//
// ONE definition for both sides: nnm_member() answers "is j in N_i" by counting the other rows that come before j in
// that order — comparisons and integers only, so the two forms cannot differ by a rounding; the host walks every
// (i, j), the device gives each lane a few j of one i.
#pragma once
#include "bm_common.h"

namespace bm {

// "key a of row ja comes before key b of row jb" in the stable ascending order with NaN last
__host__ __device__ inline bool nnm_before(double a, int ja, double b, int jb) {
  const bool an = a != a, bn = b != b;
  if (an || bn) return an == bn ? ja < jb : bn;
  return a < b || (a == b && ja < jb);
}

// drow: row i of D (n doubles).  k = n - f >= 1.
__host__ __device__ inline bool nnm_member(const double* drow, int n, int k, int i, int j) {
  if (j == i) return true;
  const double dj = drow[j];
  int before = 0;
  for (int t = 0; t < n; ++t) before += (t != i && t != j && nnm_before(drow[t], t, dj, j)) ? 1 : 0;
  return before < k - 1;
}

// Arguments both entry points refuse before doing anything.
inline bool nnm_args_ok(int n, int f) { return n >= 1 && n <= BM_MAX_ROWS && f >= 0 && f < n; }

}  // namespace bm
