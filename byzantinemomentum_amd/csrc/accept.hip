// accept.hip — the "Attack acceptation ratio" of the study row (attack.py:571,822) from the selection a rule left.
//
// Replaces (reference, PyTorch):
//   defense.influence(honests, attacks, f, **gar_args)            attack.py:822
//   which ranks the stack a second time (krum.py:142, brute.py:131, aksel.py:96, cge.py:85) and compares every
//   selected gradient with every attack by identity (krum.py:144-150): one more distance pass and a host loop.
// gradients = honests + [byz] * f_real, so "the selected row is an attack" is "its index is >= h".  The rule already
// left its selection in device memory (the ranking of bm_krum_rank / bm_stable_argsort, the subset of
// bm_brute_select_device); bm_accept_count counts, in ONE wavefront, the entries >= h among the first `count` and leaves
// the INTEGER as a double next to the step's other scalars.  The division by the rule's denominator is the host's
// `int / int`, the reference's own arithmetic: equal by construction, no tolerance.
#include "bm_common.h"

namespace bm {

// lane l looks at order[l]; the wave's ballot is the count (count <= BM_MAX_ROWS = 64 = one wavefront)
__global__ __launch_bounds__(64) void accept_count_kernel(const int32_t* __restrict__ order, int count, int h,
                                                          double* __restrict__ out) {
  static_assert(BM_MAX_ROWS == 64, "one lane per row of the selection");
  const int lane = threadIdx.x;
  const bool hit = lane < count && load_index_coherent(order + lane) >= h;
  const unsigned long long mask = __ballot(hit);
  if (lane == 0) out[0] = (double)__popcll(mask);
}

}  // namespace bm

extern "C" int bm_accept_count(const int32_t* order, int count, int h, double* out, void* stream) {
  using namespace bm;
  if (order == nullptr || out == nullptr || count < 0 || count > BM_MAX_ROWS || h < 0) return BM_EINVAL;
  // (count == 0: no lane reads, the ballot is empty and out[0] = 0)
  hipLaunchKernelGGL(accept_count_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), order, count, h, out);
  BM_LAUNCH_CHECK();
  return 0;
}
