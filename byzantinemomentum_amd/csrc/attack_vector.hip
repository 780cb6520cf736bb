// attack_vector.hip — the Byzantine vector of the reference's `nan`, `bulyan` and `empire-strict` attacks from the honest
// average, in ONE streaming pass.
//
// Replaces (reference, PyTorch):
//   byz_grad = empty_like(...); byz_grad.copy_(tensor((math.nan,)))            attacks/nan.py:36-40
//   grad_att = zeros_like(avg); grad_att[target_idx] = 1  |  ones_like(avg)    attacks/identical.py:114-127   one pass
//   grad_att.mul_(factor); byz_grad = grad_avg.add_(grad_att)                  attacks/identical.py:82-84     two passes
//   byz_grad.mul_(-epsilon)                                                    attacks/empire.py:61-62
// The direction of the `bulyan` attack is 0 / 1 per coordinate, so it is never read: the kernel forms it from the
// coordinate's index and computes avg + factor * dir with dir in {0, 1} at EVERY coordinate (no copy where dir is 0: a
// -0.0 of avg comes out as the reference's).  Two streams (avg in, the vector out; a third only when the caller wants the
// direction vector stored as well), no workspace, no atomics, no synchronisation.
#include "bm_common.h"

namespace bm {

constexpr int kAvBlock = 256;
constexpr int kAvMaxBlocks = 2048;

constexpr int kAvNan = 0, kAvShiftOne = 1, kAvShiftAll = 2, kAvScale = 3;

// `target`: the targeted coordinate counted from the FIRST coordinate of this launch (the host rebases it by Span.first);
// anything outside [0, nvec * VEC) is no coordinate of this launch.  Lane c of column v holds coordinate v * VEC + c.
template <int VEC, int KIND>
__global__ __launch_bounds__(kAvBlock) void attack_vector_kernel(const float* __restrict__ avg, int64_t nvec,
                                                                 int64_t target, float factor_host,
                                                                 const double* __restrict__ factor_dev,
                                                                 float* __restrict__ out, float* __restrict__ dir_out) {
  // the factor from device memory, rounded to fp32 as bm_multi_fma3_bdev rounds it (the host's double -> float conversion)
  const float factor = factor_dev != nullptr ? (float)factor_dev[0] : factor_host;
  const int64_t stride = (int64_t)gridDim.x * kAvBlock;
  for (int64_t v = (int64_t)blockIdx.x * kAvBlock + threadIdx.x; v < nvec; v += stride) {
    float x[VEC], dir[VEC];
    if constexpr (KIND != kAvNan) load_stream<VEC>(avg + v * VEC, x);
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      if constexpr (KIND == kAvNan) {
        x[c] = __builtin_bit_cast(float, 0x7FC00000u);
      } else if constexpr (KIND == kAvScale) {
        x[c] = x[c] * factor;
      } else {
        dir[c] = (KIND == kAvShiftAll || v * VEC + c == target) ? 1.0f : 0.0f;
        x[c] = x[c] + factor * dir[c];
      }
    }
    store_stream<VEC>(out + v * VEC, x);
    if constexpr (KIND == kAvShiftOne || KIND == kAvShiftAll) {
      if (dir_out != nullptr) store_stream<VEC>(dir_out + v * VEC, dir);
    }
  }
}

static inline bool av_overlap(const float* a, const float* b, int64_t d) {
  if (a == nullptr || b == nullptr || d == 0) return a != nullptr && a == b;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  const uintptr_t bytes = (uintptr_t)d * sizeof(float);
  return x < y ? y - x < bytes : x - y < bytes;
}

template <int VEC>
static void av_launch(int kind, const Span& sp, hipStream_t s, const float* avg, int64_t target, float factor,
                      const double* factor_dev, float* out, float* dir_out) {
  const float* a = advanced(avg, sp.first);
  float* o = out + sp.first;
  float* dr = advanced(dir_out, sp.first);
  const int64_t t = target >= 0 ? target - sp.first : -1;  // (a target before this launch's first coordinate: negative)
  const dim3 grid(sp.grid), block(kAvBlock);
  switch (kind) {
    case kAvNan:
      hipLaunchKernelGGL((attack_vector_kernel<VEC, kAvNan>), grid, block, 0, s, a, sp.count, t, factor, factor_dev, o, dr);
      break;
    case kAvShiftOne:
      hipLaunchKernelGGL((attack_vector_kernel<VEC, kAvShiftOne>), grid, block, 0, s, a, sp.count, t, factor, factor_dev, o, dr);
      break;
    case kAvShiftAll:
      hipLaunchKernelGGL((attack_vector_kernel<VEC, kAvShiftAll>), grid, block, 0, s, a, sp.count, t, factor, factor_dev, o, dr);
      break;
    default:
      hipLaunchKernelGGL((attack_vector_kernel<VEC, kAvScale>), grid, block, 0, s, a, sp.count, t, factor, factor_dev, o, dr);
      break;
  }
}

}  // namespace bm

extern "C" int bm_attack_vector(int kind, const float* avg, int64_t d, int64_t target, float factor,
                                const double* factor_dev, float* out, float* direction_out, void* stream) {
  using namespace bm;
  if (kind < kAvNan || kind > kAvScale || d < 0 || out == nullptr || (kind != kAvNan && avg == nullptr)) return BM_EINVAL;
  if (target < -1 || target >= d) return BM_EINVAL;
  if (direction_out != nullptr && (kind == kAvNan || kind == kAvScale)) return BM_EINVAL;
  if (av_overlap(out, avg, d) || av_overlap(out, direction_out, d) || av_overlap(direction_out, avg, d)) return BM_EINVAL;
  if (d == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int vec = Alignment().of(avg).of(out).of(direction_out).vec();
  return for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, kAvBlock, caps_of(kAvMaxBlocks), [&](auto width, const Span& sp) {
    av_launch<decltype(width)::value>(kind, sp, s, avg, target, factor, factor_dev, out, direction_out);
    BM_LAUNCH_CHECK();
    return 0;
  });
}
