// perturb.hip — bm_perturb_stats: what the closed form of the Min-Max / Min-Sum attacks (include/bm_gar.h,
// minmax_core.h) needs from the d-sized data, in ONE pass over the h honest rows with the column in registers, as
// stack_stats_kernel (reduce.hip) walks it: the average (its bits), the perturbation direction p, and the scalars
//   b_i = <p, avg - g_i>,   P = |p|^2,   N = |avg|^2.
// Traffic: h row reads, two row writes.  Next to the h x VEC values of a column a lane keeps h + 2 fp32 chains, so the
// row-count classes narrow the column sooner than bm_stack_stats does (40 rows at 8 bytes, 64 at 4).
//
// Accumulation: a chain is at most 16 iterations long (kPerturbFold, the interval of row_sqnorms_kernel), whatever d
// is: every 16th iteration — and once at the end — each wave adds its 64 chains of a scalar in fp64 by a fixed shuffle
// tree and its first lane adds the result to the wave's fp64 slot in LDS.  The loop's trip count is the workgroup's,
// not the lane's (lanes past the end sit out with zeros), so the tree is never entered in divergent flow.  The
// workgroup's four slots are added in wave order into the workspace, the finish kernel adds the workgroups' partials
// in launch order (lane l the partials l, l + 64, ..., then a fixed tree).  No float atomics, no synchronisation.
#include "bm_common.h"

namespace bm {

constexpr int kPerturbBlock = 256;
constexpr int kPerturbFold = 16;
constexpr int kPerturbStep = 8;  // rows between two row-count classes
constexpr int kPerturbMaxBlocks = 2048;
constexpr int kPerturbSlots = BM_PERTURB_SLOTS;

__device__ __forceinline__ float perturb_coordinate(float avg, float q, float fk, int kind) {
  if (kind == BM_PERTURB_STD) return byzantine_coordinate(avg, q, fk, -1.0f, BM_ATTACK_LITTLE | BM_ATTACK_DIRECTION);
  if (kind == BM_PERTURB_UNIT) return -avg;
  return avg > 0.0f ? -1.0f : (avg < 0.0f ? 1.0f : (avg == 0.0f ? 0.0f : avg));  // -sign(avg); a NaN stays NaN
}

// the wave's sum of one chain, in fp64, into the wave's slot (every lane of the wave must call)
__device__ __forceinline__ void perturb_fold(float& chain, double* slot) {
  double t = (double)chain;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  if ((threadIdx.x & 63) == 0) *slot += t;
  chain = 0.0f;
}

template <int KMAX, int VEC>
__global__ __launch_bounds__(kPerturbBlock) void perturb_stats_kernel(RowTable rows, int k, int64_t nvec,
                                                                      float* __restrict__ avg_out,
                                                                      float* __restrict__ dir_out, int kind,
                                                                      double* __restrict__ partial) {
  __shared__ double wide[kPerturbBlock / 64][kPerturbSlots];
  // Up to 24 rows the pointer table lives in scalar registers (two per row, 106 in all).  Beyond, it is read where the
  // launch left it, in the kernel-argument segment (the table is the first argument: offset 0), eight pointers at a
  // time and every iteration: the base is made opaque per group, so that the scalar loads can neither be hoisted out of
  // the loop nor gathered in front of it — 64 pointers at once would be spilled, 8 are not.
  constexpr bool kTableFromKernarg = KMAX > 24;
  typedef const float* RowPtr;
  typedef const __attribute__((address_space(4))) RowPtr* KernargTable;
  for (int s = threadIdx.x; s < (kPerturbBlock / 64) * kPerturbSlots; s += kPerturbBlock) (&wide[0][0])[s] = 0.0;
  __syncthreads();
  double* const mine = wide[threadIdx.x >> 6];
  // a class serves KMAX - 7 .. KMAX rows (dispatch_perturb): only its last kPerturbStep rows are there or not
  const auto has = [k](int i) { return i < KMAX - kPerturbStep || i < k; };
  const float fk = (float)k;
  float b[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) b[i] = 0.0f;
  float pp = 0.0f, nn = 0.0f;
  const int64_t stride = (int64_t)gridDim.x * kPerturbBlock;
  const int64_t base = (int64_t)blockIdx.x * kPerturbBlock;
  const int64_t iters = base < nvec ? (nvec - base + stride - 1) / stride : 0;  // the same on every lane of the workgroup
  int64_t v = base + threadIdx.x;
  for (int64_t it = 0; it < iters; ++it, v += stride) {
    if (v < nvec) {
      float x[KMAX][VEC];
      [[maybe_unused]] KernargTable karg = nullptr;
#pragma unroll
      for (int i = 0; i < KMAX; ++i)
        if (has(i)) {
          if constexpr (kTableFromKernarg) {
            if (i % kPerturbStep == 0) {
              karg = (KernargTable)__builtin_amdgcn_kernarg_segment_ptr();
              asm volatile("" : "+s"(karg));
            }
            load_stream<VEC>(karg[i] + v * VEC, x[i]);
          } else
            load_stream<VEC>(rows.p[i] + v * VEC, x[i]);
        }
      float avg[VEC], dir[VEC];
#pragma unroll
      for (int c = 0; c < VEC; ++c) {
        float s = x[0][c];  // the sequential mean and the deviation sum of stack_stats_kernel, operation for operation
#pragma unroll
        for (int i = 1; i < KMAX; ++i)
          if (has(i)) s += x[i][c];
        s = s / fk;
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < KMAX; ++i)
          if (has(i)) {
            const float df = x[i][c] - s;
            q = __builtin_fmaf(df, df, q);
          }
        const float p = perturb_coordinate(s, q, fk, kind);
        avg[c] = s;
        dir[c] = p;
        nn = __builtin_fmaf(s, s, nn);
        pp = __builtin_fmaf(p, p, pp);
#pragma unroll
        for (int i = 0; i < KMAX; ++i)
          if (has(i)) b[i] = __builtin_fmaf(p, s - x[i][c], b[i]);
      }
      store_stream<VEC>(avg_out + v * VEC, avg);
      store_stream<VEC>(dir_out + v * VEC, dir);
    }
    if ((it % kPerturbFold) == kPerturbFold - 1) {
#pragma unroll
      for (int i = 0; i < KMAX; ++i)
        if (has(i)) perturb_fold(b[i], mine + i);
      perturb_fold(pp, mine + BM_MAX_ROWS);
      perturb_fold(nn, mine + BM_MAX_ROWS + 1);
    }
  }
#pragma unroll
  for (int i = 0; i < KMAX; ++i)
    if (has(i)) perturb_fold(b[i], mine + i);
  perturb_fold(pp, mine + BM_MAX_ROWS);
  perturb_fold(nn, mine + BM_MAX_ROWS + 1);
  __syncthreads();
  if (threadIdx.x < kPerturbSlots) {
    double r = wide[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kPerturbBlock / 64; ++w) r += wide[w][threadIdx.x];
    partial[(int64_t)blockIdx.x * kPerturbSlots + threadIdx.x] = r;
  }
}

// one wave per scalar: lane l adds the partials of workgroups l, l + 64, ... in order, then a fixed shuffle tree
__global__ __launch_bounds__(64) void perturb_finish_kernel(const double* __restrict__ partial, int nparts,
                                                            double* __restrict__ scal_out) {
  const int s = blockIdx.x, lane = threadIdx.x;
  double tot = 0.0;
  for (int p = lane; p < nparts; p += 64) tot += partial[(int64_t)p * kPerturbSlots + s];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
  if (lane == 0) scal_out[s] = tot;
}

template <int KMAX, int VEC>
static int launch_perturb(const RowTable& tab, int k, int64_t nvec, float* avg, float* dir, int kind, double* partial,
                          int grid, hipStream_t s) {
  hipLaunchKernelGGL((perturb_stats_kernel<KMAX, VEC>), dim3(grid), dim3(kPerturbBlock), 0, s, tab, k, nvec, avg, dir,
                     kind, partial);
  BM_LAUNCH_CHECK();
  return 0;
}

// Row-count classes, one per kPerturbStep rows (the comparisons with the row count are then 8, not 64 scalar
// registers), and the widest column each keeps in registers without scratch (profiles/minmax_timings.txt holds the
// register counts): up to 24 rows 16 bytes, up to 40 rows 8, beyond 4.  A narrower class takes the same columns as more
// vectors.
template <int KMAX, int VEC>
static int launch_perturb_narrowed(const RowTable& tab, int k, int64_t nvec, float* avg, float* dir, int kind,
                                   double* partial, int grid, hipStream_t s) {
  constexpr int W = KMAX <= 24 ? 4 : (KMAX <= 40 ? 2 : 1);
  constexpr int V = VEC < W ? VEC : W;
  return launch_perturb<KMAX, V>(tab, k, nvec * (VEC / V), avg, dir, kind, partial, grid, s);
}
template <int VEC>
static int dispatch_perturb(const RowTable& tab, int k, int64_t nvec, float* avg, float* dir, int kind, double* partial,
                            int grid, hipStream_t s) {
  switch ((k + kPerturbStep - 1) / kPerturbStep) {
    case 1: return launch_perturb_narrowed<8, VEC>(tab, k, nvec, avg, dir, kind, partial, grid, s);
    case 2: return launch_perturb_narrowed<16, VEC>(tab, k, nvec, avg, dir, kind, partial, grid, s);
    case 3: return launch_perturb_narrowed<24, VEC>(tab, k, nvec, avg, dir, kind, partial, grid, s);
    case 4: return launch_perturb_narrowed<32, VEC>(tab, k, nvec, avg, dir, kind, partial, grid, s);
    case 5: return launch_perturb_narrowed<40, VEC>(tab, k, nvec, avg, dir, kind, partial, grid, s);
    case 6: return launch_perturb_narrowed<48, VEC>(tab, k, nvec, avg, dir, kind, partial, grid, s);
    case 7: return launch_perturb_narrowed<56, VEC>(tab, k, nvec, avg, dir, kind, partial, grid, s);
    default: return launch_perturb_narrowed<64, VEC>(tab, k, nvec, avg, dir, kind, partial, grid, s);
  }
}

// the grid cap of a launch: BM_PERTURB_GRID (tests) lowers it, so that a lane runs many iterations at a small d
static Caps perturb_caps() {
  const int knob = tuning().perturb_grid;
  const int cap = knob > 0 && knob < kPerturbMaxBlocks ? knob : kPerturbMaxBlocks - 1;
  return Caps{cap, cap + 1};
}
constexpr int kPerturbSets = kPerturbMaxBlocks;  // Caps{2047, 2048}.sets(): the most partial sets one piece writes

static bool overlaps(const float* a, const float* b, int64_t d) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  const uintptr_t len = (uintptr_t)d * sizeof(float);
  return x < y + len && y < x + len;
}

}  // namespace bm

extern "C" int64_t bm_perturb_workspace_bytes(int64_t d) {
  using namespace bm;
  if (d < 0) return BM_EINVAL;
  const int64_t pieces = piece_count(d) > 0 ? piece_count(d) : 1;
  return pieces * kPerturbSets * kPerturbSlots * (int64_t)sizeof(double);
}

extern "C" int bm_perturb_stats(const float* const* rows, int h, int64_t d, int kind, float* avg_out, float* dir_out,
                                double* scal_out, void* ws, void* stream) {
  using namespace bm;
  if (rows == nullptr || scal_out == nullptr || ws == nullptr || h < 2 || h > BM_MAX_ROWS || d < 0 ||
      (kind != BM_PERTURB_UNIT && kind != BM_PERTURB_STD && kind != BM_PERTURB_SIGN) ||
      (d > 0 && (avg_out == nullptr || dir_out == nullptr)))
    return BM_EINVAL;
  if (d > 0) {
    if (overlaps(avg_out, dir_out, d)) return BM_EINVAL;
    for (int i = 0; i < h; ++i)
      if (rows[i] == nullptr || overlaps(avg_out, rows[i], d) || overlaps(dir_out, rows[i], d)) return BM_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  RowTable tab{};
  for (int i = 0; i < h; ++i) tab.p[i] = rows[i];
  double* partial = static_cast<double*>(ws);
  const Caps caps = perturb_caps();
  int nparts = 0;
  // pieces of 2^29 columns; the width of a piece follows the alignment of its own first column
  const int rc = for_pieces(d, [&](int64_t lo, int64_t dp) {
    const RowTable t = tab.advanced(lo);
    float* const avg = avg_out + lo;
    float* const dir = dir_out + lo;
    const int vec = Alignment().of(t.p, h).of(avg).of(dir).vec();
    return for_body_and_tail<4>(Tail::kOwnLaunch, vec, dp, kPerturbBlock, caps, [&](auto width, const Span& sp) {
      return dispatch_perturb<decltype(width)::value>(t.advanced(sp.first), h, sp.count, avg + sp.first, dir + sp.first,
                                                      kind, partial + (int64_t)sp.part * kPerturbSlots, sp.grid, s);
    }, &nparts);
  });
  if (rc != 0) return rc;
  // d == 0: no partial at all, the finish kernel writes zeros
  hipLaunchKernelGGL(perturb_finish_kernel, dim3(kPerturbSlots), dim3(64), 0, s, partial, nparts, scal_out);
  BM_LAUNCH_CHECK();
  return 0;
}
