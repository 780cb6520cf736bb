// reduce.hip — row averaging by a device index table, fused stack statistics, fused dot
// products and the multi-vector momentum update.
//
// Replaces (reference, PyTorch):
//   sum(grad for _, grad in scores[:m]).div_(m)          krum.py:80, brute.py:80, aksel.py:64
//   tools.compute_avg_dev_max                             tools/pytorch.py:97-125
//   torch.dot(...)/norm() chains of the study block       attack.py:851-868
//   gmtm.mul_(mu).add_(grad, alpha=1-damp) per worker     attack.py:800-804
// Each is ONE pass over its inputs with every reduction deterministic (fixed trees, fp64
// across lanes/workgroups, no float atomics) and no host synchronisation.
#include "bm_common.h"
#include "rank_body.h"
#include "table_sum.h"

namespace bm {

constexpr int kRedBlock = 256;
constexpr int kMaxPartialBlocks = 2048;
constexpr Caps kStatsCaps{kMaxPartialBlocks - 1, kMaxPartialBlocks};  // bm_stack_stats: 3 partials per workgroup
constexpr int kMeanMaxBlocks = 256 * 32;

// ---------------------------------------------------------------------------
// selected_mean: out = (((0 + R[idx0]) + R[idx1]) + ... ) / m, sequential fp32 (MeanFold, table_sum.h).
// ---------------------------------------------------------------------------
static_assert(kRedBlock == kTableBlock, "bm_selected_mean cuts its pass for kRedBlock lanes; the plain driver walks kTableBlock");

// sel[k] = the row idx[k] names; returns the divisor.  A NEGATIVE index is the Brute search saying "no selection, do not
// use this" (brute.hip): the divisor is then NaN, the mean NaN everywhere.  Every lane of the workgroup must call.
__device__ __forceinline__ float selected_mean_prologue(const RowTable& rows, const int32_t* __restrict__ idx, int m,
                                                        float fm, const float** sel) {
  __shared__ int poisoned;
  if (threadIdx.x == 0) poisoned = 0;
  __syncthreads();
  if (threadIdx.x < m) {
    const int i = load_index_coherent(idx + threadIdx.x);
    if (i < 0) poisoned = 1;
    sel[threadIdx.x] = rows.p[i < 0 ? 0 : i];
  }
  __syncthreads();
  return poisoned ? __builtin_nanf("") : fm;
}

template <int VEC>
__global__ __launch_bounds__(kTableBlock) void selected_mean_kernel(RowTable rows, const int32_t* __restrict__ idx, int m,
                                                                    int64_t nvec, float fm, float* __restrict__ out, int tail) {
  __shared__ const float* sel[BM_MAX_ROWS];
  const MeanFold fold{selected_mean_prologue(rows, idx, m, fm, sel)};
  table_sum_plain<VEC>(sel, m, nvec, tail, out, fold);
}

// Burst form of the same kernel for long gradients (table_sum_burst): 9 x 1024 x 16 B = 144 KB of results next to the
// pointer table.
constexpr int kMeanBurstThreads = 1024;
constexpr int kMeanBurstSlots = 9;
__global__ __launch_bounds__(kMeanBurstThreads) void selected_mean_burst_kernel(RowTable rows, const int32_t* __restrict__ idx,
                                                                                int m, int64_t nvec, float fm,
                                                                                float* __restrict__ out, int tail) {
  __shared__ const float* sel[BM_MAX_ROWS];
  const MeanFold fold{selected_mean_prologue(rows, idx, m, fm, sel)};
  table_sum_burst<kMeanBurstThreads, kMeanBurstSlots>(sel, m, nvec, tail, out, fold);
}

template <int VEC>
static int launch_selected_mean(const RowTable& tab, const int32_t* idx, int m, const Span& sp, float* out,
                                hipStream_t s) {
  const int64_t nvec = sp.count;
  if constexpr (VEC == 4) {
    const int cus = compute_units();
    // measured (profiles/r02_i_selected_mean_burst.txt): m = 37 at 11.2 M 306.7 -> 284.4 us, m = 18 at 36.5 M
    // 510.7 -> 471.9 us, m = 7 at 9 M 56.7 -> 58.0 us: from 12 rows and 8 iterations per CU on
    if (tuning().mean_burst > 0 && m >= 12 && nvec < ((int64_t)1 << 30) &&
        nvec / ((int64_t)cus * kMeanBurstThreads) >= tuning().mean_burst) {
      hipLaunchKernelGGL(selected_mean_burst_kernel, dim3(cus), dim3(kMeanBurstThreads), 0, s, tab, idx, m, nvec,
                         (float)m, out, sp.tail);
      BM_LAUNCH_CHECK();
      return 0;
    }
  }
  hipLaunchKernelGGL(selected_mean_kernel<VEC>, dim3(sp.grid), dim3(kTableBlock), 0, s, tab, idx, m, nvec,
                     (float)m, out, sp.tail);
  BM_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// stack_stats: avg (sequential mean of k rows), ||avg||^2, sum_i ||x_i-avg||^2, max|avg|.
// Per-lane fp32 partials cover only a few dozen columns, everything wider is fp64.
// ---------------------------------------------------------------------------
template <int KMAX, int VEC>
__global__ __launch_bounds__(kRedBlock) void stack_stats_kernel(RowTable rows, int k, int64_t nvec,
                                                                float* __restrict__ avg_out,
                                                                float* __restrict__ scaled_out,
                                                                float scale, int attack_kind, int nt_result,
                                                                double* __restrict__ partial) {
  __shared__ double red[kRedBlock / 64];
  const float fk = (float)k;
  float norm2 = 0.0f, dev2 = 0.0f, amax = 0.0f;
  bool seen_nan = false;
  const int64_t stride = (int64_t)gridDim.x * kRedBlock;
  for (int64_t v = (int64_t)blockIdx.x * kRedBlock + threadIdx.x; v < nvec; v += stride) {
    float x[KMAX][VEC];
#pragma unroll
    for (int i = 0; i < KMAX; ++i)
      if (i < k) load_stream<VEC>(rows.p[i] + v * VEC, x[i]);
    float avg[VEC], colq[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      float s = x[0][c];  // grad_avg = samples[0].clone(); add_(...)  (tools/pytorch.py:108-110)
#pragma unroll
      for (int i = 1; i < KMAX; ++i)
        if (i < k) s += x[i][c];
      s = s / fk;
      avg[c] = s;
      norm2 = __builtin_fmaf(s, s, norm2);
      const float as = __builtin_fabsf(s);
      amax = fmaxf(amax, as);
      seen_nan |= (s != s);
      float q = 0.0f;
#pragma unroll
      for (int i = 0; i < KMAX; ++i)
        if (i < k) {
          const float df = x[i][c] - s;
          q = __builtin_fmaf(df, df, q);
        }
      dev2 += q;
      colq[c] = q;
    }
    if (avg_out != nullptr) store_result_policy<VEC>(avg_out + v * VEC, avg, nt_result);
    if (scaled_out != nullptr) {
      float sc[VEC];
#pragma unroll
      for (int c = 0; c < VEC; ++c) sc[c] = byzantine_coordinate(avg[c], colq[c], fk, scale, attack_kind);
      store_result_policy<VEC>(scaled_out + v * VEC, sc, nt_result);
    }
  }
  // torch's abs().max() propagates NaN; fmaxf does not
  if (seen_nan) amax = __builtin_nanf("");
  const double n2 = block_reduce_sum<kRedBlock>((double)norm2, red);
  const double d2 = block_reduce_sum<kRedBlock>((double)dev2, red);
  // max: NaN-propagating tree
  float m = amax;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_down(m, off, 64);
    m = (m != m || o != o) ? __builtin_nanf("") : fmaxf(m, o);
  }
  __shared__ float mred[kRedBlock / 64];
  if ((threadIdx.x & 63) == 0) mred[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float mm = mred[0];
    for (int w = 1; w < kRedBlock / 64; ++w) {
      const float o = mred[w];
      mm = (mm != mm || o != o) ? __builtin_nanf("") : fmaxf(mm, o);
    }
    partial[blockIdx.x * 3 + 0] = n2;
    partial[blockIdx.x * 3 + 1] = d2;
    partial[blockIdx.x * 3 + 2] = (double)mm;
  }
}

// Scalar tail (d % VEC columns) folded into the same partial array as one more "workgroup".
__global__ void stats_finish_kernel(const double* __restrict__ partial, int nparts,
                                    double* __restrict__ out3) {
  // one wave; fixed-order reduction of the per-workgroup partials
  const int lane = threadIdx.x;
  double n2 = 0.0, d2 = 0.0, mx = 0.0;
  bool nan = false;
  for (int b = lane; b < nparts; b += 64) {
    n2 += partial[b * 3 + 0];
    d2 += partial[b * 3 + 1];
    const double m = partial[b * 3 + 2];
    nan |= (m != m);
    mx = m > mx ? m : mx;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n2 += __shfl_down(n2, off, 64);
    d2 += __shfl_down(d2, off, 64);
    const double o = __shfl_down(mx, off, 64);
    mx = o > mx ? o : mx;
    nan |= (bool)__shfl_down((int)nan, off, 64);
  }
  if (lane == 0) {
    out3[0] = n2;
    out3[1] = d2;
    out3[2] = nan ? __builtin_nan("") : mx;
  }
}

template <int KMAX, int VEC>
static int launch_stack_stats(const RowTable& tab, int k, int64_t nvec, float* avg, float* scaled,
                              float scale, int kind, double* partial, int grid, hipStream_t s) {
  hipLaunchKernelGGL((stack_stats_kernel<KMAX, VEC>), dim3(grid), dim3(kRedBlock), 0, s, tab, k, nvec,
                     avg, scaled, scale, kind, 1, partial);
  BM_LAUNCH_CHECK();
  return 0;
}

template <int VEC>
static int dispatch_stack_stats(const RowTable& tab, int k, int64_t nvec, float* avg, float* scaled,
                                float scale, int kind, double* partial, int grid, hipStream_t s) {
  if (k <= 8) return launch_stack_stats<8, VEC>(tab, k, nvec, avg, scaled, scale, kind, partial, grid, s);
  if (k <= 16) return launch_stack_stats<16, VEC>(tab, k, nvec, avg, scaled, scale, kind, partial, grid, s);
  if (k <= 24) return launch_stack_stats<24, VEC>(tab, k, nvec, avg, scaled, scale, kind, partial, grid, s);
  if (k <= 32)
    return launch_stack_stats<32, (VEC > 2 ? 2 : VEC)>(tab, k, nvec * (VEC > 2 ? VEC / 2 : 1), avg, scaled,
                                                        scale, kind, partial, grid, s);
  return launch_stack_stats<64, 1>(tab, k, nvec * VEC, avg, scaled, scale, kind, partial, grid, s);
}

// ---------------------------------------------------------------------------
// multi_dot: Gram matrix of <= 4 "core" vectors + dot(core[0], extra[e]) for <= 32 extras.
// ---------------------------------------------------------------------------
constexpr int kMaxCore = 4;
constexpr int kMaxExtra = 32;
constexpr int kDotSlots = kMaxCore * (kMaxCore + 1) / 2 + kMaxExtra;  // 42

constexpr Caps kDotCaps = caps_of(1024);

struct DotTable {
  const float* core[kMaxCore];
  const float* extra[kMaxExtra];
  DotTable advanced(int64_t by) const {
    DotTable t = *this;
    advance(t.core, by);
    advance(t.extra, by);
    return t;
  }
};

template <int VEC>
__global__ __launch_bounds__(kRedBlock) void multi_dot_kernel(DotTable tab, int nc, int ne,
                                                              int64_t nvec,
                                                              double* __restrict__ partial) {
  __shared__ double red[kRedBlock / 64];
  float acc[kDotSlots];
#pragma unroll
  for (int i = 0; i < kDotSlots; ++i) acc[i] = 0.0f;
  const int64_t stride = (int64_t)gridDim.x * kRedBlock;
  for (int64_t v = (int64_t)blockIdx.x * kRedBlock + threadIdx.x; v < nvec; v += stride) {
    float c[kMaxCore][VEC];
#pragma unroll
    for (int a = 0; a < kMaxCore; ++a)
      if (a < nc) load_stream<VEC>(tab.core[a] + v * VEC, c[a]);
    int slot = 0;
#pragma unroll
    for (int a = 0; a < kMaxCore; ++a)
#pragma unroll
      for (int b = a; b < kMaxCore; ++b) {
        if (b < nc) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[slot] = __builtin_fmaf(c[a][e], c[b][e], acc[slot]);
        }
        ++slot;
      }
#pragma unroll
    for (int x = 0; x < kMaxExtra; ++x)
      if (x < ne) {
        float t[VEC];
        load_stream<VEC>(tab.extra[x] + v * VEC, t);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[slot + x] = __builtin_fmaf(c[0][e], t[e], acc[slot + x]);
      }
  }
#pragma unroll
  for (int i = 0; i < kDotSlots; ++i) {
    const double r = block_reduce_sum<kRedBlock>((double)acc[i], red);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * kDotSlots + i] = r;
  }
}

__global__ __launch_bounds__(64) void dot_finish_kernel(const double* __restrict__ partial, int nparts,
                                                        int nc, int ne, double* __restrict__ out) {
  // one wave per slot: lane l adds the partials of workgroups l, l+64, ... in order, then a fixed
  // shuffle tree (a single thread walking 1024 partials was 250 us of dependent loads)
  const int s = blockIdx.x, lane = threadIdx.x;
  double tot = 0.0;
  for (int b = lane; b < nparts; b += 64) tot += partial[(int64_t)b * kDotSlots + s];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
  if (lane != 0) return;
  // slot -> (a, b) of the upper triangle of a kMaxCore x kMaxCore matrix, or extra index
  int slot = 0;
  for (int a = 0; a < kMaxCore; ++a)
    for (int b = a; b < kMaxCore; ++b) {
      if (slot == s && b < nc) {
        out[a * nc + b] = tot;
        out[b * nc + a] = tot;
      }
      ++slot;
    }
  const int x = s - kMaxCore * (kMaxCore + 1) / 2;
  if (x >= 0 && x < ne) out[nc * nc + x] = tot;
}

// ---------------------------------------------------------------------------
// row_sqnorms: sq[i] = sum_j rows[i][j]^2 for k rows, every row read once by its own slice of the grid
// (blockIdx.y = row).  Behind cge.py:28-38 (`gradient.norm().item()` per gradient) and the clipping of
// attack.py:776-779,791-794; round 2 took the norms from 4 x 4 Gram blocks (bm_multi_dot, ceil(k/4) launches).
// ---------------------------------------------------------------------------
constexpr int kNormBlocks = 128;  // workgroups per row; body and tail partials of every row share the BM_WS_DOT workspace
static_assert(2 * BM_MAX_ROWS * kNormBlocks <= kDotCaps.sets() * kDotSlots, "bm_row_sqnorms: partials exceed BM_WS_DOT");
template <int VEC>
__global__ __launch_bounds__(kRedBlock) void row_sqnorms_kernel(RowTable rows, int64_t nvec, double* __restrict__ partial) {
  __shared__ double red[kRedBlock / 64];
  const float* row = rows.p[blockIdx.y];
  float acc[2] = {0.0f, 0.0f};
  double wide = 0.0;  // the fp32 chains are folded into fp64 every 16 iterations: their length does not grow with d
  const int64_t stride = (int64_t)gridDim.x * kRedBlock;
  int64_t v = (int64_t)blockIdx.x * kRedBlock + threadIdx.x;
  int since = 0;
  for (; v + stride < nvec; v += 2 * stride) {  // two loads in flight per lane
    float a[VEC], b[VEC];
    load_stream<VEC>(row + v * VEC, a);
    load_stream<VEC>(row + (v + stride) * VEC, b);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[0] = __builtin_fmaf(a[e], a[e], acc[0]);
      acc[1] = __builtin_fmaf(b[e], b[e], acc[1]);
    }
    if (++since == 16) {
      wide += (double)acc[0] + (double)acc[1];
      acc[0] = acc[1] = 0.0f;
      since = 0;
    }
  }
  if (v < nvec) {
    float a[VEC];
    load_stream<VEC>(row + v * VEC, a);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[0] = __builtin_fmaf(a[e], a[e], acc[0]);
  }
  const double r = block_reduce_sum<kRedBlock>(wide + ((double)acc[0] + (double)acc[1]), red);
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
}

// one wave per row: fixed-order sum of the row's body partials and of its (scalar) tail partial
__global__ __launch_bounds__(64) void row_sqnorms_finish_kernel(const double* __restrict__ body, int nbody,
                                                               const double* __restrict__ tail, int ntail,
                                                               double* __restrict__ out) {
  const int row = blockIdx.x, lane = threadIdx.x;
  double tot = 0.0;
  for (int b = lane; b < nbody; b += 64) tot += body[(int64_t)row * nbody + b];
  for (int b = lane; b < ntail; b += 64) tot += tail[(int64_t)row * ntail + b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
  if (lane == 0) out[row] = tot;
}

// ---------------------------------------------------------------------------
// multi_axpby: y_i = fma(b, x_i, a*y_i) for k vectors; blockIdx.y selects the vector.
// (torch's vectorised `add_(x, alpha=b)` after `mul_(a)` is a*y rounded, then one fused
//  multiply-add.)
// ---------------------------------------------------------------------------
struct AxpbyTable {
  float* y[BM_MAX_ROWS];
  const float* x[BM_MAX_ROWS];
  AxpbyTable advanced(int64_t by) const {
    AxpbyTable t = *this;
    advance(t.y, by);
    advance(t.x, by);
    return t;
  }
};

// (An unrolled variant with 4 vectors in flight per lane and non-temporal y accesses was measured
//  8 % slower at k = 20, d = 36.5 M: 1.79 ms against 1.66 ms = 5.3 TB/s for this form.)
template <int VEC>
__global__ __launch_bounds__(kRedBlock) void multi_axpby_kernel(AxpbyTable tab, int64_t nvec, float a,
                                                                float b) {
  float* __restrict__ y = tab.y[blockIdx.y];
  const float* __restrict__ x = tab.x[blockIdx.y];
  const int64_t stride = (int64_t)gridDim.x * kRedBlock;
  for (int64_t v = (int64_t)blockIdx.x * kRedBlock + threadIdx.x; v < nvec; v += stride) {
    float yy[VEC], xx[VEC];
    using T = typename VecLoad<VEC>::T;
    const T yv = *reinterpret_cast<const T*>(y + v * VEC);
    if constexpr (VEC == 1) {
      yy[0] = yv;
    } else {
#pragma unroll
      for (int c = 0; c < VEC; ++c) yy[c] = yv[c];
    }
    load_stream<VEC>(x + v * VEC, xx);
#pragma unroll
    for (int c = 0; c < VEC; ++c) yy[c] = __builtin_fmaf(b, xx[c], a * yy[c]);
    T ov;
    if constexpr (VEC == 1) {
      ov = yy[0];
    } else {
#pragma unroll
      for (int c = 0; c < VEC; ++c) ov[c] = yy[c];
    }
    *reinterpret_cast<T*>(y + v * VEC) = ov;
  }
}

// Stable argsort of n (<= 64) fp64 keys on the device; NaN keys rank last (as +inf).
__global__ __launch_bounds__(64) void stable_argsort_kernel(const double* __restrict__ keys, int n,
                                                            int32_t* __restrict__ order) {
  __shared__ double k[BM_MAX_ROWS];
  stable_argsort_body((int)threadIdx.x < n ? keys[threadIdx.x] : 0.0, n, k, order);
}

int64_t stats_workspace_bytes() { return (int64_t)kStatsCaps.sets() * 3 * (int64_t)sizeof(double); }
int64_t dot_workspace_bytes() { return (int64_t)kDotCaps.sets() * kDotSlots * (int64_t)sizeof(double); }

}  // namespace bm

extern "C" int bm_selected_mean(const float* const* rows, int n, const int32_t* idx, int m,
                                int64_t d, float* out, void* stream) {
  using namespace bm;
  if (rows == nullptr || idx == nullptr || (out == nullptr && d > 0) || n < 1 || n > BM_MAX_ROWS || m < 1 ||
      m > BM_MAX_ROWS || d < 0)
    return BM_EINVAL;
  if (d == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  RowTable tab{};
  for (int i = 0; i < n; ++i) tab.p[i] = rows[i];
  const int vec = Alignment().of(rows, n).of(out).vec();
  // (the d % VEC trailing columns ride in the last workgroup of the body's launch: no launch of their own)
  return for_body_and_tail<4>(Tail::kRidesNarrowed, vec, d, kRedBlock, caps_of(kMeanMaxBlocks), [&](auto width, const Span& sp) {
    return launch_selected_mean<decltype(width)::value>(tab, idx, m, sp, out, s);
  });
}

extern "C" int bm_stack_stats(const float* const* rows, int k, int64_t d, float* avg_out,
                              float* scaled_out, float scale, int attack_kind, double* out3, void* ws,
                              void* stream) {
  using namespace bm;
  // d == 0 is legal (an empty trailing shard): the finish kernel then writes zeros, so that every rank
  // of a sharded job reaches its collective
  if (rows == nullptr || out3 == nullptr || ws == nullptr || k < 1 || k > BM_MAX_ROWS || d < 0 ||
      ((attack_kind & ~BM_ATTACK_DIRECTION) != BM_ATTACK_EMPIRE && (attack_kind & ~BM_ATTACK_DIRECTION) != BM_ATTACK_LITTLE))
    return BM_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  RowTable tab{};
  for (int i = 0; i < k; ++i) tab.p[i] = rows[i];
  double* partial = static_cast<double*>(ws);
  const int vec = Alignment().of(rows, k).of(avg_out).of(scaled_out).vec();
  int nparts = 0;
  const int rc = for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, kRedBlock, kStatsCaps, [&](auto width, const Span& sp) {
    return dispatch_stack_stats<decltype(width)::value>(tab.advanced(sp.first), k, sp.count, advanced(avg_out, sp.first),
                                                        advanced(scaled_out, sp.first), scale, attack_kind,
                                                        partial + (int64_t)sp.part * 3, sp.grid, s);
  }, &nparts);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(64), 0, s, partial, nparts, out3);
  BM_LAUNCH_CHECK();
  return 0;
}

extern "C" int bm_multi_dot(const float* const* core, int nc, const float* const* extra, int ne,
                            int64_t d, double* out, void* ws, void* stream) {
  using namespace bm;
  if (core == nullptr || out == nullptr || ws == nullptr || nc < 1 || nc > kMaxCore || ne < 0 ||
      ne > kMaxExtra || (ne > 0 && extra == nullptr) || d < 0)
    return BM_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DotTable tab{};
  for (int i = 0; i < nc; ++i) tab.core[i] = core[i];
  for (int i = 0; i < ne; ++i) tab.extra[i] = extra[i];
  double* partial = static_cast<double*>(ws);
  const int vec = Alignment().of(core, nc).of(extra, ne).vec();
  int nparts = 0;
  const int rc = for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, kRedBlock, kDotCaps, [&](auto width, const Span& sp) {
    hipLaunchKernelGGL(multi_dot_kernel<decltype(width)::value>, dim3(sp.grid), dim3(kRedBlock), 0, s,
                       tab.advanced(sp.first), nc, ne, sp.count, partial + (int64_t)sp.part * kDotSlots);
    BM_LAUNCH_CHECK();
    return 0;
  }, &nparts);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(dot_finish_kernel, dim3(kDotSlots), dim3(64), 0, s, partial, nparts, nc, ne, out);
  BM_LAUNCH_CHECK();
  return 0;
}

extern "C" int bm_multi_axpby(float* const* y, const float* const* x, int k, int64_t d, float a,
                              float b, void* stream) {
  using namespace bm;
  if (y == nullptr || x == nullptr || k < 1 || k > BM_MAX_ROWS || d < 0) return BM_EINVAL;
  if (d == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  AxpbyTable tab{};
  for (int i = 0; i < k; ++i) {
    tab.y[i] = y[i];
    tab.x[i] = x[i];
  }
  const int vec = Alignment().of(y, k).of(x, k).vec();
  return for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, kRedBlock, caps_of(2048), [&](auto width, const Span& sp) {
    hipLaunchKernelGGL(multi_axpby_kernel<decltype(width)::value>, dim3(sp.grid, k), dim3(kRedBlock), 0, s,
                       tab.advanced(sp.first), sp.count, a, b);
    BM_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int bm_stable_argsort(const double* keys, int n, int32_t* order_out, void* stream) {
  using namespace bm;
  if (keys == nullptr || order_out == nullptr || n < 1 || n > BM_MAX_ROWS) return BM_EINVAL;
  hipLaunchKernelGGL(stable_argsort_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                     keys, n, order_out);
  BM_LAUNCH_CHECK();
  return 0;
}

extern "C" int bm_row_sqnorms(const float* const* rows, int k, int64_t d, double* sq_out, void* ws, void* stream) {
  using namespace bm;
  if (rows == nullptr || sq_out == nullptr || ws == nullptr || k < 1 || k > BM_MAX_ROWS || d < 0) return BM_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  RowTable tab{};
  for (int i = 0; i < k; ++i) tab.p[i] = rows[i];
  const int vec = Alignment().of(rows, k).vec();
  double* body_part = static_cast<double*>(ws);
  double* tail_part = body_part + (int64_t)BM_MAX_ROWS * kNormBlocks;
  int nbody = 0, ntail = 0;
  // (partials are row-major per launch, so body and tail keep an area each: under kOwnLaunch the VEC = 1 launch is the tail)
  const int rc = for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, kRedBlock, caps_of(kNormBlocks), [&](auto width, const Span& sp) {
    constexpr int VEC = decltype(width)::value;
    (VEC == 1 ? ntail : nbody) = sp.grid;
    hipLaunchKernelGGL(row_sqnorms_kernel<VEC>, dim3(sp.grid, k), dim3(kRedBlock), 0, s, tab.advanced(sp.first), sp.count,
                       VEC == 1 ? tail_part : body_part);
    BM_LAUNCH_CHECK();
    return 0;
  });
  if (rc != 0) return rc;
  // d == 0: no partial at all, the finish kernel writes zeros
  hipLaunchKernelGGL(row_sqnorms_finish_kernel, dim3(k), dim3(64), 0, s, body_part, nbody, tail_part, ntail, sq_out);
  BM_LAUNCH_CHECK();
  return 0;
}
