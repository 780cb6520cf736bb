// launch_plan.h — how a pass over d coordinates is cut into launches (host code only): the ONE place where the vector
// width, the body / tail split, the pieces of at most 2^29 columns, the grids and the order of the fp64 partial sums
// are decided.  A launch site states its kernel, block size, caps and partial stride and receives Spans.
#pragma once
#include <stdint.h>
#include <type_traits>

namespace bm {

// Columns per launch such that every byte offset fits 32 bits (saddr addressing).
constexpr int64_t kMaxColsPerLaunch = (int64_t)1 << 29;

// Grid size for a streaming kernel: enough workgroups to fill 256 CUs several times over,
// capped so that the grid-stride loop amortises launch/tail effects.
static inline int stream_grid(int64_t work_items, int block, int max_blocks) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > max_blocks) g = max_blocks;
  return (int)g;
}

// Largest vector width (4, 2 or 1 floats: 16 / 8 / 4-byte accesses) that every pointer given allows.  Null pointers
// do not constrain the width.
class Alignment {
 public:
  Alignment& of(const void* p) {
    bits_ |= reinterpret_cast<uintptr_t>(p);
    return *this;
  }
  template <class P>
  Alignment& of(P* const* table, int n) {
    for (int i = 0; i < n; ++i) of(table[i]);
    return *this;
  }
  int vec() const { return (bits_ & 15u) == 0 ? 4 : ((bits_ & 7u) == 0 ? 2 : 1); }

 private:
  uintptr_t bits_ = 0;
};

// Pointer tables advance themselves (`advanced(by)` of each table type) through these: null stays null.
template <class T>
static inline T* advanced(T* p, int64_t by) {
  return p != nullptr ? p + by : nullptr;
}
template <class T, int K>
static inline void advance(T* (&table)[K], int64_t by) {
  for (int i = 0; i < K; ++i) table[i] = advanced(table[i], by);
}

// The pieces of at most kMaxColsPerLaunch columns of a pass whose kernels address with 32-bit byte offsets:
// piece(lo, count) for each, in order; the first non-zero code ends the walk.  (max_cols: a launch site whose tests walk
// several pieces at a small d passes a smaller piece, never a larger one.)
static inline int64_t piece_count(int64_t d) { return d > 0 ? (d + kMaxColsPerLaunch - 1) / kMaxColsPerLaunch : 0; }
template <class Piece>
static int for_pieces(int64_t d, Piece&& piece, int64_t max_cols = kMaxColsPerLaunch) {
  for (int64_t lo = 0; lo < d; lo += max_cols) {
    const int64_t count = (d - lo < max_cols) ? (d - lo) : max_cols;
    if (const int rc = piece(lo, count)) return rc;
  }
  return 0;
}

// Grid caps of a pass's two launches.  A kernel that leaves one set of fp64 partial sums per workgroup writes at most
// sets() of them: a tail behind a body is one workgroup, a tail alone takes the whole grid.  Workspace sizes are
// computed from the same object the launch site passes.
struct Caps {
  int body, tail;
  constexpr int sets() const { return body + 1 > tail ? body + 1 : tail; }
};
constexpr Caps caps_of(int both) { return Caps{both, both}; }

// One launch of a cut pass.
struct Span {
  int64_t first;  // first coordinate: add it to every pointer
  int64_t count;  // vectors of VEC floats (VEC = 1: coordinates)
  int64_t end;    // one past the last coordinate this launch covers, a riding tail included
  int tail;       // trailing coordinates that ride in the last workgroup (Tail::kRides*), else 0
  int grid;       // workgroups of the plain form; a launch that takes fewer (burst forms: one per CU) says so here
  int part;       // index of this launch's first partial set in the workspace
};

// What becomes of the d % VEC trailing coordinates — a property of the kernel:
enum class Tail {
  kOwnLaunch,      // a VEC = 1 launch of the same kernel behind the body; a pass shorter than one vector is that launch alone
  kRides,          // the last workgroup of the body's launch takes them, at the pointers' width whatever d is
  kRidesNarrowed,  // the same, at the widest width that has at least one whole vector
};

template <int VEC>
using Width = std::integral_constant<int, VEC>;

// launch(Width<VEC>{}, span) -> code, at the width vec; widths above MAXVEC are never instantiated.
template <int MAXVEC, class Launch>
static int launch_at_width(int vec, Launch&& launch, Span& span) {
  if constexpr (MAXVEC >= 4)
    if (vec == 4) return launch(Width<4>{}, span);
  if constexpr (MAXVEC >= 2)
    if (vec >= 2) return launch(Width<2>{}, span);
  return launch(Width<1>{}, span);
}

// Cuts d coordinates at the width `vec` (capped at MAXVEC, the widest instance of the kernel) and calls
// launch(Width<VEC>{}, span) for the body and, under Tail::kOwnLaunch, for the scalar tail, in that order.  Returns the
// first non-zero code.  *nparts (in / out, may be null) counts the partial sets written so far: span.part numbers them
// in launch order, which is the fixed order the finish kernels add them in.  d == 0 launches nothing.
template <int MAXVEC, class Launch>
static int for_body_and_tail(Tail mode, int vec, int64_t d, int block, Caps caps, Launch&& launch, int* nparts = nullptr) {
  int parts = nparts != nullptr ? *nparts : 0;
  if (vec > MAXVEC) vec = MAXVEC;
  if (mode == Tail::kOwnLaunch && d / vec == 0) vec = 1;
  while (mode == Tail::kRidesNarrowed && vec > 1 && d / vec == 0) vec /= 2;
  const int64_t nvec = d / vec;
  int64_t body = 0;
  if (d > 0 && (vec > 1 || mode != Tail::kOwnLaunch)) {
    body = nvec * vec;
    const int rides = mode == Tail::kOwnLaunch ? 0 : (int)(d - body);
    Span span{0, nvec, body + rides, rides, stream_grid(nvec, block, caps.body), parts};
    if (const int rc = launch_at_width<MAXVEC>(vec, launch, span)) return rc;
    parts += span.grid;
    body += rides;
  }
  if (body < d) {
    const int64_t rest = d - body;
    Span span{body, rest, d, 0, body == 0 ? stream_grid(rest, block, caps.tail) : 1, parts};
    if (const int rc = launch(Width<1>{}, span)) return rc;
    parts += span.grid;
  }
  if (nparts != nullptr) *nparts = parts;
  return 0;
}

}  // namespace bm
