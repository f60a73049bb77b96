// Host side of every tile launch: the grid of n workgroups, the launch itself and the dispatch from run-time sizes to the
// compiled instantiations.  One definition each, used by every kernel file whose grid is decoded on the device as
// blockIdx.y * gridDim.x + blockIdx.x (that decoding stays in each kernel).  Host only: nothing here is device code.
#pragma once
#include <hip/hip_ext.h>
#include <type_traits>
#include <utility>
#include "mia_common.h"
#include "mia_kernels.h"

namespace mia {

// ---- the grid: n workgroups as gx = min(n, 65536) columns and gy = ceil(n / gx) <= 65535 rows (the last row may be partly idle)
constexpr int64_t kGridColumns = 65536, kGridMaxRows = 65535;
constexpr int64_t kGridMaxBlocks = kGridColumns * kGridMaxRows;
// for the *_covers functions: a launch of n workgroups has a grid
static inline bool grid_covers(int64_t n) { return n <= kGridMaxBlocks; }
// n >= 1 (the entries return before any launch for an empty range)
static inline bool launch_grid(int64_t n, dim3* grid) {
  const int64_t gx = n < kGridColumns ? n : kGridColumns;
  const int64_t gy = (n + gx - 1) / gx;
  if (gy > kGridMaxRows) return false;
  *grid = dim3((unsigned)gx, (unsigned)gy);
  return true;
}

// ---- the launch.  In this order: refuse a dynamic LDS request above kMaxDynamicLds; raise the kernel's limit above 48 KB; form the
// grid of n_blocks workgroups or refuse; launch; note() -- the caller's note_analysis_kernel(...), also on the path where the launch
// check then fails; check.  CARRIED: the step driver's hot path (the float32 tile kernels) -- a completion event left in
// launch_stop_event() rides on this dispatch packet together with its optional start partner and both are cleared, so that no later
// launch takes them; every such launch counts in tile_launch_count().
template <bool CARRIED, typename Note, typename... KArgs, typename... Args>
static inline int launch_blocks_impl(void (*kern)(KArgs...), int64_t n_blocks, unsigned block, size_t lds, hipStream_t stream, Note&& note,
                                     const Args&... args) {
  if (lds > kMaxDynamicLds) return MIA_ERR_UNSUPPORTED;
  if (lds > 48 * 1024) MIA_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  dim3 grid;
  if (!launch_grid(n_blocks, &grid)) return MIA_ERR_UNSUPPORTED;
  if constexpr (CARRIED) {
    hipEvent_t& stop = launch_stop_event();
    if (stop) {
      hipExtLaunchKernelGGL(kern, grid, dim3(block), (unsigned)lds, stream, launch_start_event(), stop, 0, args...);
      stop = nullptr;        // taken
      launch_start_event() = nullptr;
    } else {
      kern<<<grid, dim3(block), lds, stream>>>(args...);
    }
    ++tile_launch_count();
  } else {
    kern<<<grid, dim3(block), lds, stream>>>(args...);
  }
  note();
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
template <typename Note, typename... KArgs, typename... Args>
static inline int launch_blocks(void (*kern)(KArgs...), int64_t n_blocks, unsigned block, size_t lds, hipStream_t stream, Note&& note,
                                const Args&... args) {
  return launch_blocks_impl<false>(kern, n_blocks, block, lds, stream, note, args...);
}
template <typename Note, typename... KArgs, typename... Args>
static inline int launch_blocks_carried(void (*kern)(KArgs...), int64_t n_blocks, unsigned block, size_t lds, hipStream_t stream, Note&& note,
                                        const Args&... args) {
  return launch_blocks_impl<true>(kern, n_blocks, block, lds, stream, note, args...);
}
// for the launches that are no step's analysis kernel
static inline void no_note() {}

// ---- from a run-time size to a compile-time constant: f(std::integral_constant<int, V>) for the V among Vs... that equals v;
// MIA_ERR_UNSUPPORTED when none does.  f is instantiated for exactly the values listed; what it leaves out for a value
// (if constexpr) is not built.  No allocation, no type erasure: one compare chain, as the switch ladders it replaces.
// The values are listed from the largest down (dispatch_upto tries N first): the device pass emits the kernels first named inside
// nested generic lambdas in the reverse of that order, so each code object keeps its kernels in ascending order, byte for byte
// what the ladders produced.  Which value is compared first makes no difference to a launch.
template <int... Vs, typename F>
static inline int dispatch_among(int v, F&& f) {
  int rc = MIA_ERR_UNSUPPORTED;
  (void)((v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  return rc;
}
template <typename F, int... Is>
static inline int dispatch_upto_impl(int v, F&& f, std::integer_sequence<int, Is...>) { return dispatch_among<(int)(sizeof...(Is) - Is)...>(v, f); }
// ... for 1 <= v <= N
template <int N, typename F>
static inline int dispatch_upto(int v, F&& f) { return dispatch_upto_impl(v, f, std::make_integer_sequence<int, N>{}); }

}  // namespace mia
