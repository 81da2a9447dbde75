// Host-side helpers of the entry points: every .hip file includes this header (composite_wide.inc has it through
// composite.hip), and nothing in it reaches a kernel.  It holds what the wrappers share -- the error codes (through the public header, their only
// definition), the stream cast, the grid size, the launch check, the value-to-template dispatch -- and the size rules
// that more than one wrapper needs, each written once.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/gsplat_hip.h"

#define GSR_CHECK_LAUNCH()                                            \
  do {                                                                \
    if (hipGetLastError() != hipSuccess) return GSR_ERR_LAUNCH_FAILED; \
  } while (0)

// Returns a failed call's code from the calling entry point.  Positive codes are results (the sorts report which buffer
// holds the output), so a caller that needs one keeps the value itself: `const int rc = f(...); if (rc < 0) return rc;`.
#define GSR_TRY(call)                  \
  do {                                 \
    const int rc__ = (call);           \
    if (rc__ < 0) return rc__;         \
  } while (0)

inline hipStream_t gsr_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

// Blocks that cover n items, `block` items each.  The arithmetic is 64-bit; a grid dimension is 32 bits wide.
inline unsigned grid_for(int64_t n, int64_t block) { return (unsigned)((n + block - 1) / block); }

// ---- value -> template argument ------------------------------------------------------------------------------------
// gsr_pick<1, 4, 9, 16>(K, [&](auto k) { kern<decltype(k)::value><<<...>>>(...); }) calls f once, with
// std::integral_constant<int, V> for the V that equals v, and returns whether one did: the list of values IS the set of
// instantiations, and the launch with its argument list is written once.  gsr_pick_bool does the same for a flag
// (std::true_type / std::false_type).  Pickers nest: one lambda inside the other gives the cross product.
template <int... Vs, class F>
inline bool gsr_pick(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

template <class F>
inline void gsr_pick_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

// ---- the rules ------------------------------------------------------------------------------------------------------
// SH coefficient counts with kernels: degrees 0..3.
inline bool gsr_sh_degree_ok(int K) { return K == 1 || K == 4 || K == 9 || K == 16; }
template <class F>
inline bool gsr_pick_sh(int K, F&& f) { return gsr_pick<1, 4, 9, 16>(K, f); }

// Feature channels of a narrow frame, carried inside the row.
template <class F>
inline bool gsr_pick_channels(int C, F&& f) { return gsr_pick<1, 2, 3>(C, f); }

// Floats per row of a wide frame's feature table: its 4..16 channels live in rows of 4, 8 or 16.
inline int gsr_wide_width(int C) { return C <= 4 ? 4 : C <= 8 ? 8 : 16; }
template <class F>
inline bool gsr_pick_wide(int C, F&& f) { return gsr_pick<4, 8, 16>(gsr_wide_width(C), f); }

// The 16 x 16 pixel tiles of a W x H image.
struct GsrTiles {
  int tx, ty;
  int64_t n;
};
inline GsrTiles gsr_tiles(int W, int H) {
  const int tx = (W + 15) / 16, ty = (H + 15) / 16;
  return {tx, ty, (int64_t)tx * ty};
}

// The frustum cull's workspace: one count per wave of `wave_span` rows, rounded to 256 bytes; behind them the scan's
// share and a spare 256.
struct GsrCullCarve {
  int64_t waves;
  size_t counts_bytes, total_bytes;
};
inline GsrCullCarve gsr_cull_carve(int64_t N, int64_t wave_span) {
  const int64_t waves = (N + wave_span - 1) / wave_span;
  const size_t counts = (((size_t)waves * sizeof(uint32_t) + 255) / 256) * 256;
  return {waves, counts, counts + gsr_scan_workspace_bytes(waves) + 256};
}
