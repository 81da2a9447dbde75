// Device-side helpers for gfx950 (wave64).  No portability layer: DPP row shifts / row broadcasts are the
// CDNA cross-lane path, ballots are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_math.h"

#define GSR_WAVE 64

// Orders this wave's LDS accesses across its lanes (one wave per workgroup exchanges data through LDS without
// s_barrier): a wavefront-scope fence + wave barrier.  Emits no instruction -- LDS operations of one wave execute in
// order -- but keeps the compiler from moving the reads above the writes (or the next writes above the reads).
__device__ __forceinline__ void gsr_wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int gsr_lane() { return (int)(threadIdx.x & 63); }

// v + (DPP-moved v); lanes without a source read 0 (bound_ctrl).
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ float gsr_dpp_add(float v) {
  int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, BANK_MASK, true);
  return v + __int_as_float(moved);
}

// Sum over the 64 lanes in a FIXED association order (bit-reproducible); the total lands in lane 63.
__device__ __forceinline__ float gsr_wave_sum_to_lane63(float v) {
  v = gsr_dpp_add<0x111, 0xf, 0xf>(v);   // row_shr:1
  v = gsr_dpp_add<0x112, 0xf, 0xf>(v);   // row_shr:2
  v = gsr_dpp_add<0x114, 0xf, 0xf>(v);   // row_shr:4
  v = gsr_dpp_add<0x118, 0xf, 0xf>(v);   // row_shr:8   -> lane 15 of each row holds its row sum
  v = gsr_dpp_add<0x142, 0xa, 0xf>(v);   // row_bcast:15 into rows 1,3
  v = gsr_dpp_add<0x143, 0xc, 0xf>(v);   // row_bcast:31 into rows 2,3 -> lane 63 holds the total
  return v;
}

__device__ __forceinline__ float gsr_wave_sum(float v) {   // total broadcast to every lane (via SGPR)
  v = gsr_wave_sum_to_lane63(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

__device__ __forceinline__ uint32_t gsr_wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// inclusive prefix sum across the wave
__device__ __forceinline__ uint32_t gsr_wave_scan_incl_u32(uint32_t v) {
  const int lane = gsr_lane();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  return v;
}

__device__ __forceinline__ int gsr_mbcnt(uint64_t mask) {  // number of set bits of mask below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// position of the n-th set bit of m, n < popcount(m)
__device__ __forceinline__ int gsr_nth_set_bit(uint64_t m, int n) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    const int c = __popcll(m & ((1ull << w) - 1ull));
    const bool skip = n >= c;
    n -= skip ? c : 0;
    m >>= skip ? w : 0;
    pos += skip ? w : 0;
  }
  return pos;
}

// inclusive prefix sum across the wave, and the wave's total in every lane, in uint64
__device__ __forceinline__ uint64_t gsr_wave_scan_incl_u64(uint64_t v) {
  const int lane = gsr_lane();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t n = __shfl_up((unsigned long long)v, o, 64);
    if (lane >= o) v += n;
  }
  return v;
}

__device__ __forceinline__ uint64_t gsr_wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((unsigned long long)v, o, 64);
  return v;
}

// ---- Block-wide hand-offs: a value every wave has agreed on goes through a small LDS array to the whole block.
// The helpers own their array as a function-local __shared__, one per instantiation, so a kernel that calls a helper
// twice REUSES ONE ARRAY: a __syncthreads() must stand between the last read of one call's values and the publish of the
// next call.  The call site places that barrier (only gsr_block_scan_excl, whose reads end inside it, brings its own).
// None of them adds floating-point values: the association order of a float sum is part of the stage contracts
// ("Block-wide sums, ranks and scans"), so every site writes its sum as one visible expression.
// A caller that uses the wave index itself passes it as `wave`: a helper is simplified before it is inlined, and a
// second threadIdx.x >> 6 in here would be folded into the store's address apart from the caller's (other code).
template <typename T, int WAVES = 4>
using GsrWaves = T[WAVES];

// One value per wave -> the waves' values, readable by every thread.  Lane LANE of every wave publishes (0, or 63, where
// gsr_wave_sum_to_lane63 and the inclusive wave scans leave the wave's total), then the block's barrier.
template <int LANE = 0, int WAVES = 4, typename T>
__device__ __forceinline__ const GsrWaves<T, WAVES>& gsr_block_handoff(T v, int wave = threadIdx.x >> 6) {
  __shared__ T s_w[WAVES];
  if (gsr_lane() == LANE) s_w[wave] = v;
  __syncthreads();
  return s_w;
}

// Two values per wave under ONE barrier.
template <typename A, typename B, int WAVES>
struct GsrWavesPair {
  const GsrWaves<A, WAVES>& a;
  const GsrWaves<B, WAVES>& b;
};

template <int LANE = 0, int WAVES = 4, typename A, typename B>
__device__ __forceinline__ GsrWavesPair<A, B, WAVES> gsr_block_handoff(A a, B b, int wave = threadIdx.x >> 6) {
  __shared__ A s_a[WAVES];
  __shared__ B s_b[WAVES];
  if (gsr_lane() == LANE) { s_a[wave] = a; s_b[wave] = b; }
  __syncthreads();
  return {s_a, s_b};
}

// flag -> before: set flags in the threads below this one; total: set flags of the block.  256 threads.
struct GsrBlockRank {
  uint32_t before, total;
};

__device__ __forceinline__ GsrBlockRank gsr_block_rank(bool flag) {
  const uint64_t b = __ballot(flag);
  const int wave = threadIdx.x >> 6;
  const GsrWaves<uint32_t>& w = gsr_block_handoff((uint32_t)__builtin_popcountll(b), wave);
  GsrBlockRank r;
  r.before = (uint32_t)gsr_mbcnt(b);
  for (int i = 0; i < wave; ++i) r.before += w[i];
  r.total = w[0] + w[1] + w[2] + w[3];
  return r;
}

__device__ __forceinline__ uint32_t gsr_block_count(bool flag) {   // set flags of the block, in every thread
  const GsrWaves<uint32_t>& w = gsr_block_handoff((uint32_t)__builtin_popcountll(__ballot(flag)));
  return w[0] + w[1] + w[2] + w[3];
}

// Block-wide exclusive scan of one value per thread (256 threads); returns the exclusive prefix, the block's total in
// *total_out (the same in every thread).  Ends with a barrier: it may be called again at once.
__device__ __forceinline__ uint32_t gsr_block_scan_excl(uint32_t v, uint32_t* total_out) {
  const int wave = threadIdx.x >> 6;
  const uint32_t incl = gsr_wave_scan_incl_u32(v);
  const GsrWaves<uint32_t>& s_wave = gsr_block_handoff<63>(incl, wave);
  uint32_t base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t c = s_wave[w];
    if (w < wave) base += c;
    total += c;
  }
  __syncthreads();
  *total_out = total;
  return base + incl - v;
}

// The 16-lane form (256 threads = 16 DPP rows): lane 15 of every row stores its K values (row sums, from
// gsr_row_sum_to_lane15 of gsr_dpp_reduce.h), barrier; gsr_rows_sum adds column j over the rows in row order, from 0.
template <int K>
using GsrRows = float[16][K];

template <int K>
__device__ __forceinline__ const GsrRows<K>& gsr_block_rows_handoff(const float (&v)[K]) {
  __shared__ float s_rows[16][K];                 // 4 waves x 4 rows of 16 lanes
  const int lane = gsr_lane(), wave = threadIdx.x >> 6;
  if ((lane & 15) == 15) {
#pragma unroll
    for (int j = 0; j < K; ++j) s_rows[4 * wave + (lane >> 4)][j] = v[j];
  }
  __syncthreads();
  return s_rows;
}

template <int K>
__device__ __forceinline__ float gsr_rows_sum(const GsrRows<K>& rows, int j) {
  float a = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) a += rows[r][j];
  return a;
}

// Depth -> sortable u32 key.  The IEEE bit pattern of a positive float is monotone (sign bit set keeps negatives, which
// the cull never lets through, below); `bias` = key of the near plane makes the keys of a frame start at 0, so that
// they span only bits(far) - bits(near) (27 bits for 0.1 .. 100) and the radix sort needs fewer passes.  Depths outside
// [near, far] -- only possible for a caller-made depth tensor -- clamp to the ends (order among them: by index).
__device__ __forceinline__ uint32_t gsr_depth_key(float depth, uint32_t bias, uint32_t max_key) {
  const uint32_t b = __float_as_uint(depth);
  const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  const uint32_t rel = k > bias ? k - bias : 0u;
  return rel < max_key ? rel : max_key;
}

// Bijective remap of a linear block id so that the blocks dealt to one XCD (ids congruent mod 8 under the
// observed round-robin placement; speed only, never correctness) cover a contiguous range of work items.
__device__ __forceinline__ int gsr_xcd_remap(int bid, int n) {
  int q = n >> 3, r = n & 7;
  int xcd = bid & 7, within = bid >> 3;
  int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + within;
}

// Grouped variant for work lists whose length is only known on the device: runs of 2^log2_group consecutive items
// stay on one XCD (they share per-tile data in that XCD's L2) while the runs themselves are dealt round-robin, so every
// XCD still sees a uniform sample of the image.  Bijective on [0, 8 * 2^log2_group * k); the launch rounds its grid up
// to that multiple and blocks whose item falls past the end of the list return.
__device__ __forceinline__ uint32_t gsr_xcd_group_remap(uint32_t bid, uint32_t log2_group) {
  const uint32_t xcd = bid & 7u, within = bid >> 3;
  return ((((within >> log2_group) << 3) | xcd) << log2_group) | (within & ((1u << log2_group) - 1u));
}
