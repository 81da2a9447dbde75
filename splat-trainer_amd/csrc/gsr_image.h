// Integer arithmetic of the area resize (image.hip), shared with the CPU shim (hostmath_shim.cpp).  Pure functions, no
// memory access, no floating point.
//
// One axis.  A source axis of S pixels and a destination axis of T <= S pixels are laid on S * T units: source pixel i
// covers [i T, (i + 1) T), destination pixel j covers [j S, (j + 1) S).  gsr_area_first / gsr_area_last are the first and
// the last source pixel that overlap destination pixel j, gsr_area_weight the length of an overlap (0 .. T); the weights
// of one j add up to S.  With S, T <= GSR_IMAGE_MAX_SIDE every product here is below 2^31.
//
// A pixel.  sum = sum_y sum_x wy wx src <= 255 D with D = Ws Hs <= 2^30, and the result is floor((2 sum + D) / (2 D)):
// the exact mean rounded half up.  The divisor is the same for a whole call, so the division is a multiplication by a
// host-made reciprocal and a shift (gsr_image_divisor, gsr_image_round_div).
//
// Why the multiply-shift is exact.  d = 2 D, n = 2 sum + D <= 511 D < 2^40.  Take l with 2^l >= d, s = 40 + l and
// m = ceil(2^s / d), so m d = 2^s + e with 0 <= e < d.  Then n m / 2^s = n / d + n e / (d 2^s), and the second term is
// below 2^40 d / (d 2^(40 + l)) = 2^-l <= 1 / d, while the fractional part of n / d is at most 1 - 1 / d: the floor
// does not move.  m < 2^41, so n m < 2^81 needs the 128-bit product.
#pragma once
#include <stdint.h>

#include "../../include/gsplat_hip.h"
#include "gsr_math.h"         // GSR_HD

#define GSR_IMAGE_MAX_SIDE 32768

GSR_HD int32_t gsr_area_first(int32_t j, int32_t S, int32_t T) { return (int32_t)(((uint32_t)j * (uint32_t)S) / (uint32_t)T); }

GSR_HD int32_t gsr_area_last(int32_t j, int32_t S, int32_t T) {
  return (int32_t)((((uint32_t)j + 1u) * (uint32_t)S - 1u) / (uint32_t)T);
}

GSR_HD uint32_t gsr_area_weight(int32_t j, int32_t i, int32_t S, int32_t T) {
  const uint32_t a0 = (uint32_t)i * (uint32_t)T, a1 = a0 + (uint32_t)T, b0 = (uint32_t)j * (uint32_t)S, b1 = b0 + (uint32_t)S;
  const uint32_t lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
  return hi > lo ? hi - lo : 0u;
}

struct GsrImageDivisor {
  uint64_t m;        // ceil(2^shift / (2 D))
  uint64_t D;        // Ws Hs
  int32_t shift;     // 40 + ceil(log2(2 D)): 41 .. 71
};

inline GsrImageDivisor gsr_image_divisor(int32_t Ws, int32_t Hs) {      // host only; Ws, Hs in 1 .. GSR_IMAGE_MAX_SIDE
  GsrImageDivisor dv;
  dv.D = (uint64_t)Ws * (uint64_t)Hs;
  const uint64_t d = 2 * dv.D;
  int l = 0;
  while (((uint64_t)1 << l) < d) ++l;
  dv.shift = 40 + l;
  const unsigned __int128 one = 1;
  dv.m = (uint64_t)((((one << dv.shift) - 1) / d) + 1);
  return dv;
}

// floor((2 sum + D) / (2 D)) for sum <= 255 D
GSR_HD uint32_t gsr_image_round_div(uint64_t sum, uint64_t m, uint64_t D, int32_t shift) {
  const uint64_t n = 2 * sum + D;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t hi = __umul64hi(n, m), lo = n * m;
#else
  const unsigned __int128 p = (unsigned __int128)n * m;
  const uint64_t hi = (uint64_t)(p >> 64), lo = (uint64_t)p;
#endif
  return (uint32_t)(shift >= 64 ? hi >> (shift - 64) : (hi << (64 - shift)) | (lo >> shift));
}

// The argument checks of gsr_image_resize_area_u8, in the order the ABI states them.  *launch is 0 where GSR_OK means
// "nothing to do".
inline int gsr_image_check(const void* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, const void* dst, int32_t Hd,
                           int32_t Wd, int* launch) {
  *launch = 0;
  if (B < 0 || Hs < 0 || Ws < 0 || C < 0 || Hd < 0 || Wd < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (C != 1 && C != 3) return GSR_ERR_UNSUPPORTED;
  if (Ws > GSR_IMAGE_MAX_SIDE || Hs > GSR_IMAGE_MAX_SIDE) return GSR_ERR_UNSUPPORTED;
  const bool empty_src = Hs == 0 || Ws == 0;
  if (Wd > Ws || Hd > Hs || (!empty_src && (Hd == 0 || Wd == 0))) return GSR_ERR_INVALID_ARGUMENT;
  if (B == 0 || empty_src) return GSR_OK;
  if (!src || !dst) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}
