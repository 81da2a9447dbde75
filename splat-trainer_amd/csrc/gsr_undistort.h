// Arithmetic of the lens undistortion (undistort.hip), shared with the CPU shim (hostmath_shim.cpp).  Pure functions, no
// memory access.  The contract is in include/gsplat_hip.h under gsr_undistort_map and gsr_image_remap_u8.
//
// The map.  Pixel centres sit at integer coordinates.  The source camera is fx fy cx cy k1 k2 p1 p2 k3 (OpenCV's
// five-coefficient model), the target a pinhole fx' fy' cx' cy'.  Destination pixel (u, v) is taken to the target's
// normalised plane, distorted and projected with the source's intrinsics, in fp64, every product and sum rounded on its
// own in the order gsr_undistort_point writes them (no contraction: an fma would round once where the contract rounds
// twice).  1 / fx' and 1 / fy' are formed once on the host (gsr_lens_make), so a pixel costs no division.  The
// coordinate is clamped to [-1, S] (NaN -> -1) and quantised to 1/32 pixel, X = floor(32 x + 1/2): fp64 because at 1/32
// pixel of a 4000-pixel side a float's 24 bits leave 2^-7 of a step, and the quantised map is compared bit for bit.
//
// The remap.  An entry (X, Y) is clamped to [-32, 32 Ws] x [-32, 32 Hs], so any int32 is memory-safe.  x0 = X >> 5,
// ax = X & 31: taps x0 and x0 + 1 with weights 32 - ax and ax, likewise in y.  A tap outside the source, or one of
// weight 0, contributes 0; out = (sum of wy wx byte + 512) >> 10 <= 255.  All integer.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gsplat_hip.h"
#include "gsr_image.h"        // GSR_IMAGE_MAX_SIDE
#include "gsr_math.h"         // GSR_HD

struct GsrLens {
  double fx, fy, cx, cy, k1, k2, p1, p2, k3;     // the source camera
  double ifx, ify, cxt, cyt;                     // 1 / fx', 1 / fy', cx', cy' of the target
};

inline GsrLens gsr_lens_make(const double* source, const double* target) {      // host only
  GsrLens m;
  m.fx = source[0]; m.fy = source[1]; m.cx = source[2]; m.cy = source[3];
  m.k1 = source[4]; m.k2 = source[5]; m.p1 = source[6]; m.p2 = source[7]; m.k3 = source[8];
  m.ifx = 1.0 / target[0]; m.ify = 1.0 / target[1]; m.cxt = target[2]; m.cyt = target[3];
  return m;
}

// Source coordinates of destination pixel (u, v), unclamped.
GSR_HD void gsr_undistort_point(const GsrLens& m, double u, double v, double* xs_out, double* ys_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double x = (u - m.cxt) * m.ifx, y = (v - m.cyt) * m.ify;
  const double xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
  double t = r2 * m.k3;
  t = m.k2 + t;
  t = r2 * t;
  t = m.k1 + t;
  t = r2 * t;
  const double rad = 1.0 + t;
  double a = (2.0 * m.p1) * xy, b = 2.0 * xx;
  b = r2 + b;
  b = m.p2 * b;
  const double dx = a + b;
  a = 2.0 * yy;
  a = r2 + a;
  a = m.p1 * a;
  b = (2.0 * m.p2) * xy;
  const double dy = a + b;
  double xd = x * rad, yd = y * rad;
  xd = xd + dx;
  yd = yd + dy;
  double xs = m.fx * xd, ys = m.fy * yd;
  xs = xs + m.cx;
  ys = ys + m.cy;
  *xs_out = xs;
  *ys_out = ys;
}

// A source coordinate on an axis of S pixels -> units of 1/32 pixel: clamped to [-1, S], NaN -> -1.
GSR_HD int32_t gsr_undistort_quantise(double xs, int32_t S) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(xs >= -1.0)) xs = -1.0;
  if (xs > (double)S) xs = (double)S;
  return (int32_t)floor(xs * 32.0 + 0.5);
}

// One axis of a map entry: the two taps, each moved to the nearest pixel of the source (so that an address formed from
// it is valid) with the weight of a tap that lies outside set to 0.  S >= 1.
struct GsrRemapAxis {
  int32_t i0, i1;        // in 0 .. S - 1
  uint32_t w0, w1;       // 0 .. 32
};

GSR_HD GsrRemapAxis gsr_remap_axis(int32_t X, int32_t S) {
  const int32_t hi = 32 * S;
  X = X < -32 ? -32 : X > hi ? hi : X;
  const int32_t x0 = X >> 5, x1 = x0 + 1;      // -1 .. S, 0 .. S + 1
  const uint32_t a = (uint32_t)(X & 31);
  GsrRemapAxis t;
  t.w0 = x0 >= 0 && x0 < S ? 32u - a : 0u;
  t.w1 = x1 < S ? a : 0u;                      // x1 >= 0 always
  t.i0 = x0 < 0 ? 0 : x0 >= S ? S - 1 : x0;
  t.i1 = x1 >= S ? S - 1 : x1;
  return t;
}

GSR_HD uint32_t gsr_remap_round(uint32_t sum) { return (sum + 512u) >> 10; }      // sum <= 1024 * 255

// The argument checks of gsr_undistort_map, in the order the ABI states them.  *launch is 0 where GSR_OK means "nothing
// to do".
inline int gsr_undistort_map_check(const double* source, const double* target, int32_t Hs, int32_t Ws, int32_t Hd,
                                   int32_t Wd, const void* map_out, int* launch) {
  *launch = 0;
  if (Hs < 0 || Ws < 0 || Hd < 0 || Wd < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (Hs > GSR_IMAGE_MAX_SIDE || Ws > GSR_IMAGE_MAX_SIDE || Hd > GSR_IMAGE_MAX_SIDE || Wd > GSR_IMAGE_MAX_SIDE)
    return GSR_ERR_UNSUPPORTED;
  if (!source || !target) return GSR_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 9; ++k)
    if (!isfinite(source[k])) return GSR_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 4; ++k)
    if (!isfinite(target[k])) return GSR_ERR_INVALID_ARGUMENT;
  if (!(source[0] > 0.0) || !(source[1] > 0.0) || !(target[0] > 0.0) || !(target[1] > 0.0)) return GSR_ERR_INVALID_ARGUMENT;
  if (Hd == 0 || Wd == 0) return GSR_OK;
  if (!map_out) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

// The argument checks of gsr_image_remap_u8, likewise.  src is looked at only where the source has pixels.
inline int gsr_image_remap_check(const void* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, const void* map,
                                 const void* dst, int32_t Hd, int32_t Wd, int* launch) {
  *launch = 0;
  if (B < 0 || Hs < 0 || Ws < 0 || C < 0 || Hd < 0 || Wd < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (C != 1 && C != 3) return GSR_ERR_UNSUPPORTED;
  if (Hs > GSR_IMAGE_MAX_SIDE || Ws > GSR_IMAGE_MAX_SIDE || Hd > GSR_IMAGE_MAX_SIDE || Wd > GSR_IMAGE_MAX_SIDE)
    return GSR_ERR_UNSUPPORTED;
  if (B == 0 || Hd == 0 || Wd == 0) return GSR_OK;
  if (!map || !dst || (!src && Hs > 0 && Ws > 0)) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}
