// Per-pixel maths of the bilateral-grid colour correction (bilagrid.hip), shared with the CPU unit-test shim
// (hostmath_shim.cpp).  Pure functions, no memory access beyond the arguments, no wave intrinsics.
//
// Grid G [N, 12, L, GH, GW] (float32), one per image.  Pixel (row i, col j) of an H x W image samples grid k at
//   x = (j + 0.5) / W * (GW - 1),  y = (i + 0.5) / H * (GH - 1),  z = luma(r, g, b) * (L - 1), zc = clamp(z, 0, L - 1)
// trilinearly (F.grid_sample, align_corners=True, border padding), giving the 3x4 affine A[12]; out[m] = A[4m..4m+2] .
// rgb + A[4m+3].  x and y never leave the grid, so a pixel lies in the xy cell (cx, cy) = (floor x, floor y), and its 8
// corners are the cell's 4 corner columns at levels z0 and z0 + 1.  The kernels stage those columns as cols[4][L][12]
// (q = 2 dy + dx, then level, then channel) and every function here reads that layout.
//
// Rounding is pinned (explicit fmaf, no contraction): the device and the host shim give the same bits, and a constant
// grid reproduces itself exactly (lerp(t, a, a) = fma(t, 0, a) = a), so an identity grid returns the input image bit for
// bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD

#define GSR_BG_CH 12

// BT.601 luma, the guidance of the reference's BilateralGrid
GSR_HD float gsr_bg_luma(float r, float g, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return fmaf(0.114f, b, fmaf(0.587f, g, 0.299f * r));
}

// Cell of pixel j along an axis of n pixels and G grid vertices: floor((2j + 1)(G - 1) / 2n), in integers (exact, at most
// G - 2 because 2j + 1 < 2n).  Its fraction inside the cell is formed from the exact integer remainder.
GSR_HD int gsr_bg_cell(int j, int n, int G) { return ((2 * j + 1) * (G - 1)) / (2 * n); }

GSR_HD float gsr_bg_frac(int j, int cell, int n, int G, float inv_2n) {
  return (float)((2 * j + 1) * (G - 1) - 2 * n * cell) * inv_2n;
}

// First pixel of cell c: the smallest j with (2j + 1)(G - 1) >= 2 n c.  Cell c holds [gsr_bg_first(c), gsr_bg_first(c + 1))
// (the last cell ends at n); a cell narrower than a pixel can be empty.
GSR_HD int gsr_bg_first(int c, int n, int G) {
  if (c >= G - 1) return n;
  const int num = 2 * n * c - (G - 1);
  return num <= 0 ? 0 : (num + 2 * (G - 1) - 1) / (2 * (G - 1));
}

struct GsrBgZ {
  int z0;        // lower level, 0..L-2
  float tz;      // zc - z0 in [0, 1]
  bool inside;   // 0 < z < L - 1: where the guidance gradient is nonzero (grid_sample's border-padding convention)
};

GSR_HD GsrBgZ gsr_bg_z(float lum, int L) {
  GsrBgZ r;
  const float top = (float)(L - 1);
  const float z = lum * top;
  const float zc = fminf(fmaxf(z, 0.f), top);    // NaN -> 0
  int z0 = (int)floorf(zc);
  if (z0 > L - 2) z0 = L - 2;
  r.z0 = z0;
  r.tz = zc - (float)z0;
  r.inside = z > 0.f && z < top;
  return r;
}

GSR_HD float gsr_bg_lerp(float t, float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return fmaf(t, b - a, a);
}

// bilinear value of channel c at level l: x first, then y
GSR_HD float gsr_bg_bilerp(const float* cols, int L, int l, int c, float tx, float ty) {
  const int s = L * GSR_BG_CH;
  const float* p = cols + l * GSR_BG_CH + c;
  return gsr_bg_lerp(ty, gsr_bg_lerp(tx, p[0], p[s]), gsr_bg_lerp(tx, p[2 * s], p[3 * s]));
}

// out[m] = A[4m] r + A[4m+1] g + A[4m+2] b + A[4m+3]
GSR_HD float gsr_bg_row(const float* A, float r, float g, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return fmaf(A[0], r, fmaf(A[1], g, fmaf(A[2], b, A[3])));
}

GSR_HD void gsr_bg_pixel_fwd(const float* cols, int L, float tx, float ty, float r, float g, float b, float out[3]) {
  const GsrBgZ z = gsr_bg_z(gsr_bg_luma(r, g, b), L);
  float A[GSR_BG_CH];
#pragma unroll
  for (int c = 0; c < GSR_BG_CH; ++c)
    A[c] = gsr_bg_lerp(z.tz, gsr_bg_bilerp(cols, L, z.z0, c, tx, ty), gsr_bg_bilerp(cols, L, z.z0 + 1, c, tx, ty));
#pragma unroll
  for (int m = 0; m < 3; ++m) out[m] = gsr_bg_row(A + 4 * m, r, g, b);
}

// dL/drgb of one pixel from go = dL/dout: sum_m A[4m+n] go[m], plus the guidance term
// (L - 1) luma_w[n] sum_m go[m] (D[4m] r + D[4m+1] g + D[4m+2] b + D[4m+3]), D = (level z0 + 1) - (level z0) = dA/dzc,
// where 0 < z < L - 1 only.
GSR_HD void gsr_bg_pixel_bwd_rgb(const float* cols, int L, float tx, float ty, float r, float g, float b,
                                 const float go[3], float d_rgb[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const GsrBgZ z = gsr_bg_z(gsr_bg_luma(r, g, b), L);
  float A[GSR_BG_CH], D[GSR_BG_CH];
#pragma unroll
  for (int c = 0; c < GSR_BG_CH; ++c) {
    const float p0 = gsr_bg_bilerp(cols, L, z.z0, c, tx, ty), p1 = gsr_bg_bilerp(cols, L, z.z0 + 1, c, tx, ty);
    A[c] = gsr_bg_lerp(z.tz, p0, p1);
    D[c] = p1 - p0;
  }
  float dz = 0.f;
  if (z.inside) {
    dz = fmaf(go[2], gsr_bg_row(D + 8, r, g, b), fmaf(go[1], gsr_bg_row(D + 4, r, g, b), go[0] * gsr_bg_row(D, r, g, b)));
    dz *= (float)(L - 1);
  }
  const float lw[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
  for (int n = 0; n < 3; ++n)
    d_rgb[n] = fmaf(lw[n], dz, fmaf(A[8 + n], go[2], fmaf(A[4 + n], go[1], A[n] * go[0])));
}

// Weight of corner (q, level z0 + k) in the pixel's sample: wz[k] * wxy[q], wz = (1 - tz, tz),
// wxy = ((1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty).  dL/dG[4m+n] at that corner = weight * go[m] * (r, g, b, 1)[n].
GSR_HD void gsr_bg_xy_weights(float tx, float ty, float wxy[4]) {
  wxy[0] = (1.f - tx) * (1.f - ty);
  wxy[1] = tx * (1.f - ty);
  wxy[2] = (1.f - tx) * ty;
  wxy[3] = tx * ty;
}
