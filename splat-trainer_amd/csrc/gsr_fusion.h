// Arithmetic of the depth-map fusion (fusion.hip), shared with the CPU shim (hostmath_shim.cpp).  Pure functions, no
// memory access.  The contract is in include/gsplat_hip.h under gsr_fuse_check, gsr_fuse_emit and gsr_voxel_downsample.
//
// Everything is fp64, every product and sum rounded on its own in the order written here (no contraction: an fma would
// round once where the contract rounds twice).  Pixel (row i, column j) has its centre at (j + 0.5, i + 0.5), the
// renderer's convention.  A depth is valid when it is above 0 and finite.
//
// Consistency of reference pixel (i, j) of depth d against one source:
//   x = ((j + 0.5) - cx) ifx, y = ((i + 0.5) - cy) ify, X = x d, Y = y d, Z = d        (ifx = 1 / fx formed by the host)
//   p_k = ((r_k0 X + r_k1 Y) + r_k2 Z) + t_k, k = 0, 1, 2                                (rel = rows of src_t_ref, 3 x 4)
//   !(p_2 > near): no vote.  iz = 1 / p_2 (the one division), us = fx_s (p_0 iz) + cx_s, vs likewise
//   us outside [0, Ws), vs outside [0, Hs) or NaN: no vote.  js = floor(us), is = floor(vs), ds = src[is, js]
//   ds not valid: no vote.  tol = rel_tol p_2, diff = ds - p_2: |diff| <= tol agrees, else diff > tol violates (the
//   source sees past the point), else the point is occluded and casts no vote.
//
// Voxel cell of a point p (fp32, widened), per axis: s = (p - origin) inv (inv = 1 / voxel formed by the host),
// q = floor(s) clamped to [-2^20, 2^20 - 1] (NaN -> -2^20), f = s - q clamped to [0, 1] (NaN -> 0),
// F = floor(f 2^20 + 0.5).  key = (qz + 2^20) << 42 | (qy + 2^20) << 21 | (qx + 2^20).  Per voxel of n points with
// S = sum F and C = sum of a colour byte, both int64: mean = (float)(origin + (q + (S / n) 2^-20) voxel) and
// colour = (2 C + n) / (2 n) in integer division.  Integer sums: any order of addition gives the same bits.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsplat_hip.h"
#include "gsr_image.h"        // GSR_IMAGE_MAX_SIDE
#include "gsr_math.h"         // GSR_HD

struct GsrFuseRef {
  double ifx, ify, cx, cy;
};

struct GsrFuseView {          // one source: 16 doubles as the ABI passes them
  double rel[12];
  double fx, fy, cx, cy;
};

struct GsrFuseSourceSet {     // what the check kernel takes by value
  const float* depth[GSR_FUSE_MAX_SOURCES];
  int32_t H[GSR_FUSE_MAX_SOURCES], W[GSR_FUSE_MAX_SOURCES];
  GsrFuseView view[GSR_FUSE_MAX_SOURCES];
  int32_t S;
};

GSR_HD bool gsr_fuse_valid(double d) { return d > 0.0 && d <= DBL_MAX; }

// The camera-space point of pixel (i, j) at depth d.
GSR_HD void gsr_fuse_unproject(const GsrFuseRef& r, int32_t i, int32_t j, double d, double* X, double* Y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double x = (double)j + 0.5, y = (double)i + 0.5;
  x = x - r.cx;
  y = y - r.cy;
  x = x * r.ifx;
  y = y * r.ify;
  *X = x * d;
  *Y = y * d;
}

// Row k of a 3 x 4 transform applied to (X, Y, Z).
GSR_HD double gsr_fuse_row(const double* m, double X, double Y, double Z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double a = m[0] * X, b = m[1] * Y, c = m[2] * Z;
  double s = a + b;
  s = s + c;
  return s + m[3];
}

// Where (X, Y, Z) of the reference falls in a source of Hs x Ws pixels: false for no vote, else the pixel and p_2.
GSR_HD bool gsr_fuse_project(const GsrFuseView& v, int32_t Hs, int32_t Ws, double near, double X, double Y, double Z,
                             int32_t* is, int32_t* js, double* depth) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double p0 = gsr_fuse_row(v.rel, X, Y, Z), p1 = gsr_fuse_row(v.rel + 4, X, Y, Z), p2 = gsr_fuse_row(v.rel + 8, X, Y, Z);
  if (!(p2 > near)) return false;
  const double iz = 1.0 / p2;
  double us = p0 * iz, vs = p1 * iz;
  us = v.fx * us;
  vs = v.fy * vs;
  us = us + v.cx;
  vs = vs + v.cy;
  if (!(us >= 0.0) || !(us < (double)Ws) || !(vs >= 0.0) || !(vs < (double)Hs)) return false;
  *js = (int32_t)us;          // 0 <= us < Ws: truncation is floor
  *is = (int32_t)vs;
  *depth = p2;
  return true;
}

#define GSR_FUSE_NONE 0
#define GSR_FUSE_AGREE 1
#define GSR_FUSE_VIOLATE 2

GSR_HD int gsr_fuse_vote(double ds, double p2, double rel_tol) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!gsr_fuse_valid(ds)) return GSR_FUSE_NONE;
  const double tol = rel_tol * p2, diff = ds - p2;
  if (fabs(diff) <= tol) return GSR_FUSE_AGREE;
  return diff > tol ? GSR_FUSE_VIOLATE : GSR_FUSE_NONE;
}

GSR_HD uint8_t gsr_fuse_saturate(uint32_t v) { return (uint8_t)(v > 255u ? 255u : v); }

GSR_HD bool gsr_fuse_keep(double d, uint32_t agree, uint32_t violate, int32_t min_agree, int32_t max_violate) {
  return gsr_fuse_valid(d) && (int32_t)agree >= min_agree && (int32_t)violate <= max_violate;
}

// floor(clamp(c, 0, 1) 255 + 0.5); NaN -> 0.
GSR_HD uint8_t gsr_fuse_colour(float c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double v = (double)c;
  if (!(v >= 0.0)) v = 0.0;
  if (v > 1.0) v = 1.0;
  v = v * 255.0;
  v = v + 0.5;
  return (uint8_t)floor(v);
}

// ---- voxel grid ----
#define GSR_VOXEL_HALF 1048576      // 2^20 cells each way

struct GsrVoxelGrid {
  double voxel, inv, origin[3];
};

inline GsrVoxelGrid gsr_voxel_grid_make(const double* grid) {      // host only: grid = voxel, ox, oy, oz
  GsrVoxelGrid g;
  g.voxel = grid[0];
  g.inv = 1.0 / grid[0];
  g.origin[0] = grid[1]; g.origin[1] = grid[2]; g.origin[2] = grid[3];
  return g;
}

// One axis: the cell q and the offset inside it in units of 2^-20 cell.
GSR_HD void gsr_voxel_axis(float p, double origin, double inv, int32_t* q, int64_t* F) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double s = (double)p - origin;
  s = s * inv;
  double qd = floor(s);
  if (!(qd >= -(double)GSR_VOXEL_HALF)) qd = -(double)GSR_VOXEL_HALF;
  if (qd > (double)(GSR_VOXEL_HALF - 1)) qd = (double)(GSR_VOXEL_HALF - 1);
  double f = s - qd;
  if (!(f >= 0.0)) f = 0.0;
  if (f > 1.0) f = 1.0;
  f = f * 1048576.0;
  f = f + 0.5;
  *q = (int32_t)qd;
  *F = (int64_t)floor(f);
}

GSR_HD uint64_t gsr_voxel_key(int32_t qx, int32_t qy, int32_t qz) {
  return ((uint64_t)(uint32_t)(qz + GSR_VOXEL_HALF) << 42) | ((uint64_t)(uint32_t)(qy + GSR_VOXEL_HALF) << 21) |
         (uint64_t)(uint32_t)(qx + GSR_VOXEL_HALF);
}

GSR_HD uint64_t gsr_voxel_key_of(const GsrVoxelGrid& g, const float* p) {
  int32_t q[3];
  int64_t F;
  gsr_voxel_axis(p[0], g.origin[0], g.inv, &q[0], &F);
  gsr_voxel_axis(p[1], g.origin[1], g.inv, &q[1], &F);
  gsr_voxel_axis(p[2], g.origin[2], g.inv, &q[2], &F);
  return gsr_voxel_key(q[0], q[1], q[2]);
}

GSR_HD int32_t gsr_voxel_key_axis(uint64_t key, int a) { return (int32_t)((key >> (21 * a)) & 0x1fffffu) - GSR_VOXEL_HALF; }

// The mean coordinate of a voxel's n points on one axis from the integer sum S of their offsets.
GSR_HD float gsr_voxel_mean(double origin, double voxel, int32_t q, int64_t S, int64_t n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double m = (double)S / (double)n;
  m = m * (1.0 / 1048576.0);
  m = (double)q + m;
  m = m * voxel;
  m = origin + m;
  return (float)m;
}

GSR_HD uint8_t gsr_voxel_colour(int64_t C, int64_t n) { return (uint8_t)((2 * C + n) / (2 * n)); }      // round half up

// ---- the argument checks, in the order the ABI states them.  *launch is 0 where GSR_OK means "nothing to do". ----
inline bool gsr_fuse_finite(const double* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!isfinite(v[k])) return false;
  return true;
}

inline int gsr_fuse_check_args(const void* ref_depth, int32_t Hr, int32_t Wr, const double* ref_intrinsics,
                               const GsrFuseSource* sources, const double* source_params, int32_t S,
                               const double* tolerances, const void* counts, int* launch) {
  *launch = 0;
  if (Hr < 0 || Wr < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (Hr > GSR_IMAGE_MAX_SIDE || Wr > GSR_IMAGE_MAX_SIDE) return GSR_ERR_UNSUPPORTED;
  if (S < 1 || S > GSR_FUSE_MAX_SOURCES) return GSR_ERR_INVALID_ARGUMENT;
  if (!ref_intrinsics || !sources || !source_params || !tolerances) return GSR_ERR_INVALID_ARGUMENT;
  if (!gsr_fuse_finite(ref_intrinsics, 4) || !gsr_fuse_finite(source_params, 16 * S) || !gsr_fuse_finite(tolerances, 2) ||
      !(tolerances[1] >= 0.0))
    return GSR_ERR_INVALID_ARGUMENT;
  for (int s = 0; s < S; ++s) {
    if (sources[s].H < 0 || sources[s].W < 0) return GSR_ERR_INVALID_ARGUMENT;
    if (sources[s].H > GSR_IMAGE_MAX_SIDE || sources[s].W > GSR_IMAGE_MAX_SIDE) return GSR_ERR_UNSUPPORTED;
  }
  if (Hr == 0 || Wr == 0) return GSR_OK;
  if (!ref_depth || !counts) return GSR_ERR_INVALID_ARGUMENT;
  for (int s = 0; s < S; ++s)
    if (!sources[s].depth && sources[s].H > 0 && sources[s].W > 0) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

inline int gsr_fuse_mask_args(const void* ref_depth, const void* counts, int32_t Hr, int32_t Wr, int32_t min_agree,
                              int32_t max_violate, const void* keep_out, int* launch) {
  *launch = 0;
  if (Hr < 0 || Wr < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (Hr > GSR_IMAGE_MAX_SIDE || Wr > GSR_IMAGE_MAX_SIDE) return GSR_ERR_UNSUPPORTED;
  if (min_agree < 0 || min_agree > 255 || max_violate < 0 || max_violate > 255) return GSR_ERR_INVALID_ARGUMENT;
  if (Hr == 0 || Wr == 0) return GSR_OK;
  if (!ref_depth || !counts || !keep_out) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

inline int gsr_fuse_emit_args(const void* ref_depth, const void* counts, int32_t Hr, int32_t Wr,
                              const double* ref_intrinsics, const double* world_t_ref, int32_t min_agree,
                              int32_t max_violate, const void* block_offsets, int64_t base, int64_t capacity,
                              const void* points_out, const void* colors_out, const void* agree_out, int* launch) {
  *launch = 0;
  if (Hr < 0 || Wr < 0 || base < 0 || capacity < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (Hr > GSR_IMAGE_MAX_SIDE || Wr > GSR_IMAGE_MAX_SIDE) return GSR_ERR_UNSUPPORTED;
  if (min_agree < 0 || min_agree > 255 || max_violate < 0 || max_violate > 255) return GSR_ERR_INVALID_ARGUMENT;
  if (!ref_intrinsics || !world_t_ref) return GSR_ERR_INVALID_ARGUMENT;
  if (!gsr_fuse_finite(ref_intrinsics, 4) || !gsr_fuse_finite(world_t_ref, 12)) return GSR_ERR_INVALID_ARGUMENT;
  if (Hr == 0 || Wr == 0 || base >= capacity) return GSR_OK;
  if (!ref_depth || !counts || !block_offsets || !points_out || !colors_out || !agree_out) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

inline int gsr_voxel_args(const void* points, const void* colors, int64_t N, const double* grid, const void* points_out,
                          const void* colors_out, const void* counts_out, const void* K_dev, int* launch) {
  *launch = 0;
  if (N < 0 || N > 0x7fffffffll) return GSR_ERR_INVALID_ARGUMENT;
  if (!grid || !gsr_fuse_finite(grid, 4) || !(grid[0] > 0.0) || !isfinite(1.0 / grid[0])) return GSR_ERR_INVALID_ARGUMENT;
  if (N == 0) return GSR_OK;                 // nothing is written, K_dev included
  if (!points || !colors || !points_out || !colors_out || !counts_out || !K_dev) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}
