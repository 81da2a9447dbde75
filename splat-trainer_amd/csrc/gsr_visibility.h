// Per-pair maths of the frustum point queries and the fixed summation order of the per-cluster view features
// (visibility.hip).  Shared with the CPU unit-test shim (hostmath_shim.cpp), so the shim's results are the device's bit
// for bit.  Pure functions, no memory access beyond the arguments, no wave intrinsics.
//
// Camera record, 16 floats (one 64-byte line): rows 0..2 of image_t_world = expand_proj(K) @ camera_t_world, row-major
// (M[r][c] = rec[4 r + c]), then w, h, near, far.  For a point p, pinned (no contraction):
//   h_r = fmaf(M[r][2], p.z, fmaf(M[r][1], p.y, fmaf(M[r][0], p.x, M[r][3])))   r = 0, 1, 2;   d = h_2
//   inside = h_0 >= 0 && h_0 < w * d && h_1 >= 0 && h_1 < h * d && d > near && d < min(far, depth_below)
// which is the reference's test on (h_0 / d, h_1 / d) with the division multiplied out (equal in exact arithmetic for
// d > near >= 0).  Any NaN makes a comparison false: a NaN point is outside every camera.
//
// View features: value(vis) = vis > threshold ? vis : 0 (strict).  A cluster's members, in ascending point index, are
// cut at every multiple of GSR_VF_CHUNK of their position in the label-sorted order; each piece is summed left to right
// from its first element, the piece sums are dealt to 64 lanes (piece t to lane t mod 64, each lane adding in ascending t
// from 0.f), and the lanes are folded by the tree of gsr_wave_sum_to_lane63 (gsr_vf_tree64 is that tree for the host).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD

#define GSR_VIS_RECORD_FLOATS 16
#define GSR_VF_CHUNK 16

GSR_HD float gsr_vis_row(const float* m, float x, float y, float z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return fmaf(m[2], z, fmaf(m[1], y, fmaf(m[0], x, m[3])));
}

GSR_HD bool gsr_vis_inside(const float* rec, float x, float y, float z, float depth_below) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float h0 = gsr_vis_row(rec, x, y, z), h1 = gsr_vis_row(rec + 4, x, y, z), d = gsr_vis_row(rec + 8, x, y, z);
  const float w = rec[12], h = rec[13], near = rec[14], far = rec[15];
  return h0 >= 0.f && h0 < w * d && h1 >= 0.f && h1 < h * d && d > near && d < fminf(far, depth_below);
}

GSR_HD float gsr_vf_value(float vis, float threshold) { return vis > threshold ? vis : 0.f; }

#if !defined(__HIP_DEVICE_COMPILE__)
// Host mirror of gsr_wave_sum_to_lane63 (gsr_device.h): row_shr 1, 2, 4, 8 inside every row of 16 lanes (a lane without
// a source adds 0.f), then lane 15 into row 1 and lane 47 into row 3, then lane 31 into rows 2 and 3.  Returns lane 63.
inline float gsr_vf_tree64(const float* in) {
  float v[64], n[64];
  for (int i = 0; i < 64; ++i) v[i] = in[i];
  for (int k = 1; k <= 8; k <<= 1) {
    for (int i = 0; i < 64; ++i) n[i] = v[i] + ((i & 15) >= k ? v[i - k] : 0.f);
    for (int i = 0; i < 64; ++i) v[i] = n[i];
  }
  for (int i = 0; i < 64; ++i) n[i] = v[i] + (((i >> 4) & 1) ? v[(i & ~15) - 1] : 0.f);
  for (int i = 0; i < 64; ++i) v[i] = n[i];
  return v[63] + v[31];
}
#endif
