// Normal consistency (normals.hip): camera-space splat normals, normals of a depth image and the depth-normal
// consistency loss of 2DGS (Huang et al., SIGGRAPH 2024, section 4.2) / GOF.  This text is the statement of record;
// tests/normals_oracle.py restates it in fp64.  fp32 throughout, pixel (column u, row v) has its centre at
// (u + 0.5, v + 0.5), the camera is CameraParams' OpenCV pinhole: projection = fx fy cx cy, T_camera_world row-major
// 4 x 4 with rotation R_cw and translation t.  Pure functions: no memory access beyond the arguments, no wave intrinsics.
//
// Splat normal of visible row i = indexes[m].
//   q^ = rotation[i] / |rotation[i]| (xyzw), R its rotation matrix (the oracle's quat_to_rotmat_xyzw)
//   k  = the index of the smallest log_scaling[i, :], the lowest index on ties       (the splat's thinnest axis)
//   n  = R_cw R[:, k],  p = R_cw position[i] + t,  n = -n where n . p > 0            (towards the camera)
// Backward: d_rotation[i] alone, through the normalisation; k and the flip are constants of the row, and position,
// log_scaling and T_camera_world receive no gradient.
//
// Depth normal of a depth image d [H, W].
//   ray(u, v) = ((u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy, 1),  P = ray d
//   a = P(u+1, v) - P(u-1, v),  b = P(u, v+1) - P(u, v-1),  c = b x a,  n_d = c / |c|
// The differences of P are formed first, the products of the cross product after them.  A fronto-parallel surface gets
// (0, 0, -1).  The pixel is valid when it is interior (1 <= u <= W - 2, 1 <= v <= H - 2), its own depth and its four
// taps' depths are finite and > 0, and |c| > 0; otherwise n_d = (0, 0, 0) exactly.
//
// Loss on a geometry image G [H, W, 5] = N^x N^y N^z D A: the composite of the per-splat rows [n, depth, 1], so A is
// the accumulated alpha, D / A the expected depth and N^ the alpha-weighted normal (not normalised, as in 2DGS).
//   d = D / A where A >= alpha_min, else 0 (not valid);  n_d as above on d
//   l = A - N^ . n_d on valid pixels, 0 elsewhere;  L = sum l / (H W)
// Backward, with g = dL / (H W): on a valid pixel q
//   dL/dN^ = -g n_d,  dL/dA = g,  w = -g (N^ - (N^ . n_d) n_d) / |c|  (= dL/dc),  U = w x b_q (= dL/da),  V = a_q x w (= dL/db)
// and a pixel p receives through its depth, as a tap of its four neighbours' stencils, added in this order,
//   gd = ((ray(p) . U(p - x) - ray(p) . U(p + x)) + ray(p) . V(p - y)) - ray(p) . V(p + y)       (0 from a q that is not valid)
//   dD(p) = gd / A,  dA(p) += -dD(p) d(p)          where gd != 0 (then A >= alpha_min), else nothing.
// The projection receives no gradient.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"         // GSR_HD

// ---- splat normals ---------------------------------------------------------------------------------------------------
GSR_HD int gsr_nrm_thin_axis(const float* ls) {
  int k = 0;
  if (ls[1] < ls[k]) k = 1;
  if (ls[2] < ls[k]) k = 2;
  return k;
}

// Column k of the rotation matrix of the unit quaternion (x, y, z, w).
GSR_HD void gsr_nrm_column(float x, float y, float z, float w, int k, float* col) {
  if (k == 0) {
    col[0] = 1.f - 2.f * (y * y + z * z); col[1] = 2.f * (x * y + w * z); col[2] = 2.f * (x * z - w * y);
  } else if (k == 1) {
    col[0] = 2.f * (x * y - w * z); col[1] = 1.f - 2.f * (x * x + z * z); col[2] = 2.f * (y * z + w * x);
  } else {
    col[0] = 2.f * (x * z + w * y); col[1] = 2.f * (y * z - w * x); col[2] = 1.f - 2.f * (x * x + y * y);
  }
}

// g (3, the gradient of the column) -> gq (4, the gradient of the unit quaternion).
GSR_HD void gsr_nrm_column_backward(float x, float y, float z, float w, int k, const float* g, float* gq) {
  if (k == 0) {
    gq[0] = 2.f * (y * g[1] + z * g[2]);
    gq[1] = 2.f * (x * g[1] - w * g[2]) - 4.f * y * g[0];
    gq[2] = 2.f * (w * g[1] + x * g[2]) - 4.f * z * g[0];
    gq[3] = 2.f * (z * g[1] - y * g[2]);
  } else if (k == 1) {
    gq[0] = 2.f * (y * g[0] + w * g[2]) - 4.f * x * g[1];
    gq[1] = 2.f * (x * g[0] + z * g[2]);
    gq[2] = 2.f * (y * g[2] - w * g[0]) - 4.f * z * g[1];
    gq[3] = 2.f * (x * g[2] - z * g[0]);
  } else {
    gq[0] = 2.f * (z * g[0] - w * g[1]) - 4.f * x * g[2];
    gq[1] = 2.f * (w * g[0] + z * g[1]) - 4.f * y * g[2];
    gq[2] = 2.f * (x * g[0] + y * g[1]);
    gq[3] = 2.f * (y * g[0] - x * g[1]);
  }
}

// R_cw v of the row-major 4 x 4 T; with `translate` R_cw v + t.
GSR_HD void gsr_nrm_to_camera(const float* T, const float* v, bool translate, float* out) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 3; ++r)
    out[r] = (T[4 * r] * v[0] + T[4 * r + 1] * v[1]) + T[4 * r + 2] * v[2] + (translate ? T[4 * r + 3] : 0.f);
}

struct GsrSplatNormal {
  float q[4];        // the unit quaternion
  float inv_norm;    // 1 / |rotation|
  int k;             // the thin axis
  float sign;        // -1 where the normal was flipped
  float n[3];
};

GSR_HD GsrSplatNormal gsr_nrm_splat(const float* rot, const float* ls, const float* pos, const float* T) {
  GsrSplatNormal s;
  s.inv_norm = 1.f / sqrtf((rot[0] * rot[0] + rot[1] * rot[1]) + (rot[2] * rot[2] + rot[3] * rot[3]));
  for (int j = 0; j < 4; ++j) s.q[j] = rot[j] * s.inv_norm;
  s.k = gsr_nrm_thin_axis(ls);
  float col[3], p[3];
  gsr_nrm_column(s.q[0], s.q[1], s.q[2], s.q[3], s.k, col);
  gsr_nrm_to_camera(T, col, false, s.n);
  gsr_nrm_to_camera(T, pos, true, p);
  s.sign = (s.n[0] * p[0] + s.n[1] * p[1]) + s.n[2] * p[2] > 0.f ? -1.f : 1.f;
  for (int j = 0; j < 3; ++j) s.n[j] *= s.sign;
  return s;
}

// g_n (3) -> d_rotation (4) of the row the forward's `s` was made of.
GSR_HD void gsr_nrm_splat_backward(const GsrSplatNormal& s, const float* T, const float* g_n, float* d_rot) {
  float g_col[3], gq[4];
  for (int c = 0; c < 3; ++c) g_col[c] = s.sign * ((T[c] * g_n[0] + T[4 + c] * g_n[1]) + T[8 + c] * g_n[2]);   // R_cw^T g
  gsr_nrm_column_backward(s.q[0], s.q[1], s.q[2], s.q[3], s.k, g_col, gq);
  const float along = (s.q[0] * gq[0] + s.q[1] * gq[1]) + (s.q[2] * gq[2] + s.q[3] * gq[3]);
  for (int j = 0; j < 4; ++j) d_rot[j] = (gq[j] - s.q[j] * along) * s.inv_norm;
}

// ---- depth normals ---------------------------------------------------------------------------------------------------
GSR_HD float gsr_nrm_ray(float f, float c, int u) { return ((float)u + 0.5f - c) / f; }

GSR_HD bool gsr_nrm_depth_ok(float d) { return d > 0.f && d < INFINITY; }     // a NaN fails both

// The expected depth of a geometry pixel: D / A where A >= alpha_min, else 0.
GSR_HD float gsr_nrm_expected_depth(float D, float A, float alpha_min) { return A >= alpha_min ? D / A : 0.f; }

struct GsrNrmStencil {
  float a[3], b[3];   // the two differences of P
  float n[3];         // c / |c|, or 0
  float len;          // |c|
  bool valid;
};

// The stencil of pixel (u, v) whose depth is dc and whose taps' depths are dl, dr (u -+ 1) and du, dd (v -+ 1): the
// caller has established that the pixel is interior.  rx* / ry* are the rays' x at u - 1, u, u + 1 and y at v - 1, v, v + 1.
GSR_HD GsrNrmStencil gsr_nrm_stencil(float rxl, float rxc, float rxr, float ryu, float ryc, float ryd, float dc, float dl,
                                     float dr, float du, float dd) {
  GsrNrmStencil s;
  s.valid = gsr_nrm_depth_ok(dc) && gsr_nrm_depth_ok(dl) && gsr_nrm_depth_ok(dr) && gsr_nrm_depth_ok(du) &&
            gsr_nrm_depth_ok(dd);
  s.a[0] = rxr * dr - rxl * dl; s.a[1] = ryc * dr - ryc * dl; s.a[2] = dr - dl;
  s.b[0] = rxc * dd - rxc * du; s.b[1] = ryd * dd - ryu * du; s.b[2] = dd - du;
  const float c0 = s.b[1] * s.a[2] - s.b[2] * s.a[1], c1 = s.b[2] * s.a[0] - s.b[0] * s.a[2],
              c2 = s.b[0] * s.a[1] - s.b[1] * s.a[0];
  s.len = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
  s.valid = s.valid && s.len > 0.f;
  s.n[0] = s.valid ? c0 / s.len : 0.f;
  s.n[1] = s.valid ? c1 / s.len : 0.f;
  s.n[2] = s.valid ? c2 / s.len : 0.f;
  return s;
}

// l of a valid pixel.
GSR_HD float gsr_nrm_pixel_loss(const float* N, float A, const float* n) {
  return A - ((N[0] * n[0] + N[1] * n[1]) + N[2] * n[2]);
}

// U = g (w x b) and V = g (a x w) of a valid stencil: what its four taps read in the backward.
GSR_HD void gsr_nrm_stencil_backward(const GsrNrmStencil& s, const float* N, float g, float* U, float* V) {
  const float along = (N[0] * s.n[0] + N[1] * s.n[1]) + N[2] * s.n[2];
  const float scale = -g / s.len;
  const float w0 = (N[0] - along * s.n[0]) * scale, w1 = (N[1] - along * s.n[1]) * scale,
              w2 = (N[2] - along * s.n[2]) * scale;
  U[0] = w1 * s.b[2] - w2 * s.b[1]; U[1] = w2 * s.b[0] - w0 * s.b[2]; U[2] = w0 * s.b[1] - w1 * s.b[0];
  V[0] = s.a[1] * w2 - s.a[2] * w1; V[1] = s.a[2] * w0 - s.a[0] * w2; V[2] = s.a[0] * w1 - s.a[1] * w0;
}
