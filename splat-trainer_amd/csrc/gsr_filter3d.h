// Per-pair maths of the sampling-rate pass and per-row maths of the 3-D smoothing filter (filter3d.hip): the other half
// of Mip-Splatting's anti-aliasing (Yu et al., CVPR 2024, section 5.1; the 2-D half is RasterConfig.antialias in
// gsr_math.h).  Shared with the CPU unit-test shim (hostmath_shim.cpp).  Pure functions, no memory access beyond the
// arguments, no wave intrinsics, no contraction.
//
// Sampling rate.  Camera record and h_r, d = h_2 as in gsr_visibility.h; f the camera's focal max(fx, fy) in pixels; m >= 0
// the margin fraction.  Camera c samples p when
//   h_0 >= (-m w) d && h_0 < (w + m w) d && h_1 >= (-m h) d && h_1 < (h + m h) d && d > near && d < far
// (w + m w = fmaf(m, w, w); the four bracketed factors depend on the camera alone).  rate[p] = max over the sampling
// cameras of f / d, 0 when there is none.  The maximum is kept as a pair (f_b, d_b), starting at (0, 1), and camera c
// replaces it when f_c d_b > f_b d_c -- the comparison of the two quotients multiplied out, both d > 0 -- so a tie keeps
// the earlier camera; the one division f_b / d_b is made at the end.  Any NaN makes a comparison false: a NaN point is
// sampled by no camera and keeps rate 0.
//
// Smoothing.  c = strength / rate^2 (0 when rate is not > 0) is the variance added on every axis, in world units:
// sigma'_j = sqrt(sigma_j^2 + c), opacity' = opacity prod_j sigma_j / sigma'_j, on the parameterisation the rest of the path
// reads (log_scaling, alpha_logit), in the form that does not cancel:
//   u_j = c exp(-2 ls_j)    l_j = log1p(u_j)    ls'_j = ls_j + l_j / 2    lc = -(l_0 + l_1 + l_2) / 2   (log of the coefficient)
//   e = exp(-|a|)   s+ = sigmoid(a), s- = sigmoid(-a) from 1 / (1 + e) and e / (1 + e)   log s+ = min(a, 0) - log1p(e)
//   D = s- + s+ (-expm1(lc))   (= 1 - s+ exp(lc), without the cancellation)          a' = (log s+ + lc) - log(D)
// and backward, recomputing the same terms (the rate receives no gradient):
//   d ls_j = g_ls'_j / (1 + u_j) + g_a' (u_j / (1 + u_j)) / D          d a = g_a' s- / D
// A row with c == 0 is not touched by any of this: the kernels copy its inputs (its incoming gradients) bit for bit.
// Meant for ls in [-8, 8] (the scene's clamp) and c <= 1e2, where u stays below 1e9; an infinite u gives NaN gradients.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"         // GSR_HD
#include "gsr_visibility.h"   // gsr_vis_row, GSR_VIS_RECORD_FLOATS

// Folds camera (rec, f) into the running best pair (bf, bd) of the point (x, y, z).
GSR_HD void gsr_f3d_pair(const float* rec, float f, float margin, float x, float y, float z, float* bf, float* bd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float w = rec[12], h = rec[13], near = rec[14], far = rec[15];
  const float lo_w = -margin * w, hi_w = fmaf(margin, w, w), lo_h = -margin * h, hi_h = fmaf(margin, h, h);
  const float h0 = gsr_vis_row(rec, x, y, z), h1 = gsr_vis_row(rec + 4, x, y, z), d = gsr_vis_row(rec + 8, x, y, z);
  const bool in = h0 >= lo_w * d && h0 < hi_w * d && h1 >= lo_h * d && h1 < hi_h * d && d > near && d < far;
  const bool better = in && f * *bd > *bf * d;
  *bf = better ? f : *bf;
  *bd = better ? d : *bd;
}

GSR_HD float gsr_f3d_rate(float bf, float bd) { return bf / bd; }

GSR_HD float gsr_f3d_variance(float rate, float strength) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return rate > 0.f ? strength / (rate * rate) : 0.f;
}

struct GsrF3dTerms {
  float u[3], l[3];   // c exp(-2 ls_j) and its log1p
  float lc;           // log of the opacity coefficient
  float sp, sn;       // sigmoid(a), sigmoid(-a)
  float log_sp;       // log sigmoid(a)
  float D;            // 1 - sigmoid(a) exp(lc)
};

GSR_HD GsrF3dTerms gsr_f3d_terms(const float* ls, float a, float c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  GsrF3dTerms t;
  for (int j = 0; j < 3; ++j) {
    t.u[j] = c * expf(-2.f * ls[j]);
    t.l[j] = log1pf(t.u[j]);
  }
  t.lc = -0.5f * ((t.l[0] + t.l[1]) + t.l[2]);
  const float e = expf(-fabsf(a)), r = 1.f / (1.f + e);
  const float big = r, small = e * r;
  t.sp = a >= 0.f ? big : small;
  t.sn = a >= 0.f ? small : big;
  t.log_sp = fminf(a, 0.f) - log1pf(e);
  t.D = t.sn + t.sp * -expm1f(t.lc);
  return t;
}

// out_ls[3] and *out_a of one row with c != 0.
GSR_HD void gsr_f3d_forward_row(const float* ls, float a, float c, float* out_ls, float* out_a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const GsrF3dTerms t = gsr_f3d_terms(ls, a, c);
  for (int j = 0; j < 3; ++j) out_ls[j] = ls[j] + 0.5f * t.l[j];
  *out_a = (t.log_sp + t.lc) - logf(t.D);
}

// d_ls[3] and *d_a of one row with c != 0 from the gradients g_ls[3], g_a of its outputs.
GSR_HD void gsr_f3d_backward_row(const float* ls, float a, float c, const float* g_ls, float g_a, float* d_ls, float* d_a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const GsrF3dTerms t = gsr_f3d_terms(ls, a, c);
  for (int j = 0; j < 3; ++j) {
    const float k = 1.f + t.u[j];
    d_ls[j] = g_ls[j] / k + g_a * ((t.u[j] / k) / t.D);
  }
  *d_a = g_a * (t.sn / t.D);
}
