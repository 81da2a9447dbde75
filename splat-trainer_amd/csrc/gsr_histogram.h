// Per-entry maths of the histogram kernels (histogram.hip), shared with the CPU unit-test shim (hostmath_shim.cpp).
// Pure functions, no memory access beyond the arguments, no wave intrinsics, float32 throughout, no contraction.
//
// Entry.  x = v, or v / (eps + w) when the row has a weight w.  A non-finite x is GSR_HIST_NONFINITE in every mode.
//   mode 0  t = x
//   mode 1  x > min_value is kept with t = log10f(x); every other x is GSR_HIST_DROPPED
//   mode 2  t = log10f(fmaxf(x, min_value))
// and a t that is not finite (mode 2 with x <= 0 and min_value <= 0) is GSR_HIST_NONFINITE too.
//
// Bin.  hi == lo: bin 0, never outside.  Otherwise p = (t - lo) * (num_bins / (hi - lo)), b = floorf(p), t == hi takes
// the last bin (the top edge is inclusive), and a b outside [0, num_bins) -- compared as floats, so no p overflows an
// integer, and a NaN p counts as outside -- is "outside": -1 with trim on, clamped into the range with it off.
//
// Keys.  gsr_hist_key maps a float to a uint32 whose unsigned order is the float order (-0 below +0), so a minimum or a
// maximum over floats can be taken with integer atomics: exact and independent of the order.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"         // GSR_HD

#define GSR_HIST_KEPT 0
#define GSR_HIST_DROPPED 1
#define GSR_HIST_NONFINITE 2

GSR_HD bool gsr_hist_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }      // false for NaN

// class of one entry; *t is written for GSR_HIST_KEPT alone
GSR_HD int gsr_hist_entry(float v, bool weighted, float w, float eps, int mode, float min_value, float* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float x = weighted ? v / (eps + w) : v;
  if (!gsr_hist_finite(x)) return GSR_HIST_NONFINITE;
  float r = x;
  if (mode == 1) {
    if (!(x > min_value)) return GSR_HIST_DROPPED;
    r = log10f(x);
  } else if (mode == 2) {
    r = log10f(fmaxf(x, min_value));
  }
  if (!gsr_hist_finite(r)) return GSR_HIST_NONFINITE;
  *t = r;
  return GSR_HIST_KEPT;
}

// bin of a kept t in [0, num_bins), or -1 (outside, trim on); *outside is set to 1 when b fell outside the range
GSR_HD int gsr_hist_bin(float t, float lo, float hi, int num_bins, bool trim, int* outside) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *outside = 0;
  if (hi == lo) return 0;
  const float scale = (float)num_bins / (hi - lo);
  const float p = (t - lo) * scale;
  const float b = t == hi ? (float)(num_bins - 1) : floorf(p);
  if (b >= 0.f && b < (float)num_bins) return (int)b;
  *outside = 1;
  if (trim) return -1;
  return b < 0.f ? 0 : num_bins - 1;
}

GSR_HD uint32_t gsr_hist_float_bits(float x) {
  union { float f; uint32_t u; } c;
  c.f = x;
  return c.u;
}

GSR_HD uint32_t gsr_hist_key(float x) {
  const uint32_t b = gsr_hist_float_bits(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

GSR_HD float gsr_hist_unkey(uint32_t k) {
  union { float f; uint32_t u; } c;
  c.u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return c.f;
}
