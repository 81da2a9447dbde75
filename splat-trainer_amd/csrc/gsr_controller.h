// Per-row maths of the MCMC controller's position noise (controller.hip), shared with the CPU unit-test shim
// (hostmath_shim.cpp).  Pure functions, no memory access beyond the arguments, no wave intrinsics, no contraction.
//
// Draw.  Philox4x32-10 (Salmon et al., SC 2011): multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9,
// 0xBB67AE85, key = (seed lo, seed hi), counter = (i lo, i hi, step lo, step hi).  Each of the four words w gives a
// uniform u = ((w >> 8) + 0.5) 2^-24 in (0, 1); Box-Muller on the pairs (0, 1) and (2, 3) gives
// sqrt(-2 ln u_a) (cos, sin)(2 pi u_b); xi is the first three normals, |xi_j| <= sqrt(50 ln 2) < 5.9.  The draw of row i
// is a function of (seed, step, i) alone: no generator state, nothing shared between rows.
//   float32 holds k + 0.5 exactly only for k < 2^23, so both halves of Box-Muller work on exact integers:
//   ln u        k = w >> 8 < 2^23: logf((k + 0.5) 2^-24), the argument exact; else log1pf(-((2^24 - k) - 0.5) 2^-24), exact too;
//   2 pi u      the quadrant is the top two bits of k, the rest f gives the angle 2 pi (f + 0.5) 2^-24 in (0, pi / 2) --
//               the fraction exact, the product with 2 pi carried in two floats -- and the quadrant turns (cos, sin).
//
// Level.  o = sigmoid(a), h = threshold / 2, gate = sigmoid(-(o - h) margin / h): soft_lt(o, h, margin) of the reference's
// util/misc.py as ONE sigmoid of the negated argument, which keeps its relative accuracy where the gate is tiny
// (1 - sigmoid(x) quantises to multiples of 6e-8 there).  level = gate noise_level.
//
// Offset.  sigma_j = max(exp(ls_j), scale_eps), q_n = q / max(|q|, 1e-12), offset = R(q_n) (sigma * (xi level)): the
// reference's sample_gaussians (gaussians/split.py:16-36).  A row whose level max_j sigma_j is 0 in float32 has no offset.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"         // GSR_HD, gsr_quat_to_rot

#define GSR_PHILOX_M0 0xD2511F53u
#define GSR_PHILOX_M1 0xCD9E8D57u
#define GSR_PHILOX_W0 0x9E3779B9u
#define GSR_PHILOX_W1 0xBB67AE85u

GSR_HD void gsr_philox4x32(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)GSR_PHILOX_M0 * c0, p1 = (uint64_t)GSR_PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += GSR_PHILOX_W0;
    k1 += GSR_PHILOX_W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of row i at (seed, step)
GSR_HD void gsr_mcmc_words(uint64_t i, uint64_t seed, uint64_t step, uint32_t w[4]) {
  const uint32_t counter[4] = {(uint32_t)i, (uint32_t)(i >> 32), (uint32_t)step, (uint32_t)(step >> 32)};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  gsr_philox4x32(counter, key, w);
}

// sqrt(-2 ln u) of the uniform of word w
GSR_HD float gsr_mcmc_radius(uint32_t w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t k = w >> 8;
  const float lo = logf(((float)(k & 0x7FFFFFu) + 0.5f) * 0x1p-24f);
  const float hi = log1pf(-(((float)(0x1000000u - (k | 0x800000u)) - 0.5f) * 0x1p-24f));
  return sqrtf(-2.f * (k < 0x800000u ? lo : hi));
}

// (cos, sin)(2 pi u) of the uniform of word w
GSR_HD void gsr_mcmc_angle(uint32_t w, float* c, float* s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t k = w >> 8;
  const float frac = ((float)(k & 0x3FFFFFu) + 0.5f) * 0x1p-24f;         // in (0, 1/4), exact
  const float theta = fmaf(frac, 6.2831855f, frac * -1.7484555e-7f);     // 2 pi = 6.2831855 - 1.7484555e-7
  const float ct = cosf(theta), st = sinf(theta);
  const uint32_t quad = k >> 22;
  const float cq = (quad & 1u) ? -st : ct, sq = (quad & 1u) ? ct : st;
  *c = (quad & 2u) ? -cq : cq;
  *s = (quad & 2u) ? -sq : sq;
}

// the four normals of the words w; xi is the first three
GSR_HD void gsr_mcmc_normals(const uint32_t w[4], float z[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int p = 0; p < 2; ++p) {
    const float r = gsr_mcmc_radius(w[2 * p]);
    float c, s;
    gsr_mcmc_angle(w[2 * p + 1], &c, &s);
    z[2 * p] = r * c;
    z[2 * p + 1] = r * s;
  }
}

GSR_HD float gsr_mcmc_sigmoid(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float e = expf(-fabsf(x)), r = 1.f / (1.f + e);
  return x >= 0.f ? r : e * r;
}

// gate noise_level of a row with opacity logit a
GSR_HD float gsr_mcmc_level(float a, float opacity_threshold, float margin, float noise_level) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float o = gsr_mcmc_sigmoid(a), h = 0.5f * opacity_threshold;
  return gsr_mcmc_sigmoid(-(((o - h) * margin) / h)) * noise_level;
}

// sigma[3] of a row and their maximum
GSR_HD float gsr_mcmc_sigma(const float* ls, float scale_eps, float* sigma) {
  for (int j = 0; j < 3; ++j) sigma[j] = fmaxf(expf(ls[j]), scale_eps);
  return fmaxf(fmaxf(sigma[0], sigma[1]), sigma[2]);
}

// off[3] = R(q / |q|) (sigma * (xi level)), q in xyzw
GSR_HD void gsr_mcmc_offset(const float* sigma, const float* q, float level, const float* xi, float* off) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float norm = sqrtf(fmaf(q[0], q[0], fmaf(q[1], q[1], fmaf(q[2], q[2], q[3] * q[3]))));
  const float inv = 1.f / fmaxf(norm, 1e-12f);
  float qn[4], Rq[9], v[3];
  for (int j = 0; j < 4; ++j) qn[j] = q[j] * inv;
  gsr_quat_to_rot(qn, Rq);
  for (int j = 0; j < 3; ++j) v[j] = sigma[j] * (xi[j] * level);
  for (int j = 0; j < 3; ++j) off[j] = fmaf(Rq[3 * j], v[0], fmaf(Rq[3 * j + 1], v[1], Rq[3 * j + 2] * v[2]));
}

// One row: adds the offset of row i to p[3] and returns true, or returns false and leaves p alone (level max sigma == 0).
GSR_HD bool gsr_mcmc_noise_row(float* p, const float* ls, const float* q, float level, float scale_eps, uint64_t i,
                               uint64_t seed, uint64_t step) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float sigma[3], z[4], off[3];
  uint32_t w[4];
  if (!(level * gsr_mcmc_sigma(ls, scale_eps, sigma) != 0.f)) return false;
  gsr_mcmc_words(i, seed, step, w);
  gsr_mcmc_normals(w, z);
  gsr_mcmc_offset(sigma, q, level, z, off);
  for (int j = 0; j < 3; ++j) p[j] += off[j];
  return true;
}
