// Per-row maths of the neural colour model (color_model.hip): the real spherical-harmonic basis up to degree 5 and its
// gradient, F.normalize with its eps, LayerNorm without affine, GLU and the luminance activation, each with its
// derivative.  Shared with the CPU unit-test shim (hostmath_shim.cpp).  Pure functions, no wave intrinsics: the kernels
// spread a row over four lanes and do the row sums themselves.
//
// Real SH, index l(l+1) + m (-l <= m <= l), Condon-Shortley phase included:
//   Y_l^0 = K_l^0 Q_l^0(z),  Y_l^m = sqrt2 K_l^m Q_l^m(z) C_m(x, y),  Y_l^-m = sqrt2 K_l^m Q_l^m(z) S_m(x, y)
//   K_l^m = sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!),  C_m + i S_m = (x + i y)^m,
//   Q_m^m = (-1)^m (2m-1)!!,  Q_{m+1}^m = (2m+1) z Q_m^m,  Q_l^m = ((2l-1) z Q_{l-1}^m - (l+m-1) Q_{l-2}^m) / (l-m).
// Q_l^m (sin theta)^m is the associated Legendre function, so every Y is a polynomial in (x, y, z); off the unit sphere
// (d = 0 for a point at the camera) it is that polynomial's value.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD

#define GSR_CM_LN_EPS 1e-5f        // nn.LayerNorm default
#define GSR_CM_NORM_EPS 1e-12f     // F.normalize default
#define GSR_CM_SPEC_BIAS -2.0f     // intensity bias of the specular luminance activation

// Value and gradient with respect to (x, y, z): forward-mode derivative of the SH polynomials.
struct GsrDual3 {
  float v, dx, dy, dz;
};
GSR_HD GsrDual3 operator+(GsrDual3 a, GsrDual3 b) { return {a.v + b.v, a.dx + b.dx, a.dy + b.dy, a.dz + b.dz}; }
GSR_HD GsrDual3 operator-(GsrDual3 a, GsrDual3 b) { return {a.v - b.v, a.dx - b.dx, a.dy - b.dy, a.dz - b.dz}; }
GSR_HD GsrDual3 operator*(GsrDual3 a, GsrDual3 b) {
  return {a.v * b.v, a.dx * b.v + a.v * b.dx, a.dy * b.v + a.v * b.dy, a.dz * b.v + a.v * b.dz};
}
GSR_HD GsrDual3 operator*(float s, GsrDual3 a) { return {s * a.v, s * a.dx, s * a.dy, s * a.dz}; }
GSR_HD GsrDual3 gsr_cm_const(GsrDual3, float s) { return {s, 0.f, 0.f, 0.f}; }
GSR_HD float gsr_cm_const(float, float s) { return s; }

// sqrt2 K_l^m (m > 0) and K_l^0
constexpr float gsr_cm_K(int l, int m) {
  const float t[36] = {
      2.820947918e-01f, 0.f, 0.f, 0.f, 0.f, 0.f,
      4.886025119e-01f, 4.886025119e-01f, 0.f, 0.f, 0.f, 0.f,
      6.307831305e-01f, 3.641828102e-01f, 1.820914051e-01f, 0.f, 0.f, 0.f,
      7.463526652e-01f, 3.046971996e-01f, 9.635371475e-02f, 3.933623933e-02f, 0.f, 0.f,
      8.462843753e-01f, 2.676186174e-01f, 6.307831305e-02f, 1.685838828e-02f, 5.960340338e-03f, 0.f,
      9.356025796e-01f, 2.415715473e-01f, 4.565273129e-02f, 9.318824751e-03f, 2.196468058e-03f, 6.945841871e-04f};
  return t[6 * l + m];
}
constexpr float gsr_cm_Qmm(int m) { return m == 0 ? 1.f : -(float)(2 * m - 1) * gsr_cm_Qmm(m - 1); }   // (-1)^m (2m-1)!!

// Degrees l = Lv .. S of order M; q1 = Q_{Lv-1}^M, q2 = Q_{Lv-2}^M (unused at Lv = M).  Compile-time recursion, so every
// constant and every emitted index is a literal.
template <int S, int M, int Lv, typename T, typename Emit>
GSR_HD void gsr_cm_rsh_l(T z, T q1, T q2, T C, T Sn, Emit& emit) {
  if constexpr (Lv <= S) {
    T q;
    constexpr float qmm = gsr_cm_Qmm(M);
    if constexpr (Lv == M) q = gsr_cm_const(z, qmm);
    else if constexpr (Lv == M + 1) q = (float)(2 * M + 1) * (z * q1);
    else q = (1.f / (float)(Lv - M)) * ((float)(2 * Lv - 1) * (z * q1) - (float)(Lv + M - 1) * q2);
    constexpr float k = gsr_cm_K(Lv, M);
    if constexpr (M == 0) emit(Lv * (Lv + 1), k * q);
    else {
      emit(Lv * (Lv + 1) + M, k * (q * C));
      emit(Lv * (Lv + 1) - M, k * (q * Sn));
    }
    gsr_cm_rsh_l<S, M, Lv + 1>(z, q, q1, C, Sn, emit);
  }
}

template <int S, int M, typename T, typename Emit>
GSR_HD void gsr_cm_rsh_m(T x, T y, T z, T C, T Sn, Emit& emit) {
  if constexpr (M <= S) {
    gsr_cm_rsh_l<S, M, M>(z, z, z, C, Sn, emit);
    gsr_cm_rsh_m<S, M + 1>(x, y, z, C * x - Sn * y, Sn * x + C * y, emit);    // C_{m+1} + i S_{m+1} = (C_m + i S_m)(x + i y)
  }
}

// Calls emit(c, Y_c) for c = 0 .. (S+1)^2 - 1.  T is float or GsrDual3.
template <int S, typename T, typename Emit>
GSR_HD void gsr_cm_rsh(T x, T y, T z, Emit&& emit) {
  static_assert(S >= 0 && S <= 5, "SH degree 0..5");
  gsr_cm_rsh_m<S, 0>(x, y, z, gsr_cm_const(x, 1.f), gsr_cm_const(x, 0.f), emit);
}

GSR_HD float gsr_cm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// d = v / max(|v|, eps) and its vector-Jacobian product: dv = (dd - d (d . dd)) / |v| when |v| > eps, dd / eps otherwise.
GSR_HD void gsr_cm_normalize(const float v[3], float d[3], float& inv_norm, bool& clamped) {
  const float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  clamped = !(n > GSR_CM_NORM_EPS);
  const float den = clamped ? GSR_CM_NORM_EPS : n;
  inv_norm = 1.f / den;
  for (int k = 0; k < 3; ++k) d[k] = v[k] / den;
}
GSR_HD void gsr_cm_normalize_bwd(const float d[3], float inv_norm, bool clamped, const float dd[3], float dv[3]) {
  const float dot = clamped ? 0.f : d[0] * dd[0] + d[1] * dd[1] + d[2] * dd[2];
  for (int k = 0; k < 3; ++k) dv[k] = (dd[k] - d[k] * dot) * inv_norm;
}

// GLU: h = a sigmoid(b); gradients of a and b for an upstream dh.
GSR_HD float gsr_cm_glu(float a, float b) { return a * gsr_cm_sigmoid(b); }
GSR_HD void gsr_cm_glu_bwd(float a, float b, float dh, float& da, float& db) {
  const float s = gsr_cm_sigmoid(b);
  da = dh * s;
  db = dh * a * s * (1.f - s);
}

// Luminance activation: out_c = sigmoid(o_{c+1}) exp(o_0 + bias), c = 0..2; do_ = gradient of o for an upstream dout.
GSR_HD void gsr_cm_lum(const float o[4], float bias, float out[3]) {
  const float e = expf(o[0] + bias);
  for (int c = 0; c < 3; ++c) out[c] = gsr_cm_sigmoid(o[c + 1]) * e;
}
GSR_HD void gsr_cm_lum_bwd(const float o[4], float bias, const float dout[3], float do_[4]) {
  const float e = expf(o[0] + bias);
  float d0 = 0.f;
  for (int c = 0; c < 3; ++c) {
    const float s = gsr_cm_sigmoid(o[c + 1]);
    d0 += dout[c] * s * e;
    do_[c + 1] = dout[c] * e * s * (1.f - s);
  }
  do_[0] = d0;
}

// LayerNorm of one row without affine: y = (u - mean) rstd, rstd = 1 / sqrt(var + eps), var biased.  The statistics
// come from the caller's row sums (the kernels sum over four lanes): mean = sum u / F, var = sum (u - mean)^2 / F.
GSR_HD float gsr_cm_ln_rstd(float sum_sq_dev, int F) { return 1.f / sqrtf(sum_sq_dev / (float)F + GSR_CM_LN_EPS); }
// du = rstd (dy - mean(dy) - y mean(dy y)), from the row sums of dy and dy y.
GSR_HD float gsr_cm_ln_bwd(float y, float dy, float rstd, float sum_dy, float sum_dy_y, int F) {
  return rstd * (dy - sum_dy / (float)F - y * (sum_dy_y / (float)F));
}
