// Direct least-squares fit of per-point SH coefficients to view-dependent colours (sh_fit.hip): the row layout of the
// fp64 normal equations, the per-component update and the ridge Cholesky solve.  Shared with the CPU unit-test shim
// (hostmath_shim.cpp).  Pure functions, no memory access beyond the arguments, no wave intrinsics.
//
// Point p at x_p, camera j at c_j, d = normalize(x_p - c_j), Y(d) the K = (degree + 1)^2 values of gsr_sh_basis<K>
// (gsr_math.h), colour_c = 0.5 + sum_k s_ck Y_k(d) as evaluate_sh_at has it.  One view brings the colour y (3 values) and
// a weight w >= 0 of every point it sees; per point, over the views in the order they are added,
//   G   += w Y Y^T            lower triangle, T = K (K + 1) / 2 values, entry (i, j <= i) at i (i + 1) / 2 + j
//   b_c += w Y (y_c - 0.5)    3 K values, channel-major
//   W   += w
// one row of R(K) = T + 3 K + 1 doubles: 5, 23, 73, 185 for K = 1, 4, 9, 16.  The solution minimises
//   J(s) = sum_j w_j |Y(d_j) . s_c - (y_jc - 0.5)|^2 + ridge W Y0^2 sum_{k >= 1} s_ck^2
// i.e. (G + ridge W Y0^2 diag(0, 1, ..., 1)) s_c = b_c; Y0 = Y_0 is the constant term and E[Y_k^2] = Y0^2 on the sphere,
// so ridge is relative to a typical diagonal entry.  ridge >= GSR_SHF_MIN_RIDGE keeps the matrix positive definite
// wherever W > 0; W == 0 (a point no view saw) gives s = 0.
//
// Precision: the direction and the basis are float32, as everywhere on this path; every product and sum after them is
// fp64 through explicit fma, so the host and the device perform the same operations in the same order.  Every component
// of a row is one update acc = fma(w e_a, e_b, acc) over the extended operand vector
//   e = (Y_0 .. Y_{K-1}, y_0 - 0.5, y_1 - 0.5, y_2 - 0.5, 1)
// (w e_a is exact: 24 x 24 bits, or w itself), with (a, b) from GsrShfTable: G_ij = (i, j), b_ck = (k, K + c),
// W = (K + 3, K + 3).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"         // GSR_HD, gsr_sh_basis, GSR_SH_C0

#define GSR_SHF_MIN_RIDGE 1e-6f

constexpr int gsr_shf_tri(int i, int j) { return i * (i + 1) / 2 + j; }                    // j <= i
constexpr int gsr_shf_row_doubles(int K) { return K * (K + 1) / 2 + 3 * K + 1; }

// component of a row -> the two operands of its update
template <int K>
struct GsrShfTable {
  static constexpr int T = K * (K + 1) / 2, R = T + 3 * K + 1, E = K + 4;
  uint8_t a[R], b[R];
  constexpr GsrShfTable() : a{}, b{} {
    int n = 0;
    for (int i = 0; i < K; ++i)
      for (int j = 0; j <= i; ++j, ++n) { a[n] = (uint8_t)i; b[n] = (uint8_t)j; }
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < K; ++k, ++n) { a[n] = (uint8_t)k; b[n] = (uint8_t)(K + c); }
    a[n] = b[n] = (uint8_t)(K + 3);
  }
};

// e[K + 4] of one point in one view: p[3] its position, cam[3] the camera's, col[3] the colour.
template <int K>
GSR_HD void gsr_shf_operands(const float* p, const float* cam, const float* col, double* e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float vx = p[0] - cam[0], vy = p[1] - cam[1], vz = p[2] - cam[2];
  const float inv = 1.f / sqrtf((vx * vx + vy * vy) + vz * vz);
  float Y[K];
  gsr_sh_basis<K>(vx * inv, vy * inv, vz * inv, Y);
  for (int k = 0; k < K; ++k) e[k] = (double)Y[k];
  for (int c = 0; c < 3; ++c) e[K + c] = (double)col[c] - 0.5;
  e[K + 3] = 1.0;
}

GSR_HD double gsr_shf_update(double acc, float w, double ea, double eb) { return fma((double)w * ea, eb, acc); }

// ---- solve: in-place Cholesky of the packed lower triangle A, column by column -------------------------------------
// What is added to every diagonal entry but the first.
GSR_HD double gsr_shf_ridge_term(float ridge, double W) {
  return ((double)ridge * W) * ((double)GSR_SH_C0 * (double)GSR_SH_C0);
}

// A_ij - sum_{k < j} L_ik L_jk with the columns below j already factored: the pivot's square for i == j, and L_ij times
// the pivot for i > j.
GSR_HD double gsr_shf_chol_dot(const double* A, int i, int j) {
  double s = A[gsr_shf_tri(i, j)];
  for (int k = 0; k < j; ++k) s = fma(-A[gsr_shf_tri(i, k)], A[gsr_shf_tri(j, k)], s);
  return s;
}

// One step of a substitution: b_i - l z.
GSR_HD double gsr_shf_eliminate(double b, double l, double z) { return fma(-l, z, b); }

// One whole row in the order the device's lanes work in: `row` R(K) doubles as accumulated, `work` R(K) doubles,
// sh[3 K] channel-major and *weight = (float)W.
template <int K>
GSR_HD void gsr_shf_solve_row(const double* row, float ridge, double* work, float* sh, float* weight) {
  constexpr int T = K * (K + 1) / 2, R = T + 3 * K + 1;
  const double W = row[R - 1];
  *weight = (float)W;
  if (!(W > 0.0)) {
    for (int k = 0; k < 3 * K; ++k) sh[k] = 0.f;
    return;
  }
  double* A = work;
  for (int k = 0; k < R; ++k) A[k] = row[k];
  const double term = gsr_shf_ridge_term(ridge, W);
  for (int i = 1; i < K; ++i) A[gsr_shf_tri(i, i)] += term;
  for (int j = 0; j < K; ++j) {
    const double d = sqrt(gsr_shf_chol_dot(A, j, j));
    for (int i = j + 1; i < K; ++i) A[gsr_shf_tri(i, j)] = gsr_shf_chol_dot(A, i, j) / d;
    A[gsr_shf_tri(j, j)] = d;
  }
  for (int c = 0; c < 3; ++c) {
    double* b = A + T + c * K;
    for (int j = 0; j < K; ++j) {                       // L z = b
      const double z = b[j] / A[gsr_shf_tri(j, j)];
      b[j] = z;
      for (int i = j + 1; i < K; ++i) b[i] = gsr_shf_eliminate(b[i], A[gsr_shf_tri(i, j)], z);
    }
    for (int j = K - 1; j >= 0; --j) {                  // L^T s = z
      const double x = b[j] / A[gsr_shf_tri(j, j)];
      b[j] = x;
      for (int i = 0; i < j; ++i) b[i] = gsr_shf_eliminate(b[i], A[gsr_shf_tri(j, i)], x);
    }
    for (int k = 0; k < K; ++k) sh[c * K + k] = (float)b[k];
  }
}
