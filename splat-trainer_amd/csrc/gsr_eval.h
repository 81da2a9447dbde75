// Per-pixel maths of the evaluation pass's colour fit (eval.hip), shared with the CPU unit-test shim (hostmath_shim.cpp).
// Pure functions, no memory access beyond the arguments, no wave intrinsics.
//
// The fit (util/colors.py fit_colors_batch) warps an image towards a photograph with an affine-quadratic map per output
// channel, re-solved a few times as the set of unsaturated pixels changes.  For a pixel x = (r, g, b) the design row is
//   a = [r^2, rg, rb, g^2, gb, b^2, r, g, b, 1]                                   (the reference's column order)
// and channel c solves  min_w sum_p m_c(p) (a(p) . w - ref_c(p))^2  over the pixels whose input, current iterate and
// photograph are all unclipped in that channel.  Instead of a least-squares solve on a (pixels x 10) matrix the kernels
// sum the normal equations: a a^T holds only the 35 monomials of degree <= 4, so 35 + 10 fp64 sums per channel say
// everything the solve needs.  Images and iterates are fp32; every product and sum here is fp64 (r*r, r*g, ... are exact
// in fp64, the higher monomials and the sums round once per fused multiply-add, written out as fma so that the device
// and the host shim round alike).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD

#define GSR_EV_COLS 10
#define GSR_EV_MONOS 35
#define GSR_EV_SUMS 45        // 35 monomial sums, then the 10 sums of a * ref_c
#define GSR_EV_SWEEPS 12      // cyclic Jacobi sweeps of the 10 x 10 eigenproblem (converged after 6-8; the rest skip)
#define GSR_EV_WORK 240       // doubles of caller memory gsr_ev_solve works in (LDS on the device)
#define GSR_EV_RANK_CUT 1e-9  // eigenvalues <= this share of the largest are dropped

// Monomial numbering: mono[i][j] is the index of a_i a_j, numbered in order of first appearance over (i, j) row-major;
// (ci[k], cj[k]) is that first pair, the product that is accumulated for monomial k.
struct GsrEvTables {
  int mono[GSR_EV_COLS][GSR_EV_COLS];
  int ci[GSR_EV_MONOS], cj[GSR_EV_MONOS];
};

constexpr GsrEvTables gsr_ev_tables() {
  const int e[GSR_EV_COLS][3] = {{2, 0, 0}, {1, 1, 0}, {1, 0, 1}, {0, 2, 0}, {0, 1, 1},
                                 {0, 0, 2}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}};
  GsrEvTables t{};
  int code[GSR_EV_MONOS] = {};
  int n = 0;
  for (int i = 0; i < GSR_EV_COLS; ++i)
    for (int j = 0; j < GSR_EV_COLS; ++j) {
      const int c = (e[i][0] + e[j][0]) * 25 + (e[i][1] + e[j][1]) * 5 + (e[i][2] + e[j][2]);
      int k = 0;
      while (k < n && code[k] != c) ++k;
      if (k == n) { code[n] = c; t.ci[n] = i; t.cj[n] = j; ++n; }
      t.mono[i][j] = k;
    }
  return t;
}

GSR_HD bool gsr_ev_unclipped(float z, float lo, float hi) { return z >= lo && z <= hi; }   // NaN: clipped

GSR_HD void gsr_ev_row(float r, float g, float b, double a[GSR_EV_COLS]) {
  const double R = r, G = g, B = b;
  a[0] = R * R; a[1] = R * G; a[2] = R * B; a[3] = G * G; a[4] = G * B; a[5] = B * B;   // exact: 24 x 24 bit products
  a[6] = R; a[7] = G; a[8] = B; a[9] = 1.0;
}

// acc[45] += the 35 monomials of the row and the 10 products with the photograph's channel
GSR_HD void gsr_ev_accumulate(const double a[GSR_EV_COLS], double ref, double acc[GSR_EV_SUMS]) {
  constexpr GsrEvTables T = gsr_ev_tables();
#pragma unroll
  for (int k = 0; k < GSR_EV_MONOS; ++k) acc[k] = fma(a[T.ci[k]], a[T.cj[k]], acc[k]);
#pragma unroll
  for (int i = 0; i < GSR_EV_COLS; ++i) acc[GSR_EV_MONOS + i] = fma(a[i], ref, acc[GSR_EV_MONOS + i]);
}

// One channel of the warp: clip(a . w, 0, 1), the dot product in fp64 in column order, rounded to fp32 once (NaN -> 0).
GSR_HD float gsr_ev_warp(const double a[GSR_EV_COLS], const double* w) {
  double y = 0.0;
#pragma unroll
  for (int i = 0; i < GSR_EV_COLS; ++i) y = fma(a[i], w[i], y);
  return fminf(fmaxf((float)y, 0.f), 1.f);
}

// The minimum-norm least-squares weights w[10] of one channel from its 45 sums.  S = sum a a^T and t = sum a ref are
// scaled to unit diagonal (s_i = 1 / sqrt(S_ii), 1 where S_ii <= 0), the scaled S is diagonalised by cyclic Jacobi
// rotations (a fixed number of sweeps; a rotation is skipped once its off-diagonal entry is below 1e-18 of the two
// diagonal entries' geometric mean), eigenvalues <= GSR_EV_RANK_CUT * lambda_max are dropped and w = D V L^+ V^T D t.
// lambda_max <= 0 (no unmasked pixel) gives w = 0.  `work`: GSR_EV_WORK doubles; nothing is indexed outside it.
GSR_HD void gsr_ev_solve(const double* sums, double* work, double* w) {
  constexpr GsrEvTables T = gsr_ev_tables();
  constexpr int N = GSR_EV_COLS;
  double* A = work;
  double* V = work + 100;
  double* s = work + 200;
  double* t = work + 210;
  double* y = work + 220;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) A[i * N + j] = sums[T.mono[i][j]];
  for (int i = 0; i < N; ++i) {
    const double d = A[i * N + i];
    s[i] = d > 0.0 ? 1.0 / sqrt(d) : 1.0;
  }
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < N; ++j) {
      A[i * N + j] = (A[i * N + j] * s[i]) * s[j];
      V[i * N + j] = i == j ? 1.0 : 0.0;
    }
    t[i] = sums[GSR_EV_MONOS + i] * s[i];
  }
  for (int sweep = 0; sweep < GSR_EV_SWEEPS; ++sweep)
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p * N + q], app = A[p * N + p], aqq = A[q * N + q];
        if (apq * apq <= 1e-36 * fabs(app * aqq)) continue;
        const double theta = (aqq - app) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
        for (int k = 0; k < N; ++k) {                        // A <- A J
          const double akp = A[k * N + p], akq = A[k * N + q];
          A[k * N + p] = c * akp - sn * akq;
          A[k * N + q] = sn * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {                        // A <- J^T A,  V <- V J
          const double apk = A[p * N + k], aqk = A[q * N + k];
          A[p * N + k] = c * apk - sn * aqk;
          A[q * N + k] = sn * apk + c * aqk;
          const double vkp = V[k * N + p], vkq = V[k * N + q];
          V[k * N + p] = c * vkp - sn * vkq;
          V[k * N + q] = sn * vkp + c * vkq;
        }
        A[p * N + q] = 0.0;
        A[q * N + p] = 0.0;
      }
  double lmax = 0.0;
  for (int i = 0; i < N; ++i) {
    lmax = fmax(lmax, A[i * N + i]);
    y[i] = 0.0;
  }
  for (int i = 0; i < N; ++i) {
    const double lam = A[i * N + i];
    if (!(lmax > 0.0) || !(lam > GSR_EV_RANK_CUT * lmax)) continue;
    double dot = 0.0;
    for (int k = 0; k < N; ++k) dot = fma(V[k * N + i], t[k], dot);
    const double f = dot / lam;
    for (int k = 0; k < N; ++k) y[k] = fma(V[k * N + i], f, y[k]);
  }
  for (int i = 0; i < N; ++i) w[i] = s[i] * y[i];
}
