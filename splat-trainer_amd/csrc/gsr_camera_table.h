// Per-row maths of the pose tables (camera_table.hip): unit-quaternion + translation rows to 4x4 rigid transforms, the
// product of two such rows for a camera rig, and the gradients back to the rows.  Shared with the CPU unit-test shim
// (hostmath_shim.cpp).  Pure functions, no memory access beyond the arguments, no wave intrinsics, no contraction: every
// fused multiply-add is written out, and the order below is the contract the fp32 results are a function of.
//
// A row is q = (x, y, z, w) (XYZW, roma's order) and t.  Forward:
//   n = sqrt(fmaf(w, w, fmaf(z, z, fmaf(y, y, x x))))      d = max(n, GSR_POSE_EPS)      q^ = q / d  (F.normalize)
//   x2 = x^ + x^, y2, z2 likewise (exact)
//   R00 = fmaf(-z2, z^, fmaf(-y2, y^, 1))   R01 = fmaf(x2, y^, -(z2 w^))            R02 = fmaf(x2, z^, y2 w^)
//   R10 = fmaf(x2, y^, z2 w^)               R11 = fmaf(-z2, z^, fmaf(-x2, x^, 1))   R12 = fmaf(y2, z^, -(x2 w^))
//   R20 = fmaf(x2, z^, -(y2 w^))            R21 = fmaf(y2, z^, x2 w^)               R22 = fmaf(-y2, y^, fmaf(-x2, x^, 1))
// so q = 0 gives the identity.  T = [R t; 0 0 0 1].  For a rig, T = C W with C the left (camera_t_rig) and W the right
// (rig_t_world) row:
//   R_ij = fmaf(Rc_i2, Rw_2j, fmaf(Rc_i1, Rw_1j, Rc_i0 Rw_0j))      t_i = fmaf(Rc_i2, tw_2, fmaf(Rc_i1, tw_1, fmaf(Rc_i0, tw_0, tc_i)))
//
// Backward from G = dL/dT (row 3 ignored), G_R its 3x3 block and g its last column.  One image's terms:
//   left   dRc_ij = fmaf(g_i, tw_j, fmaf(G_i2, Rw_j2, fmaf(G_i1, Rw_j1, G_i0 Rw_j0)))      dtc = g
//   right  dRw_ij = fmaf(Rc_2i, G_2j, fmaf(Rc_1i, G_1j, Rc_0i G_0j))      dtw_i = fmaf(Rc_2i, g_2, fmaf(Rc_1i, g_1, Rc_0i g_0))
//   single table: dR = G_R, dt = g
// A row's (dR, dt) is the plain float sum `acc = acc + term` of its images' terms from 0, in increasing batch position.
// Then, with D = dR and S_ij = D_ij + D_ji, A_ij = D_ij - D_ji:
//   dq^_x = 2 (fmaf(w^, A21, fmaf(-(x^ + x^), D11 + D22, fmaf(z^, S02, y^ S01))))
//   dq^_y = 2 (fmaf(w^, A02, fmaf(-(y^ + y^), D00 + D22, fmaf(z^, S12, x^ S01))))
//   dq^_z = 2 (fmaf(w^, A10, fmaf(-(z^ + z^), D00 + D11, fmaf(y^, S12, x^ S02))))
//   dq^_w = 2 (fmaf(z^, A10, fmaf(y^, A02, x^ A21)))
// and through the normalisation: n >= eps: s = q^ . dq^ (fmaf chain x, y, z, w), dq = fmaf(-q^, s, dq^) / d;  n < eps
// (the clamp holds, its gradient is 0): dq = dq^ / eps, as F.normalize's autograd gives.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"         // GSR_HD

#define GSR_POSE_EPS 1e-12f

// idx clamped into [0, A): an index outside reads row 0 and sets *bad.
GSR_HD int64_t gsr_pose_index(int64_t i, int64_t A, bool* bad) {
  const bool out = i < 0 || i >= A;
  *bad = *bad || out;
  return out ? 0 : i;
}

// qh[4] = F.normalize(q), returns d = max(|q|, eps); *clamped = the clamp holds.
GSR_HD float gsr_pose_normalize(const float* q, float* qh, bool* clamped) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float n = sqrtf(fmaf(q[3], q[3], fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0]))));
  const float d = fmaxf(n, GSR_POSE_EPS);
  *clamped = !(n >= GSR_POSE_EPS);
  for (int k = 0; k < 4; ++k) qh[k] = q[k] / d;
  return d;
}

// R[9], row-major, of the normalised quaternion qh.
GSR_HD void gsr_pose_rotmat(const float* qh, float* R) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float x = qh[0], y = qh[1], z = qh[2], w = qh[3];
  const float x2 = x + x, y2 = y + y, z2 = z + z;
  R[0] = fmaf(-z2, z, fmaf(-y2, y, 1.f));
  R[1] = fmaf(x2, y, -(z2 * w));
  R[2] = fmaf(x2, z, y2 * w);
  R[3] = fmaf(x2, y, z2 * w);
  R[4] = fmaf(-z2, z, fmaf(-x2, x, 1.f));
  R[5] = fmaf(y2, z, -(x2 * w));
  R[6] = fmaf(x2, z, -(y2 * w));
  R[7] = fmaf(y2, z, x2 * w);
  R[8] = fmaf(-y2, y, fmaf(-x2, x, 1.f));
}

// R[9] of the raw row q.
GSR_HD void gsr_pose_row_rotmat(const float* q, float* R) {
  float qh[4];
  bool clamped;
  gsr_pose_normalize(q, qh, &clamped);
  gsr_pose_rotmat(qh, R);
}

// (R, t) = (Rc, tc) (Rw, tw).
GSR_HD void gsr_pose_compose(const float* Rc, const float* tc, const float* Rw, const float* tw, float* R, float* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = fmaf(Rc[3 * i + 2], Rw[6 + j], fmaf(Rc[3 * i + 1], Rw[3 + j], Rc[3 * i] * Rw[j]));
    t[i] = fmaf(Rc[3 * i + 2], tw[2], fmaf(Rc[3 * i + 1], tw[1], fmaf(Rc[3 * i], tw[0], tc[i])));
  }
}

// T[16] of one image: the left row alone (qr == NULL) or the product left x right.
GSR_HD void gsr_pose_forward_image(const float* ql, const float* tl, const float* qr, const float* tr, float* T) {
  float R[9], t[3];
  if (qr) {
    float Rc[9], Rw[9];
    gsr_pose_row_rotmat(ql, Rc);
    gsr_pose_row_rotmat(qr, Rw);
    gsr_pose_compose(Rc, tl, Rw, tr, R, t);
  } else {
    gsr_pose_row_rotmat(ql, R);
    for (int i = 0; i < 3; ++i) t[i] = tl[i];
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
    T[4 * i + 3] = t[i];
  }
  T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

// acc[12] = (dR[9], dt[3]) of a row += one image's term.  G[16] is the image's dL/dT.
// The left row of a rig (Rw, tw of the image's right row), or the row of a single table (Rw == NULL).
GSR_HD void gsr_pose_acc_left(const float* G, const float* Rw, const float* tw, float* acc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int i = 0; i < 3; ++i) {
    const float g = G[4 * i + 3];
    for (int j = 0; j < 3; ++j) {
      const float term = Rw ? fmaf(g, tw[j], fmaf(G[4 * i + 2], Rw[3 * j + 2], fmaf(G[4 * i + 1], Rw[3 * j + 1], G[4 * i] * Rw[3 * j])))
                            : G[4 * i + j];
      acc[3 * i + j] = acc[3 * i + j] + term;
    }
    acc[9 + i] = acc[9 + i] + g;
  }
}

// The right row of a rig (Rc of the image's left row).
GSR_HD void gsr_pose_acc_right(const float* G, const float* Rc, float* acc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      const float term = fmaf(Rc[6 + i], G[8 + j], fmaf(Rc[3 + i], G[4 + j], Rc[i] * G[j]));
      acc[3 * i + j] = acc[3 * i + j] + term;
    }
    const float term = fmaf(Rc[6 + i], G[11], fmaf(Rc[3 + i], G[7], Rc[i] * G[3]));
    acc[9 + i] = acc[9 + i] + term;
  }
}

// d_q[4] of the raw row q from the summed D = dL/dR[9].
GSR_HD void gsr_pose_row_backward(const float* q, const float* D, float* d_q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float qh[4], dh[4];
  bool clamped;
  const float d = gsr_pose_normalize(q, qh, &clamped);
  const float x = qh[0], y = qh[1], z = qh[2], w = qh[3];
  const float S01 = D[1] + D[3], S02 = D[2] + D[6], S12 = D[5] + D[7];
  const float A21 = D[7] - D[5], A02 = D[2] - D[6], A10 = D[3] - D[1];
  dh[0] = 2.f * fmaf(w, A21, fmaf(-(x + x), D[4] + D[8], fmaf(z, S02, y * S01)));
  dh[1] = 2.f * fmaf(w, A02, fmaf(-(y + y), D[0] + D[8], fmaf(z, S12, x * S01)));
  dh[2] = 2.f * fmaf(w, A10, fmaf(-(z + z), D[0] + D[4], fmaf(y, S12, x * S02)));
  dh[3] = 2.f * fmaf(z, A10, fmaf(y, A02, x * A21));
  if (clamped) {
    for (int k = 0; k < 4; ++k) d_q[k] = dh[k] / GSR_POSE_EPS;
  } else {
    const float s = fmaf(w, dh[3], fmaf(z, dh[2], fmaf(y, dh[1], x * dh[0])));
    for (int k = 0; k < 4; ++k) d_q[k] = fmaf(-qh[k], s, dh[k]) / d;
  }
}

// (d_q[4], d_t[3]) of row `a` of one table: the sum over the images b = 0 .. B-1 that select it, then the chain through
// the row.  `left`: the row belongs to the left table.  The other table may be absent (q_other == NULL, left only).
// Returns true when an index was out of range.
GSR_HD bool gsr_pose_backward_row(bool left, int64_t a, const float* q_own, int64_t A_own, const int64_t* idx_own,
                                  const float* q_other, const float* t_other, int64_t A_other, const int64_t* idx_other,
                                  int64_t B, const float* G, float* d_q, float* d_t) {
  float acc[12];
  bool bad = false;
  for (int k = 0; k < 12; ++k) acc[k] = 0.f;
  for (int64_t b = 0; b < B; ++b) {
    if (gsr_pose_index(idx_own[b], A_own, &bad) != a) continue;
    if (q_other) {
      const int64_t o = gsr_pose_index(idx_other[b], A_other, &bad);
      float Ro[9];
      gsr_pose_row_rotmat(q_other + 4 * o, Ro);
      if (left) gsr_pose_acc_left(G + 16 * b, Ro, t_other + 3 * o, acc);
      else gsr_pose_acc_right(G + 16 * b, Ro, acc);
    } else {
      gsr_pose_acc_left(G + 16 * b, nullptr, nullptr, acc);
    }
  }
  gsr_pose_row_backward(q_own + 4 * a, acc, d_q);
  for (int i = 0; i < 3; ++i) d_t[i] = acc[9 + i];
  return bad;
}
