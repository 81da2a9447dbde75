// Per-pair maths of the brute-force neighbour searches (neighbours.hip): the k nearest points of a cloud and the nearest
// centroid of a point.  Shared with the CPU unit-test shim (hostmath_shim.cpp), so the shim's results are the device's
// bit for bit.  Pure functions, no memory access beyond the arguments, no wave intrinsics.
//
// Squared distance, pinned: d = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with dx = q.x - c.x, ...  (no contraction).
// Order of a candidate list: (d, j) lexicographic -- ascending distance, equal distances by lower index.  A candidate
// whose distance is NaN never enters a list, nor does one at +inf (the list starts full of +inf).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD

GSR_HD float gsr_nb_dist2(float qx, float qy, float qz, float cx, float cy, float cz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

template <int K>
GSR_HD void gsr_nb_init(float (&d)[K], int32_t (&j)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) { d[i] = INFINITY; j[i] = -1; }
}

// Inserts candidate (dn, jn) into the sorted list (d, j).  The caller offers candidates in ascending index order (or
// whole sorted lists of higher indices, see knn_merge_kernel), so an equal distance goes BEHIND the entries already there:
// the strict comparisons keep the lower index first.  Fully unrolled: the list stays in registers on the device.
template <int K>
GSR_HD void gsr_nb_insert(float (&d)[K], int32_t (&j)[K], float dn, int32_t jn) {
  if (!(dn < d[K - 1])) return;
  d[K - 1] = dn;
  j[K - 1] = jn;
#pragma unroll
  for (int i = K - 1; i > 0; --i) {
    const bool sw = d[i] < d[i - 1];
    const float a = d[i - 1], b = d[i];
    const int32_t ja = j[i - 1], jb = j[i];
    d[i - 1] = sw ? b : a;
    d[i] = sw ? a : b;
    j[i - 1] = sw ? jb : ja;
    j[i] = sw ? ja : jb;
  }
}

// Mean neighbour distance of a full list: sqrt of each entry, summed in ascending order, divided by K.
template <int K>
GSR_HD float gsr_nb_mean_dist(const float (&d)[K]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) s += sqrtf(d[i]);
  return s / (float)K;
}

// Nearest-centroid step: index jn replaces the best when strictly closer, so ties keep the lowest index and a NaN
// distance never wins (a point whose distances are all NaN keeps the initial label 0).
GSR_HD void gsr_nb_argmin_step(float& best, int32_t& label, float dn, int32_t jn) {
  const bool better = dn < best;
  best = better ? dn : best;
  label = better ? jn : label;
}
