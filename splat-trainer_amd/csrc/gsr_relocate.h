// Arithmetic of the MCMC relocation move (relocate.hip), shared with the CPU shim (hostmath_shim.cpp).  Pure functions, no
// memory access beyond the arguments, no wave intrinsics.  The contract is in include/gsplat_hip.h under
// gsr_weighted_draws, gsr_relocate_weights, gsr_relocate_rescale and gsr_relocate_rows.
//
// Draw (integers only).  Draw k of domain d takes the Philox4x32-10 words at key (seed lo, seed hi), counter
// (k lo, k hi, step lo, (step hi & 0x00FFFFFF) | d << 24).  The noise step's counter is (i lo, i hi, step lo, step hi) with
// step < 2^56 in any run, so it is domain 0 and the streams of one seed never share a counter.  r = word0 2^32 + word1,
// t = floor(r S / 2^64) -- the high half of the 128-bit product -- and the source is the smallest i with P_i > t, P the
// inclusive prefix sum of the weights, S = P_{N-1}.  t takes each value of [0, S) floor(2^64 / S) or one more time: a
// weight's share of the draws is off by at most S / 2^64 of itself (below 2^-18 at 3 M rows of weight 2^24, where
// S < 2^46).  S < 2^56 is the caller's to keep.
//
// The prefix is held per block of GSR_RELOC_BLOCK = 256 rows: block_incl[b] = P of the block's last row.  A draw finds the
// first block with block_incl[b] > t and then the row inside it; which search finds them changes nothing, the answer is
// the smallest i with P_i > t.
//
// Weight.  w = 0 for a row that is not alive, else max(1, floor(2^24 sigmoid(a))) with the sigmoid in fp64 (a NaN logit
// gives 1): every alive row can be drawn and w <= 2^24.
//
// Rescale.  A source with c >= 1 copies: n = min(c + 1, 51), o = sigmoid(a), o' = 1 - (1 - o)^(1/n),
// D = sum_{k=0..n-1} C(n, k+1) (-1)^k o'^(k+1) / sqrt(k+1) -- the double sum of Eq. 9 of Kheradmand et al. 2024 collapsed
// by sum_i C(i-1, k) = C(n, k+1) -- and coeff = o / D.  All fp64.  log(1 - o) and log(o) are formed from the logit,
// -softplus(a) and -softplus(-a), not from a rounded o: at a = 16 the rounding of o alone moves 1 - o by 1e-9 of itself.
// o' = -expm1(log(1 - o) / n).  The binomials are exact in fp64: C (n - j) <= 26 C(51, 26) < 2^53.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gsplat_hip.h"
#include "gsr_controller.h"   // gsr_philox4x32
#include "gsr_math.h"         // GSR_HD

#define GSR_RELOC_BLOCK 256
#define GSR_RELOC_MAX_COPIES 51
#define GSR_RELOC_DOMAINS 256
#define GSR_RELOC_MAX_WIDTH (1 << 20)      // 4-byte words of a row: 256 rows of it are counted in 32 bits

GSR_HD uint64_t gsr_mulhi_u64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// the four words of draw k at (seed, step) in domain d
GSR_HD void gsr_reloc_words(uint64_t k, uint64_t seed, uint64_t step, uint32_t domain, uint32_t w[4]) {
  const uint32_t counter[4] = {(uint32_t)k, (uint32_t)(k >> 32), (uint32_t)step,
                               ((uint32_t)(step >> 32) & 0x00FFFFFFu) | (domain << 24)};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  gsr_philox4x32(counter, key, w);
}

// t of draw k: in [0, S) for S > 0, 0 for S == 0
GSR_HD uint64_t gsr_reloc_target(uint64_t k, uint64_t seed, uint64_t step, uint32_t domain, uint64_t S) {
  uint32_t w[4];
  gsr_reloc_words(k, seed, step, domain, w);
  return gsr_mulhi_u64(((uint64_t)w[0] << 32) | (uint64_t)w[1], S);
}

GSR_HD uint32_t gsr_reloc_weight(float a, bool alive) {
  if (!alive) return 0u;
  const double x = (double)a, e = exp(-fabs(x)), r = 1.0 / (1.0 + e);
  const double s = (x >= 0.0 ? r : e * r) * 16777216.0;
  return s >= 1.0 ? (uint32_t)floor(s) : 1u;          // (NaN: 1)
}

// One source row with c >= 1 copies: the new logit and log(coeff), which is added to each log-scale.
GSR_HD void gsr_reloc_rescale(float a, int32_t c, double o_floor, float* a_out, double* log_coeff) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int n = c < GSR_RELOC_MAX_COPIES - 1 ? (int)c + 1 : GSR_RELOC_MAX_COPIES;
  const double x = (double)a, l = log1p(exp(-fabs(x)));
  const double log_o = x >= 0.0 ? -l : x - l, log_1mo = x >= 0.0 ? -x - l : -l;
  const double op = -expm1(log_1mo / (double)n);
  double D = 0.0, binom = (double)n, power = op;      // C(n, k+1) and o'^(k+1) at k = 0
  for (int k = 0; k < n; ++k) {
    const double term = (binom * power) / sqrt((double)(k + 1));
    D = (k & 1) ? D - term : D + term;
    binom = (binom * (double)(n - k - 1)) / (double)(k + 2);
    power = power * op;
  }
  *log_coeff = log_o - log(D);
  const double hi = 1.0 - 0x1p-24, p = op < o_floor ? o_floor : op > hi ? hi : op;
  *a_out = (float)(log(p) - log1p(-p));
}

// ---- the argument checks, in the order the ABI states them.  *launch is 0 where GSR_OK means "nothing to do". ----
inline bool gsr_reloc_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline size_t gsr_reloc_draws_workspace(int64_t N) {
  const int64_t blocks = N > 0 ? (N + GSR_RELOC_BLOCK - 1) / GSR_RELOC_BLOCK : 0;
  return (size_t)(blocks > 0 ? blocks : 1) * sizeof(uint64_t);
}

inline int gsr_weighted_draws_check(const void* weights, int64_t N, int64_t n, int32_t domain, const void* sources_out,
                                    const void* counts_out, const void* total_out, const void* workspace,
                                    size_t workspace_bytes) {
  if (N < 0 || n < 0 || N > GSR_NEIGHBOURS_MAX_N || n > GSR_NEIGHBOURS_MAX_N || domain < 0 || domain >= GSR_RELOC_DOMAINS)
    return GSR_ERR_INVALID_ARGUMENT;
  if (!total_out || (N > 0 && (!weights || !counts_out)) || (n > 0 && !sources_out)) return GSR_ERR_INVALID_ARGUMENT;
  if (!gsr_reloc_aligned16(weights) || !gsr_reloc_aligned16(counts_out)) return GSR_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < gsr_reloc_draws_workspace(N)) return GSR_ERR_WORKSPACE_TOO_SMALL;
  if (!gsr_reloc_aligned16(workspace)) return GSR_ERR_INVALID_ARGUMENT;
  return GSR_OK;
}

inline int gsr_relocate_weights_check(const void* alpha_logit, int64_t N, const void* weights_out, int* launch) {
  *launch = 0;
  if (N < 0 || N > GSR_NEIGHBOURS_MAX_N) return GSR_ERR_INVALID_ARGUMENT;
  if (N == 0) return GSR_OK;
  if (!alpha_logit || !weights_out) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

inline int gsr_relocate_rescale_check(const void* alpha_logit, const void* log_scaling, const void* counts, int64_t N,
                                      float o_floor, int* launch) {
  *launch = 0;
  if (N < 0 || N > GSR_NEIGHBOURS_MAX_N || !(o_floor > 0.f) || !(o_floor < 1.f)) return GSR_ERR_INVALID_ARGUMENT;
  if (N == 0) return GSR_OK;
  if (!alpha_logit || !log_scaling || !counts) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

inline int gsr_relocate_rows_check(const void* dst_rows, const void* src_rows, int64_t n, int64_t N,
                                   const GsrRowColumnC* columns, int32_t n_columns, int* launch) {
  *launch = 0;
  if (n < 0 || N < 0 || n > GSR_NEIGHBOURS_MAX_N || N > GSR_NEIGHBOURS_MAX_N || n_columns < 0 || n_columns > GSR_MAX_COLUMNS)
    return GSR_ERR_INVALID_ARGUMENT;
  if (n == 0 || N == 0 || n_columns == 0) return GSR_OK;
  if (!dst_rows || !src_rows || !columns) return GSR_ERR_INVALID_ARGUMENT;
  for (int c = 0; c < n_columns; ++c)
    if (!columns[c].data || columns[c].width_dwords <= 0 || columns[c].width_dwords > GSR_RELOC_MAX_WIDTH ||
        ((uintptr_t)columns[c].data & 3))
      return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}
