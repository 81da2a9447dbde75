// Direct least-squares SH export fit: per-point fp64 normal equations accumulated view by view, solved once.  Row layout
// and per-component maths in gsr_sh_fit.h.  No atomics, no scratch: the rows of one call are distinct and the calls of
// one stream are ordered, so the result is a function of the views and their order alone.
//
// sh_fit_accumulate_kernel  one read-modify-write of the M listed rows.  A row is up to 1480 contiguous bytes, so a lane
//                           per point would touch 64 different rows at once; instead SHF_GROUP = 16 lanes share a point
//                           (four points per wave) and lane l owns the components l, l + 16, ...: every load and store of
//                           a group is 128 contiguous bytes.  Every lane of a group evaluates the direction and the K basis
//                           values (cheap next to the row), the group leaves the K + 4 operands of its point in LDS, and a
//                           component reads its two operands from there by the constexpr table (a register array cannot be
//                           indexed by lane).  The camera position is a device pointer read through the scalar cache: no
//                           host wait.  An index outside [0, N) is skipped.
// sh_fit_solve_kernel       one wave per block, 16 lanes per point again: the row goes to LDS (R doubles per point),
//                           lane i owns row i of the triangle.  Column j of the factor: every lane i >= j forms the pivot
//                           and its own entry from the finished columns, barrier, writes, barrier.  The three right-hand
//                           sides stay in registers, one entry per lane and channel; a substitution step broadcasts entry
//                           j from its lane with a shuffle.  16 x 16 doubles per thread would not fit in registers.
#include "gsr_device.h"
#include "gsr_sh_fit.h"
#include "gsr_host.h"

namespace {

constexpr int SHF_GROUP = 16;                          // lanes per point
constexpr int SHF_ACC_BLOCK = 256;                     // 16 points
constexpr int SHF_SOLVE_BLOCK = 64;                    // 4 points, one wave: its barriers cost nothing

template <int K>
__global__ __launch_bounds__(SHF_ACC_BLOCK) void sh_fit_accumulate_kernel(
    const float* __restrict__ pos, int64_t N, const int64_t* __restrict__ idx, int64_t M, const float* __restrict__ col,
    const float* __restrict__ wts, const float* __restrict__ cam, double* __restrict__ acc) {
  constexpr int R = GsrShfTable<K>::R, NE = GsrShfTable<K>::E, POINTS = SHF_ACC_BLOCK / SHF_GROUP;
  static constexpr GsrShfTable<K> tab{};
  __shared__ double s_e[POINTS * NE];
  const int l = threadIdx.x % SHF_GROUP, g = threadIdx.x / SHF_GROUP;
  const int64_t m = (int64_t)blockIdx.x * POINTS + g;
  int64_t i = -1;
  float w = 0.f;
  if (m < M) {
    i = idx[m];
    w = wts[m];
  }
  const bool live = i >= 0 && i < N;
  if (live) {
    double e[NE];
    gsr_shf_operands<K>(pos + 3 * i, cam, col + 3 * m, e);
#pragma unroll
    for (int k = 0; k < NE; ++k)
      if (k % SHF_GROUP == l) s_e[g * NE + k] = e[k];
  }
  __syncthreads();
  if (!live) return;
  double* row = acc + i * R;
  const double* e = s_e + g * NE;
#pragma unroll
  for (int t = 0; t < (R + SHF_GROUP - 1) / SHF_GROUP; ++t) {
    const int j = t * SHF_GROUP + l;
    if (j < R) row[j] = gsr_shf_update(row[j], w, e[tab.a[j]], e[tab.b[j]]);
  }
}

template <int K>
__global__ __launch_bounds__(SHF_SOLVE_BLOCK) void sh_fit_solve_kernel(const double* __restrict__ acc, int64_t N,
                                                                        float ridge, float* __restrict__ sh,
                                                                        float* __restrict__ weight) {
  constexpr int T = GsrShfTable<K>::T, R = GsrShfTable<K>::R, POINTS = SHF_SOLVE_BLOCK / SHF_GROUP;
  __shared__ double s_rows[POINTS * R];
  const int l = threadIdx.x % SHF_GROUP, g = threadIdx.x / SHF_GROUP;
  const int64_t n = (int64_t)blockIdx.x * POINTS + g;
  const bool live = n < N;
  double* A = s_rows + g * R;
  if (live) {
    const double* row = acc + n * R;
    for (int j = l; j < R; j += SHF_GROUP) A[j] = row[j];
  }
  __syncthreads();
  const double W = live ? A[R - 1] : 0.0;
  const bool mine = W > 0.0 && l < K;                   // this lane owns row l of a point that was seen
  if (mine && l >= 1) A[gsr_shf_tri(l, l)] += gsr_shf_ridge_term(ridge, W);
  __syncthreads();
  for (int j = 0; j < K; ++j) {
    double v = 0.0;
    if (mine && l >= j) {
      const double d = sqrt(gsr_shf_chol_dot(A, j, j));
      v = l == j ? d : gsr_shf_chol_dot(A, l, j) / d;
    }
    __syncthreads();
    if (mine && l >= j) A[gsr_shf_tri(l, j)] = v;
    __syncthreads();
  }
  double b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) b[c] = mine ? A[T + c * K + l] : 0.0;
  for (int j = 0; j < K; ++j) {                         // L z = b
    const double d = mine ? A[gsr_shf_tri(j, j)] : 1.0;
    const double lij = mine && l > j ? A[gsr_shf_tri(l, j)] : 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double z = __shfl(b[c], j, SHF_GROUP) / d;
      b[c] = l == j ? z : (l > j ? gsr_shf_eliminate(b[c], lij, z) : b[c]);
    }
  }
  for (int j = K - 1; j >= 0; --j) {                    // L^T s = z
    const double d = mine ? A[gsr_shf_tri(j, j)] : 1.0;
    const double lji = mine && l < j ? A[gsr_shf_tri(j, l)] : 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = __shfl(b[c], j, SHF_GROUP) / d;
      b[c] = l == j ? x : (l < j ? gsr_shf_eliminate(b[c], lji, x) : b[c]);
    }
  }
  if (live && l < K) {
#pragma unroll
    for (int c = 0; c < 3; ++c) sh[(n * 3 + c) * K + l] = mine ? (float)b[c] : 0.f;
  }
  if (live && l == 0) weight[n] = (float)W;
}

}  // namespace

extern "C" {

int gsr_sh_fit_row_doubles(int32_t K) {
  return gsr_sh_degree_ok(K) ? gsr_shf_row_doubles(K) : 0;
}

int gsr_sh_fit_accumulate(const float* positions, int64_t N, const int64_t* indexes, int64_t M, const float* colors,
                          const float* weights, const float* camera_pos, int32_t K, double* acc, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!positions || !indexes || !colors || !weights || !camera_pos || !acc || N < 1 || N > GSR_NEIGHBOURS_MAX_N ||
      M < 1 || M > N || !gsr_sh_fit_row_doubles(K))
    return GSR_ERR_INVALID_ARGUMENT;
  const unsigned grid = grid_for(M, SHF_ACC_BLOCK / SHF_GROUP);
  gsr_pick_sh(K, [&](auto k) {
    sh_fit_accumulate_kernel<decltype(k)::value><<<grid, SHF_ACC_BLOCK, 0, stream>>>(positions, N, indexes, M, colors, weights,
                                                                                    camera_pos, acc);
  });
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_sh_fit_solve(const double* acc, int64_t N, int32_t K, float ridge, float* sh_out, float* weight_out,
                     void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!acc || !sh_out || !weight_out || N < 1 || N > GSR_NEIGHBOURS_MAX_N || !gsr_sh_fit_row_doubles(K) ||
      !(ridge >= GSR_SHF_MIN_RIDGE) || !(ridge < INFINITY))
    return GSR_ERR_INVALID_ARGUMENT;
  const unsigned grid = grid_for(N, SHF_SOLVE_BLOCK / SHF_GROUP);
  gsr_pick_sh(K, [&](auto k) {
    sh_fit_solve_kernel<decltype(k)::value><<<grid, SHF_SOLVE_BLOCK, 0, stream>>>(acc, N, ridge, sh_out, weight_out);
  });
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
