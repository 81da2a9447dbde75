// The MCMC controller's position noise: position[i] += R(q_i) (sigma_i * xi_i level_i) in place, xi_i from a counter-based
// generator keyed on (seed, step, i).  Per-row maths in gsr_controller.h.  No atomics, no LDS, no scratch: row i is a
// function of its own inputs, the seed, the step and i alone -- not of N, of the launch shape or of another row.
//
// mcmc_noise_kernel  a wave owns 256 consecutive rows, MN_ROWS slots of 64: lane l tests the rows 64 k + l -- it reads
//                    their points_in_view (int16) and alpha_logit, and a row that has too few views or whose level is 0,
//                    an opaque point, costs those 6 bytes and nothing else.  The rows that are left are then dealt out
//                    again: the wave's ballots give every lane the j-th live row in row order (j = lane, lane + 64, ...),
//                    so the row code runs once per 64 LIVE rows with every lane busy instead of once per slot with a
//                    few, and neighbouring lanes move neighbouring rows.  Which lane computes a row changes nothing: a
//                    row is a function of its own values.  A row that is not perturbed is never stored.
// mcmc_draws_kernel  one lane per row: the raw words and the normals of rows 0..N-1, for the tests that pin the generator.
#include "gsr_device.h"
#include "gsr_controller.h"
#include "gsr_host.h"

namespace {

constexpr int MN_BLOCK = 256;
constexpr int MN_ROWS = 4;                  // rows a lane tests: a wave owns 64 * MN_ROWS rows

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int W>
__device__ __forceinline__ void load_row(const float* __restrict__ src, int64_t r, float* v) {
#pragma unroll
  for (int k = 0; k < W; ++k) v[k] = src[r * W + k];
}

__global__ __launch_bounds__(MN_BLOCK) void mcmc_noise_kernel(float* __restrict__ position,
                                                              const float* __restrict__ log_scaling,
                                                              const float* __restrict__ rotation,
                                                              const float* __restrict__ alpha_logit,
                                                              const int16_t* __restrict__ points_in_view, int64_t N,
                                                              int min_views, float opacity_threshold, float margin,
                                                              float noise_level, float scale_eps, uint64_t seed,
                                                              uint64_t step) {
  const int lane = threadIdx.x & 63;
  const int64_t wave_row0 = ((int64_t)blockIdx.x * MN_BLOCK + (threadIdx.x - lane)) * MN_ROWS;
  if (wave_row0 >= N) return;               // (the whole wave)
  uint64_t mask[MN_ROWS];
#pragma unroll
  for (int k = 0; k < MN_ROWS; ++k) {
    const int64_t r = wave_row0 + 64 * k + lane;
    bool live = false;
    if (r < N && (int)points_in_view[r] > min_views)
      live = gsr_mcmc_level(alpha_logit[r], opacity_threshold, margin, noise_level) != 0.f;
    mask[k] = __ballot(live);
  }
  const int s1 = __popcll(mask[0]), s2 = s1 + __popcll(mask[1]), s3 = s2 + __popcll(mask[2]), total = s3 + __popcll(mask[3]);
  for (int j = lane; j < total; j += 64) {
    const int k = (j >= s1) + (j >= s2) + (j >= s3);
    const uint64_t m = k == 0 ? mask[0] : k == 1 ? mask[1] : k == 2 ? mask[2] : mask[3];
    const int first = k == 0 ? 0 : k == 1 ? s1 : k == 2 ? s2 : s3;
    const int64_t r = wave_row0 + 64 * k + gsr_nth_set_bit(m, j - first);      // a live row: r < N
    const float level = gsr_mcmc_level(alpha_logit[r], opacity_threshold, margin, noise_level);   // the bits tested above
    float p[3], ls[3], q[4];
    load_row<3>(log_scaling, r, ls);
    load_row<4>(rotation, r, q);
    load_row<3>(position, r, p);
    if (gsr_mcmc_noise_row(p, ls, q, level, scale_eps, (uint64_t)r, seed, step)) {
      position[3 * r] = p[0];
      position[3 * r + 1] = p[1];
      position[3 * r + 2] = p[2];
    }
  }
}

__global__ __launch_bounds__(MN_BLOCK) void mcmc_draws_kernel(int64_t N, uint64_t seed, uint64_t step,
                                                              uint32_t* __restrict__ words_out,
                                                              float* __restrict__ normals_out) {
  const int64_t i = (int64_t)blockIdx.x * MN_BLOCK + threadIdx.x;
  if (i >= N) return;
  uint32_t w[4];
  gsr_mcmc_words((uint64_t)i, seed, step, w);
  if (words_out) reinterpret_cast<uint4*>(words_out)[i] = make_uint4(w[0], w[1], w[2], w[3]);
  if (normals_out) {
    float z[4];
    gsr_mcmc_normals(w, z);
    normals_out[3 * i] = z[0];
    normals_out[3 * i + 1] = z[1];
    normals_out[3 * i + 2] = z[2];
  }
}

}  // namespace

extern "C" {

int gsr_mcmc_noise(float* position, const float* log_scaling, const float* rotation_xyzw, const float* alpha_logit,
                   const int16_t* points_in_view, int64_t N, int32_t min_views, float opacity_threshold, float margin,
                   float noise_level, float scale_eps, uint64_t seed, uint64_t step, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (N == 0) return GSR_OK;
  if (!position || !log_scaling || !rotation_xyzw || !alpha_logit || !points_in_view || N < 0 ||
      N > GSR_NEIGHBOURS_MAX_N || !(opacity_threshold > 0.f) || !(margin >= 0.f) || !(noise_level >= 0.f) ||
      !(scale_eps >= 0.f))
    return GSR_ERR_INVALID_ARGUMENT;
  mcmc_noise_kernel<<<grid_for(N, MN_BLOCK * MN_ROWS), MN_BLOCK, 0, stream>>>(
      position, log_scaling, rotation_xyzw, alpha_logit, points_in_view, N, (int)min_views, opacity_threshold, margin,
      noise_level, scale_eps, seed, step);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_mcmc_draws(int64_t N, uint64_t seed, uint64_t step, uint32_t* words_out, float* normals_out, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (N == 0 || (!words_out && !normals_out)) return GSR_OK;
  if (N < 0 || N > GSR_NEIGHBOURS_MAX_N || !aligned16(words_out)) return GSR_ERR_INVALID_ARGUMENT;
  mcmc_draws_kernel<<<grid_for(N, MN_BLOCK), MN_BLOCK, 0, stream>>>(N, seed, step, words_out, normals_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
