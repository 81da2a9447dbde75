// Mip-Splatting's 3-D smoothing filter: the per-point sampling rate over a camera table and the fused forward / backward
// of the smoothing itself.  Per-pair and per-row maths in gsr_filter3d.h.  No atomics, no LDS, no scratch: every result is
// a function of the inputs alone.
//
// sampling_rate_kernel     every lane keeps SR_PPL points and their running best (focal, depth) pair in registers; the
//                          cameras are wave-uniform and come through the scalar cache -- one 64-byte record and one
//                          focal each, SR_STEP per step of the sweep, in ascending order -- as in frustum_counts_kernel
//                          (visibility.hip).  One division per point at the end.
// filter3d_forward_kernel  one lane per F3_ROWS consecutive rows, read and written as float4 (a group that reaches past
// filter3d_backward_kernel N goes row by row); a row whose added variance is 0 is copied.  The backward recomputes the
//                          forward's terms from the inputs: nothing is saved between the two.
#include "gsr_device.h"
#include "gsr_filter3d.h"
#include "gsr_host.h"

namespace {

constexpr int F3_BLOCK = 256;
constexpr int SR_PPL = 4;                   // points per lane
constexpr int SR_STEP = 4;                  // cameras per step of the sweep
constexpr int F3_ROWS = 4;                  // rows per lane: 3 float4 of log_scaling, one each of alpha_logit and rate

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__global__ __launch_bounds__(F3_BLOCK) void sampling_rate_kernel(const float* __restrict__ p, int N,
                                                                  const float* __restrict__ rec,
                                                                  const float* __restrict__ focal, int V, float margin,
                                                                  float* __restrict__ rate) {
  const int64_t base = (int64_t)blockIdx.x * (F3_BLOCK * SR_PPL) + threadIdx.x;
  float x[SR_PPL], y[SR_PPL], z[SR_PPL], bf[SR_PPL], bd[SR_PPL];
#pragma unroll
  for (int u = 0; u < SR_PPL; ++u) {
    const int64_t i = base + (int64_t)u * F3_BLOCK;
    const bool live = i < N;
    const int64_t q = live ? i : (int64_t)N - 1;
    x[u] = live ? p[3 * q] : NAN;              // a lane past N holds a NaN point: sampled by no camera
    y[u] = p[3 * q + 1];
    z[u] = p[3 * q + 2];
    bf[u] = 0.f;
    bd[u] = 1.f;
  }
  int c = 0;
  for (; c + SR_STEP <= V; c += SR_STEP) {
#pragma unroll
    for (int s = 0; s < SR_STEP; ++s) {
      const float* r = rec + (int64_t)GSR_VIS_RECORD_FLOATS * (c + s);
      const float f = focal[c + s];
#pragma unroll
      for (int u = 0; u < SR_PPL; ++u) gsr_f3d_pair(r, f, margin, x[u], y[u], z[u], &bf[u], &bd[u]);
    }
  }
  for (; c < V; ++c) {
    const float* r = rec + (int64_t)GSR_VIS_RECORD_FLOATS * c;
    const float f = focal[c];
#pragma unroll
    for (int u = 0; u < SR_PPL; ++u) gsr_f3d_pair(r, f, margin, x[u], y[u], z[u], &bf[u], &bd[u]);
  }
#pragma unroll
  for (int u = 0; u < SR_PPL; ++u) {
    const int64_t i = base + (int64_t)u * F3_BLOCK;
    if (i < N) rate[i] = gsr_f3d_rate(bf[u], bd[u]);
  }
}

// F3_ROWS rows of a [N, W] float32 array starting at row r0, as float4 when the whole group is inside the array.
template <int W>
__device__ __forceinline__ void load_rows(const float* __restrict__ src, int64_t r0, int64_t N, float* v) {
  constexpr int n = F3_ROWS * W;
  if (r0 + F3_ROWS <= N) {
    const float4* s4 = reinterpret_cast<const float4*>(src + r0 * W);
#pragma unroll
    for (int q = 0; q < n / 4; ++q) {
      const float4 t = s4[q];
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < n; ++k) v[k] = r0 + k / W < N ? src[r0 * W + k] : 0.f;
  }
}

template <int W>
__device__ __forceinline__ void store_rows(float* __restrict__ dst, int64_t r0, int64_t N, const float* v) {
  constexpr int n = F3_ROWS * W;
  if (r0 + F3_ROWS <= N) {
    float4* d4 = reinterpret_cast<float4*>(dst + r0 * W);
#pragma unroll
    for (int q = 0; q < n / 4; ++q) d4[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < n; ++k)
      if (r0 + k / W < N) dst[r0 * W + k] = v[k];
  }
}

__global__ __launch_bounds__(F3_BLOCK) void filter3d_forward_kernel(const float* __restrict__ log_scaling,
                                                                     const float* __restrict__ alpha_logit,
                                                                     const float* __restrict__ rate, int64_t N,
                                                                     float strength, float* __restrict__ out_ls,
                                                                     float* __restrict__ out_a) {
  const int64_t r0 = ((int64_t)blockIdx.x * F3_BLOCK + threadIdx.x) * F3_ROWS;
  if (r0 >= N) return;
  float ls[F3_ROWS * 3], a[F3_ROWS], rt[F3_ROWS];
  load_rows<3>(log_scaling, r0, N, ls);
  load_rows<1>(alpha_logit, r0, N, a);
  load_rows<1>(rate, r0, N, rt);
#pragma unroll
  for (int k = 0; k < F3_ROWS; ++k) {
    const float c = gsr_f3d_variance(rt[k], strength);
    if (c != 0.f) gsr_f3d_forward_row(ls + 3 * k, a[k], c, ls + 3 * k, a + k);
  }
  store_rows<3>(out_ls, r0, N, ls);
  store_rows<1>(out_a, r0, N, a);
}

__global__ __launch_bounds__(F3_BLOCK) void filter3d_backward_kernel(const float* __restrict__ log_scaling,
                                                                      const float* __restrict__ alpha_logit,
                                                                      const float* __restrict__ rate, int64_t N,
                                                                      float strength, const float* __restrict__ g_ls,
                                                                      const float* __restrict__ g_a,
                                                                      float* __restrict__ d_ls, float* __restrict__ d_a) {
  const int64_t r0 = ((int64_t)blockIdx.x * F3_BLOCK + threadIdx.x) * F3_ROWS;
  if (r0 >= N) return;
  float ls[F3_ROWS * 3], a[F3_ROWS], rt[F3_ROWS], gl[F3_ROWS * 3], ga[F3_ROWS];
  load_rows<3>(log_scaling, r0, N, ls);
  load_rows<1>(alpha_logit, r0, N, a);
  load_rows<1>(rate, r0, N, rt);
  load_rows<3>(g_ls, r0, N, gl);
  load_rows<1>(g_a, r0, N, ga);
#pragma unroll
  for (int k = 0; k < F3_ROWS; ++k) {
    const float c = gsr_f3d_variance(rt[k], strength);
    if (c != 0.f) gsr_f3d_backward_row(ls + 3 * k, a[k], c, gl + 3 * k, ga[k], gl + 3 * k, ga + k);
  }
  store_rows<3>(d_ls, r0, N, gl);
  store_rows<1>(d_a, r0, N, ga);
}

}  // namespace

extern "C" {

int gsr_sampling_rate(const float* points, int64_t N, const float* records, const float* focal, int64_t V, float margin,
                      float* rate_out, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!points || !records || !focal || !rate_out || N < 1 || N > GSR_NEIGHBOURS_MAX_N || V < 1 ||
      V > GSR_VISIBILITY_MAX_CAMERAS || !(margin >= 0.f))
    return GSR_ERR_INVALID_ARGUMENT;
  sampling_rate_kernel<<<grid_for(N, F3_BLOCK * SR_PPL), F3_BLOCK, 0, stream>>>(points, (int)N, records, focal, (int)V,
                                                                                margin, rate_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_filter3d_forward(const float* log_scaling, const float* alpha_logit, const float* rate, int64_t N, float strength,
                         float* out_log_scaling, float* out_alpha_logit, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!log_scaling || !alpha_logit || !rate || !out_log_scaling || !out_alpha_logit || N < 1 ||
      N > GSR_NEIGHBOURS_MAX_N || !(strength >= 0.f))
    return GSR_ERR_INVALID_ARGUMENT;
  if (!aligned16(log_scaling) || !aligned16(alpha_logit) || !aligned16(rate) || !aligned16(out_log_scaling) ||
      !aligned16(out_alpha_logit))
    return GSR_ERR_INVALID_ARGUMENT;
  filter3d_forward_kernel<<<grid_for(N, F3_BLOCK * F3_ROWS), F3_BLOCK, 0, stream>>>(
      log_scaling, alpha_logit, rate, N, strength, out_log_scaling, out_alpha_logit);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_filter3d_backward(const float* log_scaling, const float* alpha_logit, const float* rate, int64_t N, float strength,
                          const float* d_out_log_scaling, const float* d_out_alpha_logit, float* d_log_scaling,
                          float* d_alpha_logit, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!log_scaling || !alpha_logit || !rate || !d_out_log_scaling || !d_out_alpha_logit || !d_log_scaling ||
      !d_alpha_logit || N < 1 || N > GSR_NEIGHBOURS_MAX_N || !(strength >= 0.f))
    return GSR_ERR_INVALID_ARGUMENT;
  if (!aligned16(log_scaling) || !aligned16(alpha_logit) || !aligned16(rate) || !aligned16(d_out_log_scaling) ||
      !aligned16(d_out_alpha_logit) || !aligned16(d_log_scaling) || !aligned16(d_alpha_logit))
    return GSR_ERR_INVALID_ARGUMENT;
  filter3d_backward_kernel<<<grid_for(N, F3_BLOCK * F3_ROWS), F3_BLOCK, 0, stream>>>(
      log_scaling, alpha_logit, rate, N, strength, d_out_log_scaling, d_out_alpha_logit, d_log_scaling, d_alpha_logit);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
