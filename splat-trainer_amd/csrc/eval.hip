// Evaluation pass (trainer/evaluation.py Evaluation, util/colors.py fit_colors_batch): the iterative affine-quadratic
// colour fit of a rendering to its photograph, and the three image metrics of one image in one call.
//
// Colour fit.  The torch form solves 3 x num_iters least-squares problems on a (pixels x 10) matrix; here one pass
// kernel runs num_iters + 1 times and sums the normal equations instead (gsr_eval.h: 35 + 10 fp64 sums per channel):
//   pass k   reads x0, iterate k-1 and ref; applies warp k-1 (pass 0 copies x0); writes iterate k (fp32); except on the
//            last pass accumulates the moments of iterate k over the pixels unclipped in x0, iterate k and ref
//   finish   one block adds the per-block slots in block order, solves the three 10 x 10 systems (one lane each) and
//            leaves the 30 weights (fp64) on the device for pass k+1
// The host is not involved between passes.  Grid: min(ceil(P / 256), 1024) x 3 blocks of 256, blockIdx.y = the channel
// whose moments the block sums and whose iterate it writes (45 fp64 accumulators per thread, no scratch); a thread takes
// its pixels in ascending order, a wave adds its lanes in a fixed shuffle tree, the four waves are added in order into
// the block's slot.  Nothing is atomic: two runs give the same bits.
#include "gsr_device.h"
#include "gsr_eval.h"
#include "gsr_host.h"

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_MAX_BLOCKS = 1024;
constexpr int EV_MAX_ITERS = 64;

inline int ev_blocks(int64_t P) {
  const int64_t want = (P + EV_THREADS - 1) / EV_THREADS;
  return (int)(want < EV_MAX_BLOCKS ? want : EV_MAX_BLOCKS);
}

// total of the wave's 64 lanes in lane 0: v[l] += v[l + off] for off = 32, 16, .., 1 (a fixed tree)
__device__ __forceinline__ double ev_wave_sum_to_lane0(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__global__ __launch_bounds__(EV_THREADS) void color_fit_pass_kernel(const float* __restrict__ x0,
                                                                    const float* __restrict__ prev,
                                                                    const float* __restrict__ ref,
                                                                    float* __restrict__ next,
                                                                    const double* __restrict__ weights, int64_t P,
                                                                    float lo, float hi, int accumulate,
                                                                    double* __restrict__ slots) {
  __shared__ double s_w[3 * GSR_EV_COLS];
  __shared__ double s_part[EV_THREADS / 64][GSR_EV_SUMS];
  const int c = blockIdx.y;
  if (weights) {
    if (threadIdx.x < 3 * GSR_EV_COLS) s_w[threadIdx.x] = weights[threadIdx.x];
    __syncthreads();
  }
  double acc[GSR_EV_SUMS];
#pragma unroll
  for (int k = 0; k < GSR_EV_SUMS; ++k) acc[k] = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x; p < P; p += (int64_t)gridDim.x * EV_THREADS) {
    const int64_t o = 3 * p;
    float x[3] = {prev[o], prev[o + 1], prev[o + 2]};
    double a[GSR_EV_COLS];
    if (weights) {
      gsr_ev_row(x[0], x[1], x[2], a);
#pragma unroll
      for (int k = 0; k < 3; ++k) x[k] = gsr_ev_warp(a, s_w + GSR_EV_COLS * k);
    }
    const float xc = c == 0 ? x[0] : (c == 1 ? x[1] : x[2]);
    next[o + c] = xc;
    if (accumulate) {
      const float rc = ref[o + c];
      if (gsr_ev_unclipped(x0[o + c], lo, hi) && gsr_ev_unclipped(xc, lo, hi) && gsr_ev_unclipped(rc, lo, hi)) {
        gsr_ev_row(x[0], x[1], x[2], a);
        gsr_ev_accumulate(a, (double)rc, acc);
      }
    }
  }
  if (!accumulate) return;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < GSR_EV_SUMS; ++k) {
    const double v = ev_wave_sum_to_lane0(acc[k]);
    if (gsr_lane() == 0) s_part[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < GSR_EV_SUMS)
    slots[((int64_t)c * gridDim.x + blockIdx.x) * GSR_EV_SUMS + threadIdx.x] =
        ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
}

// slots [3][blocks][45] -> weights [3][10]
__global__ __launch_bounds__(EV_THREADS) void color_fit_finish_kernel(const double* __restrict__ slots, int blocks,
                                                                      double* __restrict__ weights) {
  __shared__ double s_sums[3][GSR_EV_SUMS];
  __shared__ double s_work[3][GSR_EV_WORK];
  if (threadIdx.x < 3 * GSR_EV_SUMS) {
    const int c = threadIdx.x / GSR_EV_SUMS, k = threadIdx.x % GSR_EV_SUMS;
    double acc = 0.0;
    for (int b = 0; b < blocks; ++b) acc += slots[((int64_t)c * blocks + b) * GSR_EV_SUMS + k];
    s_sums[c][k] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 3) gsr_ev_solve(s_sums[threadIdx.x], s_work[threadIdx.x], weights + GSR_EV_COLS * threadIdx.x);
}

struct FitPlan {          // byte offsets into the workspace
  size_t other, slots, weights, total;
};

FitPlan fit_plan(int64_t P) {
  FitPlan p;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 255) / 256 * 256; return o; };
  p.other = take((size_t)P * 3 * sizeof(float));
  p.slots = take((size_t)3 * ev_blocks(P) * GSR_EV_SUMS * sizeof(double));
  p.weights = take((size_t)3 * GSR_EV_COLS * sizeof(double));
  p.total = at;
  return p;
}

struct MetricsPlan {
  size_t ssim, mse, l1, total;
};

MetricsPlan metrics_plan(int32_t H, int32_t W) {
  MetricsPlan p;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 255) / 256 * 256; return o; };
  p.ssim = take(gsr_ssim_workspace_bytes(1, 3, H, W));
  p.mse = take(gsr_pixel_loss_workspace_bytes((int64_t)H * W * 3));
  p.l1 = take(gsr_pixel_loss_workspace_bytes((int64_t)H * W * 3));
  p.total = at;
  return p;
}

}  // namespace

extern "C" {

size_t gsr_color_fit_workspace_bytes(int64_t P) {
  if (P <= 0) return 256;
  return fit_plan(P).total + 256;
}

int gsr_color_fit(const float* image, const float* ref, int64_t P, int32_t num_iters, float eps, float* out,
                  void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (P <= 0 || !image || !ref || !out || out == image || out == ref || num_iters < 0 || num_iters > EV_MAX_ITERS ||
      !(eps >= 0.f && eps < 0.5f))
    return GSR_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < gsr_color_fit_workspace_bytes(P)) return GSR_ERR_WORKSPACE_TOO_SMALL;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return GSR_ERR_INVALID_ARGUMENT;
  uint8_t* base = reinterpret_cast<uint8_t*>(workspace);
  const FitPlan plan = fit_plan(P);
  float* other = reinterpret_cast<float*>(base + plan.other);
  double* slots = reinterpret_cast<double*>(base + plan.slots);
  double* weights = reinterpret_cast<double*>(base + plan.weights);
  const int blocks = ev_blocks(P);
  const dim3 grid(blocks, 3);
  const float lo = eps, hi = (float)(1.0 - (double)eps);
  const float* prev = image;
  for (int k = 0; k <= num_iters; ++k) {
    float* next = ((num_iters - k) & 1) ? other : out;          // the iterates alternate; the last one lands in `out`
    const int accumulate = k < num_iters ? 1 : 0;
    color_fit_pass_kernel<<<grid, EV_THREADS, 0, stream>>>(image, prev, ref, next, k ? weights : nullptr, P, lo, hi,
                                                          accumulate, slots);
    GSR_CHECK_LAUNCH();
    if (accumulate) {
      color_fit_finish_kernel<<<1, EV_THREADS, 0, stream>>>(slots, blocks, weights);
      GSR_CHECK_LAUNCH();
    }
    prev = next;
  }
  return GSR_OK;
}

size_t gsr_image_metrics_workspace_bytes(int32_t H, int32_t W) {
  if (H <= 0 || W <= 0) return 256;
  return metrics_plan(H, W).total + 256;
}

int gsr_image_metrics(const float* image, const float* source, int32_t H, int32_t W, float* metrics_out,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (H <= 10 || W <= 10 || !image || !source || !metrics_out) return GSR_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < gsr_image_metrics_workspace_bytes(H, W)) return GSR_ERR_WORKSPACE_TOO_SMALL;
  uint8_t* base = reinterpret_cast<uint8_t*>(workspace);
  const MetricsPlan plan = metrics_plan(H, W);
  const int64_t n = (int64_t)H * W * 3;
  const float none = 3.0e38f;                                   // no clamp: Evaluation uses plain mse_loss / l1_loss
  int rc = gsr_pixel_loss_forward(image, source, n, 0, -none, none, metrics_out, base + plan.mse,
                                  gsr_pixel_loss_workspace_bytes(n), stream);
  if (rc != GSR_OK) return rc;
  rc = gsr_pixel_loss_forward(image, source, n, 1, -none, none, metrics_out + 1, base + plan.l1,
                              gsr_pixel_loss_workspace_bytes(n), stream);
  if (rc != GSR_OK) return rc;
  const int64_t strides[4] = {0, 1, (int64_t)W * 3, 3};         // the (H, W, 3) image seen as one batch of 3 planes
  return gsr_ssim_forward(image, source, strides, strides, 1, 3, H, W, 5, metrics_out + 2, nullptr, nullptr, nullptr,
                          base + plan.ssim, gsr_ssim_workspace_bytes(1, 3, H, W), stream);
}

}  // extern "C"
