// Normal consistency: camera-space splat normals, normals of a depth image and the fused depth-normal consistency loss
// with its backward.  The arithmetic and the contract are in gsr_normals.h, the entry points in include/gsplat_hip.h.
//
// splat_normals_forward_kernel / _backward_kernel.  One thread per visible row; the camera's 16 floats are wave-uniform.
//   The forward writes rows of 3 floats, or [n, depth, 1] rows of 5 (the feature rows of the geometry image); the
//   backward recomputes the forward's terms and writes row indexes[m] of d_rotation: the indexes are unique, one writer.
// pixel_normals_kernel<LOSS>.  256 threads own a tile of 32 x 8 pixels.  The tile's depths and a ring of one pixel go
//   through LDS (34 x 10 floats), so a depth is read from memory 1.33 times, not 5.  LOSS = false reads a plain depth
//   map; LOSS = true reads the geometry image [H, W, 5] and forms D / A.  A pixel of G is 20 bytes: a wave's two rows of
//   32 pixels are two runs of 640 bytes, five cache lines each, which the five per-channel loads of a lane walk with a
//   20-byte stride -- every line comes from memory once and is touched by up to five instructions.  A row of 32 pixels
//   starts on a 16-byte boundary only where W is a multiple of 4, so the image is not staged through LDS as float4.
//   With LOSS the block's l are added in a fixed order (wave sum by DPP, the four waves' sums handed off through
//   gsr_device.h and added as ((w0 + w1) + w2) + w3) into partials[block].
// normal_loss_finish_kernel.  One block: thread t adds partials t, t + 256, ... in ascending order, then the same block
//   sum; L = total / (H W).  Two runs give the same bits.
// normal_loss_backward_kernel.  The same tile.  Depths with a ring of two (36 x 12) are staged; then every pixel of the
//   tile and a ring of one (340, two per thread at most) evaluates ITS OWN stencil once and leaves n_d, U and V in LDS;
//   then each tile pixel gathers from its left, right, up and down neighbour, in that order.  Nothing is read from the
//   forward: it recomputes.  No atomics, no scratch, one writer per element, plain vector stores.
#include "gsr_device.h"
#include "gsr_host.h"
#include "gsr_normals.h"

namespace {

constexpr int NB = 256;            // threads per block
constexpr int TW = 32, TH = 8;     // the tile: a wave holds two rows of 32 pixels
constexpr int NRM_MAX_SIDE = 32768;

__global__ __launch_bounds__(NB) void splat_normals_forward_kernel(const float* __restrict__ rotation,
                                                                   const float* __restrict__ log_scaling,
                                                                   const float* __restrict__ position, int64_t N,
                                                                   const int64_t* __restrict__ indexes, int64_t M,
                                                                   const float* __restrict__ T_camera_world,
                                                                   const float* __restrict__ depth,
                                                                   float* __restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * NB + threadIdx.x;
  if (m >= M) return;
  const int64_t i = indexes[m];
  float n[3] = {0.f, 0.f, 0.f};
  if ((uint64_t)i < (uint64_t)N) {                     // a row outside the scene gets the normal 0
    const float4 q = reinterpret_cast<const float4*>(rotation)[i];
    const float rot[4] = {q.x, q.y, q.z, q.w};
    const float ls[3] = {log_scaling[3 * i], log_scaling[3 * i + 1], log_scaling[3 * i + 2]};
    const float pos[3] = {position[3 * i], position[3 * i + 1], position[3 * i + 2]};
    float T[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) T[j] = T_camera_world[j];
    const GsrSplatNormal s = gsr_nrm_splat(rot, ls, pos, T);
    n[0] = s.n[0]; n[1] = s.n[1]; n[2] = s.n[2];
  }
  if (depth) {
    float* o = out + 5 * m;
    o[0] = n[0]; o[1] = n[1]; o[2] = n[2]; o[3] = depth[m]; o[4] = 1.f;
  } else {
    float* o = out + 3 * m;
    o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
  }
}

__global__ __launch_bounds__(NB) void splat_normals_backward_kernel(const float* __restrict__ rotation,
                                                                    const float* __restrict__ log_scaling,
                                                                    const float* __restrict__ position, int64_t N,
                                                                    const int64_t* __restrict__ indexes, int64_t M,
                                                                    const float* __restrict__ T_camera_world,
                                                                    const float* __restrict__ d_out, int stride,
                                                                    float* __restrict__ d_rotation,
                                                                    float* __restrict__ d_depth) {
  const int64_t m = (int64_t)blockIdx.x * NB + threadIdx.x;
  if (m >= M) return;
  const float* g = d_out + (int64_t)stride * m;
  if (d_depth) d_depth[m] = g[3];
  const int64_t i = indexes[m];
  if ((uint64_t)i >= (uint64_t)N) return;
  const float4 q = reinterpret_cast<const float4*>(rotation)[i];
  const float rot[4] = {q.x, q.y, q.z, q.w};
  const float ls[3] = {log_scaling[3 * i], log_scaling[3 * i + 1], log_scaling[3 * i + 2]};
  const float pos[3] = {position[3 * i], position[3 * i + 1], position[3 * i + 2]};
  float T[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) T[j] = T_camera_world[j];
  const GsrSplatNormal s = gsr_nrm_splat(rot, ls, pos, T);
  const float g_n[3] = {g[0], g[1], g[2]};
  float d[4];
  gsr_nrm_splat_backward(s, T, g_n, d);
  reinterpret_cast<float4*>(d_rotation)[i] = make_float4(d[0], d[1], d[2], d[3]);
}

// The depth of pixel (x, y) as the stencils read it; 0 (not valid) outside the image.
template <bool LOSS>
__device__ __forceinline__ float depth_at(const float* __restrict__ src, int x, int y, int W, int H, float alpha_min) {
  if (x < 0 || y < 0 || x >= W || y >= H) return 0.f;
  const int64_t p = (int64_t)y * W + x;
  if (!LOSS) return src[p];
  return gsr_nrm_expected_depth(src[5 * p + 3], src[5 * p + 4], alpha_min);
}

// Depths of the tile at (x0, y0) and a ring of R pixels -> s_d, rows of TW + 2 R floats.
template <bool LOSS, int R>
__device__ __forceinline__ void stage_depths(const float* __restrict__ src, int x0, int y0, int W, int H, float alpha_min,
                                             float* s_d) {
  constexpr int SW = TW + 2 * R, SH = TH + 2 * R;
  for (int i = threadIdx.x; i < SW * SH; i += NB) {
    const int hx = i % SW, hy = i / SW;
    s_d[i] = depth_at<LOSS>(src, x0 - R + hx, y0 - R + hy, W, H, alpha_min);
  }
  __syncthreads();
}

// The stencil of image pixel (x, y), whose depth is s_d[at] in rows of `pitch` floats.
__device__ __forceinline__ GsrNrmStencil stencil_at(const float* s_d, int at, int pitch, int x, int y, int W, int H,
                                                    float fx, float fy, float cx, float cy) {
  const bool interior = x >= 1 && y >= 1 && x <= W - 2 && y <= H - 2;
  GsrNrmStencil s = gsr_nrm_stencil(gsr_nrm_ray(fx, cx, x - 1), gsr_nrm_ray(fx, cx, x), gsr_nrm_ray(fx, cx, x + 1),
                                    gsr_nrm_ray(fy, cy, y - 1), gsr_nrm_ray(fy, cy, y), gsr_nrm_ray(fy, cy, y + 1),
                                    interior ? s_d[at] : 0.f, s_d[at - 1], s_d[at + 1], s_d[at - pitch], s_d[at + pitch]);
  return s;
}

template <bool LOSS>
__global__ __launch_bounds__(NB) void pixel_normals_kernel(const float* __restrict__ src, int H, int W,
                                                           const float* __restrict__ projection, float alpha_min,
                                                           float* __restrict__ normals_out,
                                                           float* __restrict__ partials) {
  constexpr int P = TW + 2;
  __shared__ float s_d[P * (TH + 2)];
  const int tid = threadIdx.x, tx = tid & (TW - 1), ty = tid >> 5;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, x = x0 + tx, y = y0 + ty;
  stage_depths<LOSS, 1>(src, x0, y0, W, H, alpha_min, s_d);
  const float fx = projection[0], fy = projection[1], cx = projection[2], cy = projection[3];
  const bool inside = x < W && y < H;
  float l = 0.f;
  if (inside) {
    const GsrNrmStencil s = stencil_at(s_d, (ty + 1) * P + tx + 1, P, x, y, W, H, fx, fy, cx, cy);
    const int64_t p = (int64_t)y * W + x;
    float* o = normals_out + 3 * p;
    o[0] = s.n[0]; o[1] = s.n[1]; o[2] = s.n[2];
    if (LOSS && s.valid) {
      const float N[3] = {src[5 * p], src[5 * p + 1], src[5 * p + 2]};
      l = gsr_nrm_pixel_loss(N, src[5 * p + 4], s.n);
    }
  }
  if (LOSS) {
    const int wave = tid >> 6;
    const GsrWaves<float>& w = gsr_block_handoff<63>(gsr_wave_sum_to_lane63(l), wave);
    if (tid == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
  }
}

__global__ __launch_bounds__(NB) void normal_loss_finish_kernel(const float* __restrict__ partials, int64_t blocks,
                                                                float pixels, float* __restrict__ loss_out) {
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < blocks; i += NB) acc += partials[i];
  const int wave = threadIdx.x >> 6;
  const GsrWaves<float>& w = gsr_block_handoff<63>(gsr_wave_sum_to_lane63(acc), wave);
  if (threadIdx.x == 0) loss_out[0] = (((w[0] + w[1]) + w[2]) + w[3]) / pixels;
}

__global__ __launch_bounds__(NB) void normal_loss_backward_kernel(const float* __restrict__ G, int H, int W,
                                                                  const float* __restrict__ projection, float alpha_min,
                                                                  const float* __restrict__ d_loss,
                                                                  float* __restrict__ d_G) {
  constexpr int PD = TW + 4;                          // pitch of the depths (ring of two)
  constexpr int PQ = TW + 2, NQ = PQ * (TH + 2);      // pitch and count of the stencils (ring of one)
  __shared__ float s_d[PD * (TH + 4)];
  __shared__ float s_q[9][NQ];                        // n_d (0 where not valid), U, V of each stencil
  const int tid = threadIdx.x, tx = tid & (TW - 1), ty = tid >> 5;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, x = x0 + tx, y = y0 + ty;
  stage_depths<true, 2>(G, x0, y0, W, H, alpha_min, s_d);
  const float fx = projection[0], fy = projection[1], cx = projection[2], cy = projection[3];
  const float g = d_loss[0] / ((float)H * (float)W);
  for (int i = tid; i < NQ; i += NB) {
    const int hx = i % PQ, hy = i / PQ, qx = x0 - 1 + hx, qy = y0 - 1 + hy;
    float r[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (qx >= 1 && qy >= 1 && qx <= W - 2 && qy <= H - 2) {
      const GsrNrmStencil s = stencil_at(s_d, (hy + 1) * PD + hx + 1, PD, qx, qy, W, H, fx, fy, cx, cy);
      if (s.valid) {
        const int64_t q = (int64_t)qy * W + qx;
        const float N[3] = {G[5 * q], G[5 * q + 1], G[5 * q + 2]};
        r[0] = s.n[0]; r[1] = s.n[1]; r[2] = s.n[2];
        gsr_nrm_stencil_backward(s, N, g, r + 3, r + 6);
      }
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) s_q[j][i] = r[j];
  }
  __syncthreads();
  if (x >= W || y >= H) return;
  const int at = (ty + 1) * PQ + tx + 1;
  const float rx = gsr_nrm_ray(fx, cx, x), ry = gsr_nrm_ray(fy, cy, y);
  const float left = (rx * s_q[3][at - 1] + ry * s_q[4][at - 1]) + s_q[5][at - 1];
  const float right = (rx * s_q[3][at + 1] + ry * s_q[4][at + 1]) + s_q[5][at + 1];
  const float up = (rx * s_q[6][at - PQ] + ry * s_q[7][at - PQ]) + s_q[8][at - PQ];
  const float down = (rx * s_q[6][at + PQ] + ry * s_q[7][at + PQ]) + s_q[8][at + PQ];
  const float gd = ((left - right) + up) - down;
  const bool valid = s_q[0][at] != 0.f || s_q[1][at] != 0.f || s_q[2][at] != 0.f;      // a unit vector, or 0
  const int64_t p = (int64_t)y * W + x;
  float dD = 0.f, dA = valid ? g : 0.f;
  if (gd != 0.f) {                                    // then this pixel is a tap of a valid one: A >= alpha_min, d valid
    dD = gd / G[5 * p + 4];
    dA -= dD * s_d[(ty + 2) * PD + tx + 2];
  }
  float* o = d_G + 5 * p;
  o[0] = valid ? -g * s_q[0][at] : 0.f;
  o[1] = valid ? -g * s_q[1][at] : 0.f;
  o[2] = valid ? -g * s_q[2][at] : 0.f;
  o[3] = dD;
  o[4] = dA;
}

}  // namespace

extern "C" {

int gsr_splat_normals_forward(const float* rotation_xyzw, const float* log_scaling, const float* position, int64_t N,
                              const int64_t* indexes, int64_t M, const float* T_camera_world, const float* depth,
                              float* out, void* stream_) {
  if (M < 0 || N < 0 || M > GSR_NEIGHBOURS_MAX_N || N > GSR_NEIGHBOURS_MAX_N) return GSR_ERR_INVALID_ARGUMENT;
  if (M == 0) return GSR_OK;
  if (!rotation_xyzw || !log_scaling || !position || !indexes || !T_camera_world || !out) return GSR_ERR_INVALID_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(rotation_xyzw) & 15) return GSR_ERR_INVALID_ARGUMENT;
  splat_normals_forward_kernel<<<grid_for(M, NB), NB, 0, gsr_stream(stream_)>>>(rotation_xyzw, log_scaling, position, N,
                                                                               indexes, M, T_camera_world, depth, out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_splat_normals_backward(const float* rotation_xyzw, const float* log_scaling, const float* position, int64_t N,
                               const int64_t* indexes, int64_t M, const float* T_camera_world, const float* d_out,
                               int32_t stride, float* d_rotation, float* d_depth, void* stream_) {
  if (M < 0 || N < 0 || M > GSR_NEIGHBOURS_MAX_N || N > GSR_NEIGHBOURS_MAX_N || (stride != 3 && stride != 5))
    return GSR_ERR_INVALID_ARGUMENT;
  if (d_depth && stride != 5) return GSR_ERR_INVALID_ARGUMENT;
  if (M == 0) return GSR_OK;
  if (!rotation_xyzw || !log_scaling || !position || !indexes || !T_camera_world || !d_out || !d_rotation)
    return GSR_ERR_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(rotation_xyzw) | reinterpret_cast<uintptr_t>(d_rotation)) & 15)
    return GSR_ERR_INVALID_ARGUMENT;
  splat_normals_backward_kernel<<<grid_for(M, NB), NB, 0, gsr_stream(stream_)>>>(
      rotation_xyzw, log_scaling, position, N, indexes, M, T_camera_world, d_out, stride, d_rotation, d_depth);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_depth_normals(const float* depth, int32_t H, int32_t W, const float* projection, float* normals_out,
                      void* stream_) {
  if (H < 0 || W < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (H > NRM_MAX_SIDE || W > NRM_MAX_SIDE) return GSR_ERR_UNSUPPORTED;
  if (H == 0 || W == 0) return GSR_OK;
  if (!depth || !projection || !normals_out) return GSR_ERR_INVALID_ARGUMENT;
  const dim3 grid(grid_for(W, TW), grid_for(H, TH));
  pixel_normals_kernel<false><<<grid, NB, 0, gsr_stream(stream_)>>>(depth, H, W, projection, 0.f, normals_out, nullptr);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int64_t gsr_normal_loss_blocks(int32_t H, int32_t W) {
  if (H <= 0 || W <= 0 || H > NRM_MAX_SIDE || W > NRM_MAX_SIDE) return 0;
  return (int64_t)grid_for(W, TW) * grid_for(H, TH);
}

int gsr_normal_loss_forward(const float* geometry, int32_t H, int32_t W, const float* projection, float alpha_min,
                            float* normals_out, float* partials, float* loss_out, void* stream_) {
  if (H < 0 || W < 0 || !(alpha_min == alpha_min)) return GSR_ERR_INVALID_ARGUMENT;
  if (H > NRM_MAX_SIDE || W > NRM_MAX_SIDE) return GSR_ERR_UNSUPPORTED;
  if (H == 0 || W == 0) return GSR_OK;
  if (!geometry || !projection || !normals_out || !partials || !loss_out) return GSR_ERR_INVALID_ARGUMENT;
  hipStream_t stream = gsr_stream(stream_);
  const dim3 grid(grid_for(W, TW), grid_for(H, TH));
  pixel_normals_kernel<true><<<grid, NB, 0, stream>>>(geometry, H, W, projection, alpha_min, normals_out, partials);
  GSR_CHECK_LAUNCH();
  normal_loss_finish_kernel<<<1, NB, 0, stream>>>(partials, (int64_t)grid.x * grid.y, (float)H * (float)W, loss_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_normal_loss_backward(const float* geometry, int32_t H, int32_t W, const float* projection, float alpha_min,
                             const float* d_loss, float* d_geometry, void* stream_) {
  if (H < 0 || W < 0 || !(alpha_min == alpha_min)) return GSR_ERR_INVALID_ARGUMENT;
  if (H > NRM_MAX_SIDE || W > NRM_MAX_SIDE) return GSR_ERR_UNSUPPORTED;
  if (H == 0 || W == 0) return GSR_OK;
  if (!geometry || !projection || !d_loss || !d_geometry) return GSR_ERR_INVALID_ARGUMENT;
  const dim3 grid(grid_for(W, TW), grid_for(H, TH));
  normal_loss_backward_kernel<<<grid, NB, 0, gsr_stream(stream_)>>>(geometry, H, W, projection, alpha_min, d_loss,
                                                                   d_geometry);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
