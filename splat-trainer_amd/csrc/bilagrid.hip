// Bilateral-grid colour correction (the reference's BilateralCorrector): slice forward, slice backward and the total
// variation of the grids.  Per-pixel maths in gsr_bilagrid.h.  No float atomics anywhere: every sum has a fixed order, so
// two runs give the same bits.
//
// Work split of the slice kernels: the (GW - 1) x (GH - 1) xy cells of the grid, each cut into S sub-ranges of its pixels
// (S fixed by the grid shape, gsr_bg_subdivisions), one 256-thread workgroup per (cell, sub-range).  All pixels of a
// workgroup share the cell's 4 corner columns, staged once in LDS as cols[4][L][12].
//   forward:  out = A(rgb) rgb + a per pixel; nothing else is written (backward recomputes A).
//   backward: dL/drgb per pixel; for the grid, every workgroup writes ONE slot of 4 x L x 12 floats -- the sum over its
//             pixels of (corner weight) x go[m] x (r, g, b, 1)[n] per (corner q, level, channel).  The levels go one at a
//             time (48 register accumulators per thread, one pass over the pixels per level: a pixel touches levels
//             z0 and z0 + 1 only, and a pass no pixel of the workgroup touches writes zeros without a reduction); the
//             workgroup sums a pass by DPP row sums and then its 16 row sums through LDS in row order.  Two levels per
//             pass (96 accumulators) spilled at the 128-VGPR cap and do the same reduction work.  bg_grad_finish_kernel gives each grid vertex the slots of its (at most 4)
//             adjacent cells, cells in (y, x) order and sub-ranges in order.
#include "gsr_device.h"
#include "gsr_dpp_reduce.h"
#include "gsr_bilagrid.h"
#include "gsr_host.h"

namespace {

constexpr int BG_BLOCK = 256;
constexpr int BG_LW = 1;                                  // levels per backward pass
constexpr int BG_ACC = BG_LW * 4 * GSR_BG_CH;             // 48 accumulators per thread
constexpr int BG_TARGET_WORKGROUPS = 1024;                // 4 per CU
constexpr int BG_TV_MAX_BLOCKS = 1024;

struct BgShape {
  int L, GH, GW, H, W, S;
  float inv_2w, inv_2h;
};

int bg_subdivisions(int GH, int GW) {
  const int cells = (GH - 1) * (GW - 1);
  const int s = (BG_TARGET_WORKGROUPS + cells - 1) / cells;
  return s < 1 ? 1 : (s > 16 ? 16 : s);
}

bool bg_shape_ok(int L, int GH, int GW) {
  return L >= 2 && L <= 64 && GH >= 2 && GH <= 64 && GW >= 2 && GW <= 64;
}

BgShape bg_shape(int L, int GH, int GW, int H, int W) {
  return BgShape{L, GH, GW, H, W, bg_subdivisions(GH, GW), 1.f / (2.f * (float)W), 1.f / (2.f * (float)H)};
}

size_t bg_slot_floats(int L, int GH, int GW) {
  return (size_t)(GH - 1) * (GW - 1) * bg_subdivisions(GH, GW) * 4 * L * GSR_BG_CH;
}

// Corner columns of the workgroup's cell into LDS, and the pixel sub-range: calls f(row, col, ty, tx) for each pixel of
// this thread (rows of the cell's pixel rectangle, flattened and cut into S equal ranges; thread t takes every 256th).
struct BgCell {
  int cx, cy, i0, j0, cw;
  int p, p_end;
};

__device__ __forceinline__ BgCell bg_stage(const float* __restrict__ grid, const BgShape& sh, float* cols) {
  const int cell = blockIdx.x / sh.S, s = blockIdx.x - cell * sh.S;
  BgCell b;
  b.cy = cell / (sh.GW - 1);
  b.cx = cell - b.cy * (sh.GW - 1);
  const int n_col = 4 * sh.L * GSR_BG_CH, per_q = sh.L * GSR_BG_CH;
  for (int e = threadIdx.x; e < n_col; e += BG_BLOCK) {
    const int q = e / per_q, rem = e - q * per_q, l = rem / GSR_BG_CH, c = rem - l * GSR_BG_CH;
    cols[e] = grid[(((int64_t)c * sh.L + l) * sh.GH + b.cy + (q >> 1)) * sh.GW + b.cx + (q & 1)];
  }
  b.j0 = gsr_bg_first(b.cx, sh.W, sh.GW);
  b.i0 = gsr_bg_first(b.cy, sh.H, sh.GH);
  b.cw = gsr_bg_first(b.cx + 1, sh.W, sh.GW) - b.j0;
  const int64_t n = (int64_t)b.cw * (gsr_bg_first(b.cy + 1, sh.H, sh.GH) - b.i0);
  b.p = (int)(n * s / sh.S);
  b.p_end = (int)(n * (s + 1) / sh.S);
  return b;
}

template <class F>
__device__ __forceinline__ void bg_for_pixels(const BgCell& b, const BgShape& sh, F&& f) {
  int p = b.p + (int)threadIdx.x;
  if (p >= b.p_end) return;
  const int dr = BG_BLOCK / b.cw, dc = BG_BLOCK - dr * b.cw;
  int r = p / b.cw, c = p - r * b.cw;
  for (; p < b.p_end; p += BG_BLOCK) {
    const int row = b.i0 + r, col = b.j0 + c;
    f(row, col, gsr_bg_frac(row, b.cy, sh.H, sh.GH, sh.inv_2h), gsr_bg_frac(col, b.cx, sh.W, sh.GW, sh.inv_2w));
    r += dr;
    c += dc;
    if (c >= b.cw) { c -= b.cw; ++r; }
  }
}

__global__ __launch_bounds__(BG_BLOCK) void bg_slice_fwd_kernel(const float* __restrict__ grid, BgShape sh,
                                                                 const float* __restrict__ rgb,
                                                                 float* __restrict__ out) {
  extern __shared__ float cols[];
  const BgCell b = bg_stage(grid, sh, cols);
  __syncthreads();
  bg_for_pixels(b, sh, [&](int row, int col, float ty, float tx) {
    const uint32_t o = 3u * ((uint32_t)row * (uint32_t)sh.W + (uint32_t)col);
    float v[3];
    gsr_bg_pixel_fwd(cols, sh.L, tx, ty, rgb[o], rgb[o + 1], rgb[o + 2], v);
    out[o] = v[0]; out[o + 1] = v[1]; out[o + 2] = v[2];
  });
}

__global__ __launch_bounds__(BG_BLOCK) __attribute__((amdgpu_waves_per_eu(4))) void bg_slice_bwd_kernel(const float* __restrict__ grid, BgShape sh,
                                                                 const float* __restrict__ rgb,
                                                                 const float* __restrict__ gout,
                                                                 float* __restrict__ d_rgb,
                                                                 float* __restrict__ slots) {
  extern __shared__ float cols[];
  // gsr_block_rows_handoff's layout, kept here: through the helper this kernel's schedule changes, and its float sums
  // pin it to identical code
  __shared__ float s_rows[16][BG_ACC];        // 4 waves x 4 rows of 16 lanes
  const BgCell b = bg_stage(grid, sh, cols);
  __syncthreads();
  if (d_rgb) {
    bg_for_pixels(b, sh, [&](int row, int col, float ty, float tx) {
      const uint32_t o = 3u * ((uint32_t)row * (uint32_t)sh.W + (uint32_t)col);
      const float go[3] = {gout[o], gout[o + 1], gout[o + 2]};
      float d[3];
      gsr_bg_pixel_bwd_rgb(cols, sh.L, tx, ty, rgb[o], rgb[o + 1], rgb[o + 2], go, d);
      d_rgb[o] = d[0]; d_rgb[o + 1] = d[1]; d_rgb[o + 2] = d[2];
    });
  }
  if (!slots) return;
  float* slot = slots + (int64_t)blockIdx.x * 4 * sh.L * GSR_BG_CH;
  const int lane = gsr_lane(), wave = threadIdx.x >> 6;
  for (int lb = 0; lb < sh.L; lb += BG_LW) {
    float acc[BG_ACC];                        // [k][q][c]
#pragma unroll
    for (int j = 0; j < BG_ACC; ++j) acc[j] = 0.f;
    bool touched = false;
    bg_for_pixels(b, sh, [&](int row, int col, float ty, float tx) {
      const uint32_t o = 3u * ((uint32_t)row * (uint32_t)sh.W + (uint32_t)col);
      const float r = rgb[o], g = rgb[o + 1], bl = rgb[o + 2];
      const GsrBgZ z = gsr_bg_z(gsr_bg_luma(r, g, bl), sh.L);
      const int k0 = z.z0 - lb;               // level z0 is k0 of this pass, z0 + 1 is k0 + 1
      if (k0 < -1 || k0 >= BG_LW) return;
      touched = true;
      float u[GSR_BG_CH];                     // go[m] * (r, g, b, 1)[n]
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const float gm = gout[o + m];
        u[4 * m] = gm * r; u[4 * m + 1] = gm * g; u[4 * m + 2] = gm * bl; u[4 * m + 3] = gm;
      }
      float wxy[4];
      gsr_bg_xy_weights(tx, ty, wxy);
#pragma unroll
      for (int k = 0; k < BG_LW; ++k) {
        const float wz = k == k0 ? 1.f - z.tz : (k == k0 + 1 ? z.tz : 0.f);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float w = wz * wxy[q];
#pragma unroll
          for (int c = 0; c < GSR_BG_CH; ++c) acc[(k * 4 + q) * GSR_BG_CH + c] = fmaf(w, u[c], acc[(k * 4 + q) * GSR_BG_CH + c]);
        }
      }
    });
    if (!__syncthreads_or(touched)) {          // no pixel of the workgroup at these levels
      for (int j = threadIdx.x; j < BG_ACC; j += BG_BLOCK) {
        const int k = j / (4 * GSR_BG_CH), q = (j / GSR_BG_CH) & 3, c = j % GSR_BG_CH;
        if (lb + k < sh.L) slot[(q * sh.L + lb + k) * GSR_BG_CH + c] = 0.f;
      }
      continue;
    }
#pragma unroll
    for (int j = 0; j < BG_ACC; ++j) acc[j] = gsr_row_sum_to_lane15(acc[j]);
    if ((lane & 15) == 15) {
#pragma unroll
      for (int j = 0; j < BG_ACC; ++j) s_rows[4 * wave + (lane >> 4)][j] = acc[j];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < BG_ACC; j += BG_BLOCK) {
      float a = 0.f;
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) a += s_rows[rr][j];
      const int k = j / (4 * GSR_BG_CH), q = (j / GSR_BG_CH) & 3, c = j % GSR_BG_CH;
      if (lb + k < sh.L) slot[(q * sh.L + lb + k) * GSR_BG_CH + c] = a;
    }
    __syncthreads();                           // s_rows is reused by the next pass
  }
}

// One thread per vertex (c, l, gy, gx) of grid k: the slots of the adjacent cells, (cy, cx) ascending, sub-ranges in order.
__global__ __launch_bounds__(BG_BLOCK) void bg_grad_finish_kernel(const float* __restrict__ slots, BgShape sh,
                                                                   float* __restrict__ d_grid) {
  const int total = GSR_BG_CH * sh.L * sh.GH * sh.GW;
  const int e = blockIdx.x * BG_BLOCK + threadIdx.x;
  if (e >= total) return;
  const int gx = e % sh.GW, t = e / sh.GW, gy = t % sh.GH, t2 = t / sh.GH, l = t2 % sh.L, c = t2 / sh.L;
  const int slot_floats = 4 * sh.L * GSR_BG_CH;
  float a = 0.f;
  for (int cy = gy - 1; cy <= gy; ++cy) {
    if (cy < 0 || cy > sh.GH - 2) continue;
    for (int cx = gx - 1; cx <= gx; ++cx) {
      if (cx < 0 || cx > sh.GW - 2) continue;
      const int q = 2 * (gy - cy) + (gx - cx);
      const float* p = slots + (int64_t)(cy * (sh.GW - 1) + cx) * sh.S * slot_floats + (q * sh.L + l) * GSR_BG_CH + c;
      for (int s = 0; s < sh.S; ++s) a += p[(int64_t)s * slot_floats];
    }
  }
  d_grid[e] = a;
}

// Total variation: per element the squares of its three forward differences (value) and
// d = sum over axes of (g - previous) - (next - g) (gradient), written as gscale * d (added when accumulate).  Blocks
// (x: elements of one grid, y: grids, both grid-stride, counts fixed by the shape) each write one partial sum.
__global__ __launch_bounds__(BG_BLOCK) void bg_tv_kernel(const float* __restrict__ G, int64_t N, int L, int GH, int GW,
                                                          float gscale, float* __restrict__ dG, int accumulate,
                                                          float* __restrict__ partials) {
  const int per = GSR_BG_CH * L * GH * GW, plane = GH * GW;
  float v = 0.f;
  for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
    const float* g0 = G + n * per;
    for (int w = blockIdx.x * BG_BLOCK + threadIdx.x; w < per; w += gridDim.x * BG_BLOCK) {
      const int gx = w % GW, t = w / GW, gy = t % GH, l = (t / GH) % L;
      const float g = g0[w];
      float d = 0.f;
      if (gx + 1 < GW) { const float f = g0[w + 1] - g; v = fmaf(f, f, v); d -= f; }
      if (gx > 0) d += g - g0[w - 1];
      if (gy + 1 < GH) { const float f = g0[w + GW] - g; v = fmaf(f, f, v); d -= f; }
      if (gy > 0) d += g - g0[w - GW];
      if (l + 1 < L) { const float f = g0[w + plane] - g; v = fmaf(f, f, v); d -= f; }
      if (l > 0) d += g - g0[w - plane];
      if (dG) {
        float* o = dG + n * per + w;
        *o = accumulate ? fmaf(gscale, d, *o) : gscale * d;
      }
    }
  }
  const GsrWaves<float>& s_wave = gsr_block_handoff<63>(gsr_wave_sum_to_lane63(v));
  if (threadIdx.x == 0)
    partials[blockIdx.y * gridDim.x + blockIdx.x] = (((0.f + s_wave[0]) + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// One block: partials in order (thread t: t, t + 256, ...), then the block sum; tv_out[0] = scale * total.
__global__ __launch_bounds__(BG_BLOCK) void bg_tv_finish_kernel(const float* __restrict__ partials, int n, float scale,
                                                                 float* __restrict__ tv_out) {
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += BG_BLOCK) v += partials[i];
  const GsrWaves<float>& s_wave = gsr_block_handoff<63>(gsr_wave_sum_to_lane63(v));
  if (threadIdx.x == 0) tv_out[0] = scale * ((((0.f + s_wave[0]) + s_wave[1]) + s_wave[2]) + s_wave[3]);
}

void bg_tv_blocks(int64_t N, int L, int GH, int GW, unsigned& bx, unsigned& by) {
  const int per = GSR_BG_CH * L * GH * GW;
  bx = grid_for(per, BG_BLOCK);
  if (bx > (unsigned)BG_TV_MAX_BLOCKS) bx = BG_TV_MAX_BLOCKS;
  int64_t y = BG_TV_MAX_BLOCKS / bx;
  if (y < 1) y = 1;
  if (y > N) y = N;
  by = (unsigned)y;
}

bool bg_image_ok(int H, int W) { return H >= 1 && W >= 1 && H <= GSR_BILAGRID_MAX_SIDE && W <= GSR_BILAGRID_MAX_SIDE; }

}  // namespace

extern "C" {

size_t gsr_bilagrid_workspace_bytes(int32_t L, int32_t GH, int32_t GW) {
  if (!bg_shape_ok(L, GH, GW)) return 0;
  const size_t slots = bg_slot_floats(L, GH, GW);
  return sizeof(float) * (slots > (size_t)BG_TV_MAX_BLOCKS ? slots : (size_t)BG_TV_MAX_BLOCKS);
}

int gsr_bilagrid_slice_forward(const float* grids, int64_t N, int32_t L, int32_t GH, int32_t GW, int64_t k,
                               const float* rgb, int32_t H, int32_t W, float* out, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!grids || !rgb || !out || !bg_shape_ok(L, GH, GW) || k < 0 || k >= N || !bg_image_ok(H, W))
    return GSR_ERR_INVALID_ARGUMENT;
  const BgShape sh = bg_shape(L, GH, GW, H, W);
  const float* grid = grids + k * (int64_t)GSR_BG_CH * L * GH * GW;
  bg_slice_fwd_kernel<<<(GH - 1) * (GW - 1) * sh.S, BG_BLOCK, sizeof(float) * 4 * L * GSR_BG_CH, stream>>>(grid, sh, rgb,
                                                                                                           out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_bilagrid_slice_backward(const float* grids, int64_t N, int32_t L, int32_t GH, int32_t GW, int64_t k,
                                const float* rgb, int32_t H, int32_t W, const float* d_out, float* d_rgb, float* d_grids,
                                void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!grids || !rgb || !d_out || !bg_shape_ok(L, GH, GW) || k < 0 || k >= N || !bg_image_ok(H, W))
    return GSR_ERR_INVALID_ARGUMENT;
  if (!d_rgb && !d_grids) return GSR_OK;
  if (d_grids && (!workspace || workspace_bytes < gsr_bilagrid_workspace_bytes(L, GH, GW)))
    return GSR_ERR_WORKSPACE_TOO_SMALL;
  const BgShape sh = bg_shape(L, GH, GW, H, W);
  const int64_t per = (int64_t)GSR_BG_CH * L * GH * GW;
  float* slots = d_grids ? static_cast<float*>(workspace) : nullptr;
  bg_slice_bwd_kernel<<<(GH - 1) * (GW - 1) * sh.S, BG_BLOCK, sizeof(float) * 4 * L * GSR_BG_CH, stream>>>(
      grids + k * per, sh, rgb, d_out, d_rgb, slots);
  GSR_CHECK_LAUNCH();
  if (d_grids) {
    bg_grad_finish_kernel<<<grid_for(per, BG_BLOCK), BG_BLOCK, 0, stream>>>(slots, sh, d_grids + k * per);
    GSR_CHECK_LAUNCH();
  }
  return GSR_OK;
}

int gsr_bilagrid_tv(const float* grids, int64_t N, int32_t L, int32_t GH, int32_t GW, float weight, float* tv_out,
                    float* d_grids, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!grids || !tv_out || N < 1 || !bg_shape_ok(L, GH, GW)) return GSR_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < sizeof(float) * BG_TV_MAX_BLOCKS) return GSR_ERR_WORKSPACE_TOO_SMALL;
  unsigned bx, by;
  bg_tv_blocks(N, L, GH, GW, bx, by);
  // tv = (1/N) sum_axes sum (diff^2) / (12 L GH GW); dtv/dG = 2 d / (N 12 L GH GW)
  const double count = (double)N * GSR_BG_CH * L * GH * GW;
  float* partials = static_cast<float*>(workspace);
  bg_tv_kernel<<<dim3(bx, by), BG_BLOCK, 0, stream>>>(grids, N, L, GH, GW, (float)(2.0 * weight / count), d_grids,
                                                      accumulate ? 1 : 0, partials);
  GSR_CHECK_LAUNCH();
  bg_tv_finish_kernel<<<1, BG_BLOCK, 0, stream>>>(partials, (int)(bx * by), (float)(weight / count), tv_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
