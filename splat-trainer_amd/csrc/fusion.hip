// Depth-map fusion: multi-view consistency counts of one reference depth map, emission of the kept pixels as coloured
// world points, and the voxel-grid mean of a point cloud.  The arithmetic is in gsr_fusion.h (fp64, no contraction),
// the contract in include/gsplat_hip.h.
//
// fuse_check_kernel.  One thread per reference pixel in blocks of 16 x 16 pixels, so that the gathers of a block fall
//   into a compact region of each source.  The sources travel in the kernel arguments; the thread walks them with its
//   point in registers and writes its two counters once.  It is the only writer of them: no atomics.
// fuse_mask_kernel / fuse_emit_kernel.  One thread per pixel in row-major blocks of GSR_COMPACT_BLOCK, the block
//   size of gsr_compact_offsets.  The mask kernel writes the keep byte; the emit kernel evaluates the same predicate again, ranks
//   the kept pixels of its block by ballot and writes row base + block offset + rank.
// voxel_*.  The 63-bit cell key is sorted as two words by two stable passes of the radix sort (low word, then the high
//   word gathered through the first permutation); only the permutation is kept.  Run heads are flagged by comparing the
//   keys of neighbours, scanned into run numbers, and the starts scattered.  voxel_reduce_kernel gives every run a lane:
//   a run of up to VX_LONG points is summed by its lane, a longer one by the whole wave in turn (ballot over the lanes
//   that hold one).  The sums are int64, so the split changes no bit.
// No float atomics, no scratch, plain vector stores.
#include "gsr_device.h"
#include "gsr_host.h"
#include "gsr_fusion.h"

namespace {

constexpr int FB = GSR_COMPACT_BLOCK;   // threads per block: the emit kernel ranks inside gsr_compact_offsets' blocks
constexpr int FT = 16;             // side of the check kernel's pixel block
constexpr uint32_t VX_LONG = 32;   // a run longer than this is summed by the wave

__global__ __launch_bounds__(FB) void fuse_check_kernel(const float* __restrict__ ref_depth, int32_t Hr, int32_t Wr,
                                                        GsrFuseRef ref, GsrFuseSourceSet set, double near, double rel_tol,
                                                        uint8_t* __restrict__ counts) {
  const int j = (int)blockIdx.x * FT + (int)(threadIdx.x & (FT - 1)), i = (int)blockIdx.y * FT + (int)(threadIdx.x / FT);
  if (i >= Hr || j >= Wr) return;
  const int64_t px = (int64_t)i * Wr + j;
  const double d = (double)ref_depth[px];
  if (!gsr_fuse_valid(d)) return;
  double X, Y;
  gsr_fuse_unproject(ref, i, j, d, &X, &Y);
  uint32_t agree = 0, violate = 0;
  for (int s = 0; s < set.S; ++s) {
    int32_t is, js;
    double p2;
    if (!gsr_fuse_project(set.view[s], set.H[s], set.W[s], near, X, Y, d, &is, &js, &p2)) continue;
    const double ds = (double)set.depth[s][(int64_t)is * set.W[s] + js];
    const int vote = gsr_fuse_vote(ds, p2, rel_tol);
    agree += vote == GSR_FUSE_AGREE;
    violate += vote == GSR_FUSE_VIOLATE;
  }
  uint8_t* c = counts + 2 * px;
  const uint32_t a0 = c[0], v0 = c[1];
  c[0] = gsr_fuse_saturate(a0 + agree);
  c[1] = gsr_fuse_saturate(v0 + violate);
}

__global__ __launch_bounds__(FB) void fuse_mask_kernel(const float* __restrict__ ref_depth, const uint8_t* __restrict__ counts,
                                                       int64_t n_px, int32_t min_agree, int32_t max_violate,
                                                       uint8_t* __restrict__ keep_out) {
  const int64_t px = (int64_t)blockIdx.x * FB + threadIdx.x;
  if (px >= n_px) return;
  keep_out[px] = gsr_fuse_keep((double)ref_depth[px], counts[2 * px], counts[2 * px + 1], min_agree, max_violate) ? 1 : 0;
}

struct FuseWorld {
  double m[12];
};

__global__ __launch_bounds__(FB) void fuse_emit_kernel(const float* __restrict__ ref_depth, const uint8_t* __restrict__ counts,
                                                       const float* __restrict__ image, uint32_t n_px, uint32_t Wr,
                                                       GsrFuseRef ref, FuseWorld world, int32_t min_agree,
                                                       int32_t max_violate, const uint32_t* __restrict__ block_offsets,
                                                       int64_t base, int64_t capacity, float* __restrict__ points_out,
                                                       uint8_t* __restrict__ colors_out, uint8_t* __restrict__ agree_out) {
  const uint32_t px = blockIdx.x * FB + threadIdx.x;      // n_px <= 2^30
  double d = 0.0;
  uint32_t agree = 0;
  bool k = false;
  if (px < n_px) {
    d = (double)ref_depth[px];
    agree = counts[2 * (int64_t)px];
    k = gsr_fuse_keep(d, agree, counts[2 * (int64_t)px + 1], min_agree, max_violate);
  }
  const uint32_t rank = gsr_block_rank(k).before;
  const int64_t row = base + (int64_t)block_offsets[blockIdx.x] + rank;
  if (!k || row >= capacity) return;
  const uint32_t i = px / Wr, j = px - i * Wr;
  double X, Y;
  gsr_fuse_unproject(ref, (int32_t)i, (int32_t)j, d, &X, &Y);
  float* p = points_out + 3 * row;
  p[0] = (float)gsr_fuse_row(world.m, X, Y, d);
  p[1] = (float)gsr_fuse_row(world.m + 4, X, Y, d);
  p[2] = (float)gsr_fuse_row(world.m + 8, X, Y, d);
  uint8_t* c = colors_out + 3 * row;
  if (image) {
    const float* im = image + 3 * (int64_t)px;
    c[0] = gsr_fuse_colour(im[0]);
    c[1] = gsr_fuse_colour(im[1]);
    c[2] = gsr_fuse_colour(im[2]);
  } else {
    c[0] = 255; c[1] = 255; c[2] = 255;
  }
  agree_out[row] = (uint8_t)agree;
}

// ---- voxel grid ----
__global__ __launch_bounds__(FB) void voxel_low_keys_kernel(const float* __restrict__ points, uint32_t N, GsrVoxelGrid g,
                                                            uint32_t* __restrict__ keys_out) {
  const uint32_t i = blockIdx.x * FB + threadIdx.x;
  if (i >= N) return;
  keys_out[i] = (uint32_t)gsr_voxel_key_of(g, points + 3 * (int64_t)i);
}

// The high words in the order of the first pass: keys_out[i] of point order[i].
__global__ __launch_bounds__(FB) void voxel_high_keys_kernel(const float* __restrict__ points, uint32_t N, GsrVoxelGrid g,
                                                             const uint32_t* __restrict__ order,
                                                             uint32_t* __restrict__ keys_out) {
  const uint32_t i = blockIdx.x * FB + threadIdx.x;
  if (i >= N) return;
  keys_out[i] = (uint32_t)(gsr_voxel_key_of(g, points + 3 * (int64_t)order[i]) >> 32);
}

__global__ __launch_bounds__(FB) void voxel_heads_kernel(const float* __restrict__ points, uint32_t N, GsrVoxelGrid g,
                                                         const uint32_t* __restrict__ order, uint32_t* __restrict__ heads_out) {
  const uint32_t i = blockIdx.x * FB + threadIdx.x;
  if (i >= N) return;
  uint32_t head = 1;
  if (i > 0)
    head = gsr_voxel_key_of(g, points + 3 * (int64_t)order[i]) != gsr_voxel_key_of(g, points + 3 * (int64_t)order[i - 1]);
  heads_out[i] = head;
}

// starts_out[r] = first position of run r; starts_out[K] = N.
__global__ __launch_bounds__(FB) void voxel_starts_kernel(const uint32_t* __restrict__ heads, const uint32_t* __restrict__ run_of,
                                                          uint32_t N, uint32_t* __restrict__ starts_out) {
  const uint32_t i = blockIdx.x * FB + threadIdx.x;
  if (i >= N) return;
  const uint32_t h = heads[i], r = run_of[i];
  if (h) starts_out[r] = i;
  if (i == N - 1) starts_out[r + h] = N;
}

struct VoxelSums {
  int64_t S[3], C[3];
};

__device__ __forceinline__ void voxel_add(VoxelSums& a, const GsrVoxelGrid& g, const float* __restrict__ points,
                                          const uint8_t* __restrict__ colors, uint32_t point) {
  const float* p = points + 3 * (int64_t)point;
  const uint8_t* c = colors + 3 * (int64_t)point;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int32_t q;
    int64_t F;
    gsr_voxel_axis(p[k], g.origin[k], g.inv, &q, &F);
    a.S[k] += F;
    a.C[k] += (int64_t)c[k];
  }
}

__device__ __forceinline__ void voxel_write(const VoxelSums& a, const GsrVoxelGrid& g, const float* __restrict__ points,
                                            uint32_t first_point, uint32_t n, uint32_t r, float* __restrict__ points_out,
                                            uint8_t* __restrict__ colors_out, int32_t* __restrict__ counts_out) {
  const float* p = points + 3 * (int64_t)first_point;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int32_t q;
    int64_t F;
    gsr_voxel_axis(p[k], g.origin[k], g.inv, &q, &F);
    points_out[3 * (int64_t)r + k] = gsr_voxel_mean(g.origin[k], g.voxel, q, a.S[k], (int64_t)n);
    colors_out[3 * (int64_t)r + k] = gsr_voxel_colour(a.C[k], (int64_t)n);
  }
  counts_out[r] = (int32_t)n;
}

__global__ __launch_bounds__(FB) void voxel_reduce_kernel(const float* __restrict__ points, const uint8_t* __restrict__ colors,
                                                          const uint32_t* __restrict__ order, const uint32_t* __restrict__ starts,
                                                          const uint32_t* __restrict__ K_dev, GsrVoxelGrid g,
                                                          float* __restrict__ points_out, uint8_t* __restrict__ colors_out,
                                                          int32_t* __restrict__ counts_out) {
  const uint32_t K = K_dev[0];
  const uint32_t r = blockIdx.x * FB + threadIdx.x;
  const bool live = r < K;
  uint32_t b = 0, e = 0;
  if (live) {
    b = starts[r];
    e = starts[r + 1];
  }
  const bool wide = live && e - b > VX_LONG;
  if (live && !wide) {
    VoxelSums a = {};
    for (uint32_t i = b; i < e; ++i) voxel_add(a, g, points, colors, order[i]);
    voxel_write(a, g, points, order[b], e - b, r, points_out, colors_out, counts_out);
  }
  uint64_t todo = __ballot(wide);
  const int lane = gsr_lane();
  while (todo) {
    const int owner = __builtin_ctzll(todo);
    todo &= todo - 1;
    const uint32_t bb = (uint32_t)__shfl((int)b, owner, 64), ee = (uint32_t)__shfl((int)e, owner, 64);
    VoxelSums a = {};
    for (uint32_t i = bb + (uint32_t)lane; i < ee; i += 64) voxel_add(a, g, points, colors, order[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.S[k] += __shfl_xor((long long)a.S[k], o, 64);
        a.C[k] += __shfl_xor((long long)a.C[k], o, 64);
      }
    }
    if (lane == owner) voxel_write(a, g, points, order[bb], ee - bb, r, points_out, colors_out, counts_out);
  }
}

// The workspace of gsr_voxel_downsample: four arrays of N + 1 words, then the sort's and the scan's shares.
struct VoxelCarve {
  size_t array_bytes, sort_bytes, scan_bytes, total_bytes;
};
VoxelCarve voxel_carve(int64_t N) {
  const int64_t n = N > 0 ? N : 0;
  VoxelCarve c;
  c.array_bytes = (((size_t)(n + 1) * sizeof(uint32_t) + 255) / 256) * 256;
  c.sort_bytes = ((gsr_sort_workspace_bytes(n) + 255) / 256) * 256;
  c.scan_bytes = ((gsr_scan_workspace_bytes(n) + 255) / 256) * 256;
  c.total_bytes = 4 * c.array_bytes + c.sort_bytes + c.scan_bytes + 256;
  return c;
}

}  // namespace

extern "C" {

int gsr_fuse_check(const float* ref_depth, int32_t Hr, int32_t Wr, const double* ref_intrinsics_host,
                   const GsrFuseSource* sources_host, const double* source_params_host, int32_t S,
                   const double* tolerances_host, uint8_t* counts, void* stream_) {
  int launch = 0;
  const int rc = gsr_fuse_check_args(ref_depth, Hr, Wr, ref_intrinsics_host, sources_host, source_params_host, S,
                                     tolerances_host, counts, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrFuseRef ref = {ref_intrinsics_host[0], ref_intrinsics_host[1], ref_intrinsics_host[2], ref_intrinsics_host[3]};
  GsrFuseSourceSet set = {};
  set.S = S;
  for (int s = 0; s < S; ++s) {
    set.depth[s] = sources_host[s].depth;
    set.H[s] = sources_host[s].H;
    set.W[s] = sources_host[s].W;
    const double* p = source_params_host + 16 * s;
    for (int k = 0; k < 12; ++k) set.view[s].rel[k] = p[k];
    set.view[s].fx = p[12]; set.view[s].fy = p[13]; set.view[s].cx = p[14]; set.view[s].cy = p[15];
  }
  fuse_check_kernel<<<dim3(grid_for(Wr, FT), grid_for(Hr, FT)), FB, 0, gsr_stream(stream_)>>>(
      ref_depth, Hr, Wr, ref, set, tolerances_host[0], tolerances_host[1], counts);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_fuse_mask(const float* ref_depth, const uint8_t* counts, int32_t Hr, int32_t Wr, int32_t min_agree,
                  int32_t max_violate, uint8_t* keep_out, void* stream_) {
  int launch = 0;
  const int rc = gsr_fuse_mask_args(ref_depth, counts, Hr, Wr, min_agree, max_violate, keep_out, &launch);
  if (rc < 0 || !launch) return rc;
  const int64_t n_px = (int64_t)Hr * Wr;
  fuse_mask_kernel<<<grid_for(n_px, FB), FB, 0, gsr_stream(stream_)>>>(ref_depth, counts, n_px, min_agree, max_violate,
                                                                      keep_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_fuse_emit(const float* ref_depth, const uint8_t* counts, const float* image, int32_t Hr, int32_t Wr,
                  const double* ref_intrinsics_host, const double* world_t_ref_host, int32_t min_agree,
                  int32_t max_violate, const uint32_t* block_offsets, int64_t base, int64_t capacity, float* points_out,
                  uint8_t* colors_out, uint8_t* agree_out, void* stream_) {
  int launch = 0;
  const int rc = gsr_fuse_emit_args(ref_depth, counts, Hr, Wr, ref_intrinsics_host, world_t_ref_host, min_agree,
                                    max_violate, block_offsets, base, capacity, points_out, colors_out, agree_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrFuseRef ref = {ref_intrinsics_host[0], ref_intrinsics_host[1], ref_intrinsics_host[2], ref_intrinsics_host[3]};
  FuseWorld world;
  for (int k = 0; k < 12; ++k) world.m[k] = world_t_ref_host[k];
  const int64_t n_px = (int64_t)Hr * Wr;
  fuse_emit_kernel<<<grid_for(n_px, FB), FB, 0, gsr_stream(stream_)>>>(
      ref_depth, counts, image, (uint32_t)n_px, (uint32_t)Wr, ref, world, min_agree, max_violate, block_offsets, base,
      capacity, points_out, colors_out, agree_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

size_t gsr_voxel_workspace_bytes(int64_t N) { return voxel_carve(N).total_bytes; }

int gsr_voxel_downsample(const float* points, const uint8_t* colors, int64_t N, const double* grid_host,
                         float* points_out, uint8_t* colors_out, int32_t* counts_out, uint32_t* K_dev, void* workspace,
                         size_t workspace_bytes, void* stream_) {
  int launch = 0;
  const int rc = gsr_voxel_args(points, colors, N, grid_host, points_out, colors_out, counts_out, K_dev, &launch);
  if (rc < 0 || !launch) return rc;
  const VoxelCarve carve = voxel_carve(N);
  if (!workspace || workspace_bytes < carve.total_bytes) return GSR_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t stream = gsr_stream(stream_);
  const GsrVoxelGrid g = gsr_voxel_grid_make(grid_host);
  uint8_t* ws = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
  uint32_t* keys[2] = {reinterpret_cast<uint32_t*>(ws), reinterpret_cast<uint32_t*>(ws + carve.array_bytes)};
  uint32_t* vals[2] = {reinterpret_cast<uint32_t*>(ws + 2 * carve.array_bytes),
                       reinterpret_cast<uint32_t*>(ws + 3 * carve.array_bytes)};
  void* sort_ws = ws + 4 * carve.array_bytes;
  void* scan_ws = ws + 4 * carve.array_bytes + carve.sort_bytes;
  const uint32_t n = (uint32_t)N;
  const unsigned blocks = grid_for(N, FB);

  voxel_low_keys_kernel<<<blocks, FB, 0, stream>>>(points, n, g, keys[0]);
  GSR_CHECK_LAUNCH();
  const int first = gsr_sort_pairs_u32(keys[0], vals[0], keys[1], vals[1], N, 1, 0, 32, sort_ws, carve.sort_bytes, nullptr,
                                       stream_);
  if (first < 0) return first;
  // the high words go where the first pass left its keys: its permutation is the second pass's input
  voxel_high_keys_kernel<<<blocks, FB, 0, stream>>>(points, n, g, vals[first], keys[first]);
  GSR_CHECK_LAUNCH();
  const int second = gsr_sort_pairs_u32(keys[first], vals[first], keys[first ^ 1], vals[first ^ 1], N, 0, 0, 31, sort_ws,
                                        carve.sort_bytes, nullptr, stream_);
  if (second < 0) return second;
  const int at = first ^ second;                       // where the order is; the other three arrays are free
  const uint32_t* order = vals[at];
  uint32_t* heads = keys[at ^ 1];
  uint32_t* run_of = vals[at ^ 1];
  uint32_t* starts = keys[at];
  voxel_heads_kernel<<<blocks, FB, 0, stream>>>(points, n, g, order, heads);
  GSR_CHECK_LAUNCH();
  GSR_TRY(gsr_exclusive_scan_u32(heads, run_of, N, K_dev, scan_ws, carve.scan_bytes, stream_));
  voxel_starts_kernel<<<blocks, FB, 0, stream>>>(heads, run_of, n, starts);
  GSR_CHECK_LAUNCH();
  voxel_reduce_kernel<<<blocks, FB, 0, stream>>>(points, colors, order, starts, K_dev, g, points_out, colors_out,
                                                 counts_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
