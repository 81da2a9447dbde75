// Frustum point queries and per-cluster view features (the reference's visibility/query_points.py point_visibility /
// camera_counts / foreground_visibility and visibility/cluster.py PointClusters.view_features).  Per-pair maths and the
// summation order in gsr_visibility.h.  No float atomics: the counts are integers and the feature sums have a fixed order.
//
// frustum_counts_kernel  every lane keeps FR_PPL points in registers; the cameras are wave-uniform and come through the
//                        scalar cache, one 64-byte record each, FR_STEP per step.  A camera's count over the wave is a
//                        ballot + popcount per point slot; lane (c mod 64) keeps the count of camera c, so a tile of 64
//                        cameras costs one LDS round per block: the waves' 64 counts are added and leave the block as
//                        one integer atomic per camera that saw a point.
// view features (one call, no host sync), the cluster order (points sorted by label, [start, end) per cluster) built once
// by the caller with gsr_sort_pairs_u32 + gsr_tile_ranges:
//   vf_scatter_kernel     dense[idx[j]] = value(vis[j]) into the zero-filled scratch, point_visible[idx[j]] += 1;
//   vf_chunk_sum_kernel   one thread per GSR_VF_CHUNK consecutive sorted points: the sum of each run of one label inside
//                         the chunk, written to slot[run start] (as km_chunk_sum_kernel of neighbours.hip);
//   vf_finish_kernel      one wave per cluster: its slots lane-strided, then the fixed DPP tree; an empty cluster gives 0.
#include "gsr_device.h"
#include "gsr_visibility.h"
#include "gsr_host.h"

namespace {

constexpr int VIS_BLOCK = 256;
constexpr int FR_PPL = 4;                   // points per lane
constexpr int FR_STEP = 4;                  // cameras per step of the sweep
constexpr int FR_TILE = 64;                 // cameras per block-level combine (one per lane)

__global__ __launch_bounds__(VIS_BLOCK) void frustum_counts_kernel(const float* __restrict__ p, int N,
                                                                    const float* __restrict__ rec, int V, float depth_below,
                                                                    int32_t* __restrict__ point_counts,
                                                                    int32_t* __restrict__ camera_counts) {
  __shared__ int32_t s_cnt[VIS_BLOCK / 64][FR_TILE];
  const int lane = gsr_lane();
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
  const int64_t base = (int64_t)blockIdx.x * (VIS_BLOCK * FR_PPL) + threadIdx.x;
  float x[FR_PPL], y[FR_PPL], z[FR_PPL];
  int32_t seen[FR_PPL];
#pragma unroll
  for (int u = 0; u < FR_PPL; ++u) {
    const int64_t i = base + (int64_t)u * VIS_BLOCK;
    const bool live = i < N;
    const int64_t q = live ? i : (int64_t)N - 1;
    x[u] = live ? p[3 * q] : NAN;              // a lane past N holds a NaN point: outside every camera
    y[u] = p[3 * q + 1];
    z[u] = p[3 * q + 2];
    seen[u] = 0;
  }
  for (int c0 = 0; c0 < V; c0 += FR_TILE) {
    const int c1 = min(c0 + FR_TILE, V);
    int32_t mine = 0;                          // lane l: the wave's count for camera c0 + l
    int c = c0;
    for (; c + FR_STEP <= c1; c += FR_STEP) {
#pragma unroll
      for (int s = 0; s < FR_STEP; ++s) {
        const float* r = rec + (int64_t)GSR_VIS_RECORD_FLOATS * (c + s);
        int32_t n = 0;
#pragma unroll
        for (int u = 0; u < FR_PPL; ++u) {
          const bool in = gsr_vis_inside(r, x[u], y[u], z[u], depth_below);
          seen[u] += in ? 1 : 0;
          n += (int32_t)__popcll(__ballot(in));
        }
        mine = lane == c + s - c0 ? n : mine;
      }
    }
    for (; c < c1; ++c) {
      const float* r = rec + (int64_t)GSR_VIS_RECORD_FLOATS * c;
      int32_t n = 0;
#pragma unroll
      for (int u = 0; u < FR_PPL; ++u) {
        const bool in = gsr_vis_inside(r, x[u], y[u], z[u], depth_below);
        seen[u] += in ? 1 : 0;
        n += (int32_t)__popcll(__ballot(in));
      }
      mine = lane == c - c0 ? n : mine;
    }
    if (camera_counts) {                       // (a kernel argument: uniform over the block, the barriers are safe)
      s_cnt[wave][lane] = mine;
      __syncthreads();
      if (threadIdx.x < FR_TILE && c0 + (int)threadIdx.x < V) {
        int32_t t = 0;
#pragma unroll
        for (int w = 0; w < VIS_BLOCK / 64; ++w) t += s_cnt[w][threadIdx.x];
        if (t) atomicAdd(camera_counts + c0 + threadIdx.x, t);
      }
      __syncthreads();
    }
  }
  if (point_counts) {
#pragma unroll
    for (int u = 0; u < FR_PPL; ++u) {
      const int64_t i = base + (int64_t)u * VIS_BLOCK;
      if (i < N) point_counts[i] = seen[u];
    }
  }
}

// Entries whose index falls outside [0, N) are skipped (the contract excludes them; nothing is written out of bounds).
__global__ __launch_bounds__(VIS_BLOCK) void vf_scatter_kernel(const int64_t* __restrict__ idx,
                                                                const float* __restrict__ vis, int64_t M, int64_t N,
                                                                float threshold, float* __restrict__ dense,
                                                                int32_t* __restrict__ point_visible) {
  const int64_t j = (int64_t)blockIdx.x * VIS_BLOCK + threadIdx.x;
  if (j >= M) return;
  const int64_t i = idx[j];
  if (i < 0 || i >= N) return;
  dense[i] = gsr_vf_value(vis[j], threshold);
  if (point_visible) atomicAdd(point_visible + i, 1);
}

// Thread c: sorted positions [c GSR_VF_CHUNK, (c + 1) GSR_VF_CHUNK) ∩ [0, N).
__global__ __launch_bounds__(VIS_BLOCK) void vf_chunk_sum_kernel(const float* __restrict__ dense,
                                                                  const uint32_t* __restrict__ skeys,
                                                                  const uint32_t* __restrict__ svals, int N,
                                                                  float* __restrict__ slots) {
  constexpr int CH = GSR_VF_CHUNK;
  const int64_t p0 = ((int64_t)blockIdx.x * VIS_BLOCK + threadIdx.x) * CH;
  if (p0 >= N) return;
  const int n = (int)min((int64_t)CH, (int64_t)N - p0);
  uint32_t key[CH], v[CH];
  if (n == CH) {
    const uint4* k4 = reinterpret_cast<const uint4*>(skeys + p0);
    const uint4* v4 = reinterpret_cast<const uint4*>(svals + p0);
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) {
      const uint4 a = k4[q], b = v4[q];
      key[4 * q] = a.x; key[4 * q + 1] = a.y; key[4 * q + 2] = a.z; key[4 * q + 3] = a.w;
      v[4 * q] = b.x; v[4 * q + 1] = b.y; v[4 * q + 2] = b.z; v[4 * q + 3] = b.w;
    }
  } else {
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      key[u] = u < n ? skeys[p0 + u] : 0u;
      v[u] = u < n ? svals[p0 + u] : 0u;
    }
  }
  float val[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) val[u] = u < n ? dense[v[u]] : 0.f;
  float s = val[0];
  int64_t start = p0;
#pragma unroll
  for (int u = 1; u < CH; ++u) {
    if (u < n) {
      if (key[u] != key[u - 1]) {
        slots[start] = s;
        start = p0 + u;
        s = val[u];
      } else {
        s += val[u];
      }
    }
  }
  slots[start] = s;
}

// One wave per cluster; range [K, 2] from gsr_tile_ranges (zero-filled first: an absent cluster reads [0, 0)).
__global__ __launch_bounds__(VIS_BLOCK) void vf_finish_kernel(const float* __restrict__ slots,
                                                               const uint32_t* __restrict__ range, int K,
                                                               float* __restrict__ out) {
  constexpr int CH = GSR_VF_CHUNK;
  const int c = (int)blockIdx.x * (VIS_BLOCK / 64) + (__builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6);
  if (c >= K) return;
  const int64_t s = range[2 * c], e = range[2 * c + 1];
  float a = 0.f;
  if (e > s) {
    const int64_t first = s / CH + 1, last = (e - 1) / CH;
    const int64_t T = 1 + (last >= first ? last - first + 1 : 0);
    for (int64_t t = gsr_lane(); t < T; t += 64) a += slots[t == 0 ? s : (first + t - 1) * CH];
  }
  a = gsr_wave_sum_to_lane63(a);
  if (gsr_lane() == 63) out[c] = a;
}

}  // namespace

extern "C" {

int gsr_frustum_counts(const float* points, int64_t N, const float* records, int64_t V, float depth_below,
                       int32_t* point_counts_out, int32_t* camera_counts_out, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!points || !records || N < 1 || N > GSR_NEIGHBOURS_MAX_N || V < 1 || V > GSR_VISIBILITY_MAX_CAMERAS)
    return GSR_ERR_INVALID_ARGUMENT;
  if (!point_counts_out && !camera_counts_out) return GSR_ERR_INVALID_ARGUMENT;
  if (camera_counts_out && hipMemsetAsync(camera_counts_out, 0, sizeof(int32_t) * V, stream) != hipSuccess)
    return GSR_ERR_LAUNCH_FAILED;
  frustum_counts_kernel<<<grid_for(N, VIS_BLOCK * FR_PPL), VIS_BLOCK, 0, stream>>>(
      points, (int)N, records, (int)V, depth_below, point_counts_out, camera_counts_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_view_features(const int64_t* point_idx, const float* point_vis, int64_t M, float threshold,
                      const uint32_t* sorted_labels, const uint32_t* sorted_points, const uint32_t* cluster_range,
                      int64_t N, int64_t K, float* dense_scratch, float* slot_scratch, float* features_out,
                      int32_t* point_visible, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (M < 0 || M > GSR_NEIGHBOURS_MAX_N || (M > 0 && (!point_idx || !point_vis)) || !sorted_labels || !sorted_points ||
      !cluster_range || N < 1 || N > GSR_NEIGHBOURS_MAX_N || K < 1 || K > GSR_NEIGHBOURS_MAX_N || !dense_scratch ||
      !slot_scratch || !features_out)
    return GSR_ERR_INVALID_ARGUMENT;
  if (hipMemsetAsync(dense_scratch, 0, sizeof(float) * N, stream) != hipSuccess) return GSR_ERR_LAUNCH_FAILED;
  if (M > 0) {
    vf_scatter_kernel<<<grid_for(M, VIS_BLOCK), VIS_BLOCK, 0, stream>>>(point_idx, point_vis, M, N, threshold,
                                                                        dense_scratch, point_visible);
    GSR_CHECK_LAUNCH();
  }
  vf_chunk_sum_kernel<<<grid_for((N + GSR_VF_CHUNK - 1) / GSR_VF_CHUNK, VIS_BLOCK), VIS_BLOCK, 0, stream>>>(
      dense_scratch, sorted_labels, sorted_points, (int)N, slot_scratch);
  GSR_CHECK_LAUNCH();
  vf_finish_kernel<<<grid_for(K, VIS_BLOCK / 64), VIS_BLOCK, 0, stream>>>(slot_scratch, cluster_range, (int)K,
                                                                          features_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
