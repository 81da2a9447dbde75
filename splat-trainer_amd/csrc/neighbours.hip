// Brute-force neighbour searches over 3-D points: the k nearest points of every point of a cloud (kNN, the reference's
// estimate_scale) and Lloyd k-means (the reference's assign_clusters / kmeans_iter).  Per-pair maths in gsr_neighbours.h.
// No float atomics anywhere: every sum has a fixed order, so two runs give the same bits.
//
// kNN: one lane per query, its sorted top-k list in registers (k a template parameter).  The candidates are
//   wave-uniform and come through the scalar cache, eight per step; a step whose eight distances all miss the list's
//   last entry in every lane costs no insertion.  Only the 64-candidate tile holding the wave's own queries masks self.
//   Small clouds would leave SIMDs idle, so the candidates are cut into S segments of a multiple of 64 points (grid y);
//   every segment writes a partial list and knn_merge_kernel inserts the lists of segments 1.. into that of segment 0, in
//   segment order.  Each later list holds only higher indices, so the merged list is the one a single sweep gives.
// k-means iteration (all enqueued by one call, no host sync):
//   km_assign_kernel   one lane per point, centroids wave-uniform: label (int64, optional) and a u32 sort key;
//   gsr_sort_pairs_u32 stable radix sort of (label, point index) over ceil(log2 K) bits;
//   gsr_tile_ranges    [start, end) of every cluster in the sorted order;
//   km_chunk_sum_kernel one thread per KM_CH consecutive sorted points: the sum of each run of one label inside the
//                      chunk, in sorted order, written to slot[run start] (a run starts at its cluster's start or at a
//                      chunk boundary);
//   km_finish_kernel   one wave per cluster: the slots at its start and at each chunk boundary inside it, lane-strided
//                      then a fixed DPP tree, divided by the count; an empty cluster keeps its centroid.
#include "gsr_device.h"
#include "gsr_neighbours.h"
#include "gsr_host.h"

namespace {

constexpr int NB_BLOCK = 256;
constexpr int NB_STEP = 8;                  // candidates / centroids per step of the sweeps
constexpr int KNN_TARGET_WAVES = 4096;      // 4 waves per SIMD
constexpr int64_t KNN_MIN_SEGMENT = 1024;
constexpr int KNN_MAX_SEGMENTS = 16;
constexpr int KM_CH = 16;                   // sorted points per chunk of the centroid sums

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- kNN --------------------------------------------------------------------------------------------------------

// Segment length (a multiple of 64) and count for N points: enough waves to fill the chip, segments not too short.
void knn_segments(int64_t N, int64_t& seg_len, int& S) {
  const int64_t waves = (N + 63) / 64;
  int64_t s = (KNN_TARGET_WAVES + waves - 1) / waves;
  if (s > N / KNN_MIN_SEGMENT) s = N / KNN_MIN_SEGMENT;
  if (s > KNN_MAX_SEGMENTS) s = KNN_MAX_SEGMENTS;
  if (s < 1) s = 1;
  seg_len = (((N + s - 1) / s + 63) / 64) * 64;
  S = (int)((N + seg_len - 1) / seg_len);
}

// Candidates [a, b) into the list; SELF: candidate i (this lane's own point) is skipped.
template <int K, bool SELF>
__device__ __forceinline__ void knn_sweep(const float* __restrict__ p, int a, int b, float qx, float qy, float qz, int i,
                                          float (&d)[K], int32_t (&jj)[K]) {
  int j = a;
  for (; j + NB_STEP <= b; j += NB_STEP) {
    const float* c = p + 3 * (int64_t)j;
    float dn[NB_STEP];
#pragma unroll
    for (int u = 0; u < NB_STEP; ++u) {
      dn[u] = gsr_nb_dist2(qx, qy, qz, c[3 * u], c[3 * u + 1], c[3 * u + 2]);
      if (SELF && j + u == i) dn[u] = NAN;
    }
    const float m = fminf(fminf(fminf(dn[0], dn[1]), fminf(dn[2], dn[3])), fminf(fminf(dn[4], dn[5]), fminf(dn[6], dn[7])));
    if (m < d[K - 1]) {
#pragma unroll
      for (int u = 0; u < NB_STEP; ++u) gsr_nb_insert(d, jj, dn[u], j + u);
    }
  }
  for (; j < b; ++j) {
    const float* c = p + 3 * (int64_t)j;
    const float dn = gsr_nb_dist2(qx, qy, qz, c[0], c[1], c[2]);
    if (!SELF || j != i) gsr_nb_insert(d, jj, dn, j);
  }
}

template <int K>
__device__ __forceinline__ void knn_write(int64_t i, const float (&d)[K], const int32_t (&jj)[K], float* __restrict__ dist2,
                                          int64_t* __restrict__ idx, float* __restrict__ scale) {
#pragma unroll
  for (int t = 0; t < K; ++t) {
    dist2[i * K + t] = d[t];
    idx[i * K + t] = jj[t];
  }
  if (scale) scale[i] = gsr_nb_mean_dist(d);
}

// grid (ceil(N / 256), S); S == 1 writes the outputs, otherwise partial lists part_d / part_j [S, N, K].
template <int K>
__global__ __launch_bounds__(NB_BLOCK) void knn_kernel(const float* __restrict__ p, int N, int seg_len,
                                                        float* __restrict__ dist2, int64_t* __restrict__ idx,
                                                        float* __restrict__ scale, float* __restrict__ part_d,
                                                        int32_t* __restrict__ part_j) {
  const int i = (int)blockIdx.x * NB_BLOCK + (int)threadIdx.x;
  const int wb = (int)blockIdx.x * NB_BLOCK + (__builtin_amdgcn_readfirstlane((int)threadIdx.x) & ~63);  // wave's first query
  const int a = (int)blockIdx.y * seg_len, b = min(a + seg_len, N);
  const int qi = i < N ? i : N - 1;                                   // lanes past N sweep a copy of the last point
  const float qx = p[3 * (int64_t)qi], qy = p[3 * (int64_t)qi + 1], qz = p[3 * (int64_t)qi + 2];
  float d[K];
  int32_t jj[K];
  gsr_nb_init(d, jj);
  const int t0 = min(max(wb, a), b), t1 = min(max(wb + 64, a), b);   // the self tile clipped to the segment
  knn_sweep<K, false>(p, a, t0, qx, qy, qz, i, d, jj);
  knn_sweep<K, true>(p, t0, t1, qx, qy, qz, i, d, jj);
  knn_sweep<K, false>(p, t1, b, qx, qy, qz, i, d, jj);
  if (i >= N) return;
  if (gridDim.y == 1) {
    knn_write(i, d, jj, dist2, idx, scale);
    return;
  }
  const int64_t o = ((int64_t)blockIdx.y * N + i) * K;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    part_d[o + t] = d[t];
    part_j[o + t] = jj[t];
  }
}

// One thread per query: the list of segment 0, then those of segments 1 .. S-1 inserted in order.
template <int K>
__global__ __launch_bounds__(NB_BLOCK) void knn_merge_kernel(const float* __restrict__ part_d,
                                                              const int32_t* __restrict__ part_j, int N, int S,
                                                              float* __restrict__ dist2, int64_t* __restrict__ idx,
                                                              float* __restrict__ scale) {
  const int i = (int)blockIdx.x * NB_BLOCK + (int)threadIdx.x;
  if (i >= N) return;
  float d[K];
  int32_t jj[K];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    d[t] = part_d[(int64_t)i * K + t];
    jj[t] = part_j[(int64_t)i * K + t];
  }
  for (int s = 1; s < S; ++s) {
    const int64_t o = ((int64_t)s * N + i) * K;
#pragma unroll
    for (int t = 0; t < K; ++t) gsr_nb_insert(d, jj, part_d[o + t], part_j[o + t]);
  }
  knn_write(i, d, jj, dist2, idx, scale);
}

template <int K>
int knn_launch(const float* points, int N, float* dist2, int64_t* idx, float* scale, void* workspace, hipStream_t stream) {
  int64_t seg_len;
  int S;
  knn_segments(N, seg_len, S);
  float* part_d = static_cast<float*>(workspace);
  int32_t* part_j = reinterpret_cast<int32_t*>(static_cast<uint8_t*>(workspace) +
                                               align256(sizeof(float) * (size_t)S * N * K));
  knn_kernel<K><<<dim3(grid_for(N, NB_BLOCK), S), NB_BLOCK, 0, stream>>>(points, N, (int)seg_len, dist2, idx, scale,
                                                                          part_d, part_j);
  GSR_CHECK_LAUNCH();
  if (S > 1) {
    knn_merge_kernel<K><<<grid_for(N, NB_BLOCK), NB_BLOCK, 0, stream>>>(part_d, part_j, N, S, dist2, idx, scale);
    GSR_CHECK_LAUNCH();
  }
  return GSR_OK;
}

// ---- k-means ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(NB_BLOCK) void km_assign_kernel(const float* __restrict__ x, int N,
                                                              const float* __restrict__ cent, int K,
                                                              int64_t* __restrict__ labels, uint32_t* __restrict__ keys) {
  const int i = (int)blockIdx.x * NB_BLOCK + (int)threadIdx.x;
  if (i >= N) return;
  const float qx = x[3 * (int64_t)i], qy = x[3 * (int64_t)i + 1], qz = x[3 * (int64_t)i + 2];
  float best = INFINITY;
  int32_t label = 0;
  int j = 0;
  for (; j + NB_STEP <= K; j += NB_STEP) {
    const float* c = cent + 3 * (int64_t)j;
#pragma unroll
    for (int u = 0; u < NB_STEP; ++u)
      gsr_nb_argmin_step(best, label, gsr_nb_dist2(qx, qy, qz, c[3 * u], c[3 * u + 1], c[3 * u + 2]), j + u);
  }
  for (; j < K; ++j) {
    const float* c = cent + 3 * (int64_t)j;
    gsr_nb_argmin_step(best, label, gsr_nb_dist2(qx, qy, qz, c[0], c[1], c[2]), j);
  }
  if (labels) labels[i] = label;
  if (keys) keys[i] = (uint32_t)label;
}

// Thread c: sorted positions [c KM_CH, (c + 1) KM_CH) ∩ [0, N).
__global__ __launch_bounds__(NB_BLOCK) void km_chunk_sum_kernel(const float* __restrict__ x,
                                                                 const uint32_t* __restrict__ skeys,
                                                                 const uint32_t* __restrict__ svals, int N,
                                                                 float* __restrict__ slots) {
  const int64_t p0 = ((int64_t)blockIdx.x * NB_BLOCK + threadIdx.x) * KM_CH;
  if (p0 >= N) return;
  const int n = (int)min((int64_t)KM_CH, (int64_t)N - p0);
  uint32_t key[KM_CH], v[KM_CH];
  if (n == KM_CH) {
    const uint4* k4 = reinterpret_cast<const uint4*>(skeys + p0);
    const uint4* v4 = reinterpret_cast<const uint4*>(svals + p0);
#pragma unroll
    for (int q = 0; q < KM_CH / 4; ++q) {
      const uint4 a = k4[q], b = v4[q];
      key[4 * q] = a.x; key[4 * q + 1] = a.y; key[4 * q + 2] = a.z; key[4 * q + 3] = a.w;
      v[4 * q] = b.x; v[4 * q + 1] = b.y; v[4 * q + 2] = b.z; v[4 * q + 3] = b.w;
    }
  } else {
#pragma unroll
    for (int u = 0; u < KM_CH; ++u) {
      key[u] = u < n ? skeys[p0 + u] : 0u;
      v[u] = u < n ? svals[p0 + u] : 0u;
    }
  }
  float px[KM_CH], py[KM_CH], pz[KM_CH];
#pragma unroll
  for (int u = 0; u < KM_CH; ++u) {
    const float* q = x + 3 * (int64_t)v[u];
    px[u] = u < n ? q[0] : 0.f;
    py[u] = u < n ? q[1] : 0.f;
    pz[u] = u < n ? q[2] : 0.f;
  }
  float sx = px[0], sy = py[0], sz = pz[0];
  int64_t start = p0;
#pragma unroll
  for (int u = 1; u < KM_CH; ++u) {
    if (u < n) {
      if (key[u] != key[u - 1]) {
        slots[3 * start] = sx; slots[3 * start + 1] = sy; slots[3 * start + 2] = sz;
        start = p0 + u;
        sx = px[u]; sy = py[u]; sz = pz[u];
      } else {
        sx += px[u]; sy += py[u]; sz += pz[u];
      }
    }
  }
  slots[3 * start] = sx; slots[3 * start + 1] = sy; slots[3 * start + 2] = sz;
}

// One wave per cluster; range [K, 2] from gsr_tile_ranges (zero-filled first: an absent cluster reads [0, 0)).
__global__ __launch_bounds__(NB_BLOCK) void km_finish_kernel(const float* __restrict__ slots,
                                                              const uint32_t* __restrict__ range, int K,
                                                              float* __restrict__ cent) {
  const int c = (int)blockIdx.x * (NB_BLOCK / 64) + (__builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6);
  if (c >= K) return;
  const int64_t s = range[2 * c], e = range[2 * c + 1];
  if (e <= s) return;                                      // empty: the centroid stays
  const int64_t first = s / KM_CH + 1, last = (e - 1) / KM_CH;
  const int64_t T = 1 + (last >= first ? last - first + 1 : 0);
  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int64_t t = gsr_lane(); t < T; t += 64) {
    const int64_t pos = t == 0 ? s : (first + t - 1) * KM_CH;
    ax += slots[3 * pos];
    ay += slots[3 * pos + 1];
    az += slots[3 * pos + 2];
  }
  ax = gsr_wave_sum_to_lane63(ax);
  ay = gsr_wave_sum_to_lane63(ay);
  az = gsr_wave_sum_to_lane63(az);
  if (gsr_lane() == 63) {
    const float n = (float)(e - s);
    cent[3 * c] = ax / n;
    cent[3 * c + 1] = ay / n;
    cent[3 * c + 2] = az / n;
  }
}

int bit_length(int64_t v) {
  int b = 0;
  while (v > 0) { ++b; v >>= 1; }
  return b;
}

struct KmWork {
  uint32_t *keys_a, *vals_a, *keys_b, *vals_b, *range;
  float* slots;
  void* sort_ws;
  size_t sort_bytes, total;
};

KmWork km_layout(int64_t N, int64_t K, void* base) {
  KmWork w{};
  uint8_t* p = static_cast<uint8_t*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) { uint8_t* q = p ? p + off : nullptr; off += align256(bytes); return q; };
  w.keys_a = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * N));
  w.vals_a = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * N));
  w.keys_b = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * N));
  w.vals_b = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * N));
  w.range = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * 2 * K));
  w.slots = reinterpret_cast<float*>(take(sizeof(float) * 3 * N));
  w.sort_bytes = gsr_sort_workspace_bytes(N);
  w.sort_ws = take(w.sort_bytes);
  w.total = off;
  return w;
}

bool km_args_ok(const float* x, int64_t N, const float* centroids, int64_t K) {
  return x && centroids && N >= 1 && N <= GSR_NEIGHBOURS_MAX_N && K >= 1 && K <= GSR_NEIGHBOURS_MAX_N;
}

}  // namespace

extern "C" {

size_t gsr_knn_workspace_bytes(int64_t N, int32_t k) {
  if (N < 2 || N > GSR_NEIGHBOURS_MAX_N || k < 1 || k > GSR_KNN_MAX_K) return 0;
  int64_t seg_len;
  int S;
  knn_segments(N, seg_len, S);
  if (S == 1) return 256;
  return align256(sizeof(float) * (size_t)S * N * k) + align256(sizeof(int32_t) * (size_t)S * N * k);
}

int gsr_knn(const float* points, int64_t N, int32_t k, float* dist2_out, int64_t* idx_out, float* scale_out,
            void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!points || !dist2_out || !idx_out || k < 1 || k > GSR_KNN_MAX_K || N < k + 1 || N > GSR_NEIGHBOURS_MAX_N)
    return GSR_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < gsr_knn_workspace_bytes(N, k)) return GSR_ERR_WORKSPACE_TOO_SMALL;
  const int n = (int)N;
  int rc = GSR_ERR_INVALID_ARGUMENT;
  gsr_pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(k, [&](auto kk) {
    rc = knn_launch<decltype(kk)::value>(points, n, dist2_out, idx_out, scale_out, workspace, stream);
  });
  return rc;
}

int gsr_assign_clusters(const float* x, int64_t N, const float* centroids, int64_t K, int64_t* labels_out,
                        void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!km_args_ok(x, N, centroids, K) || !labels_out) return GSR_ERR_INVALID_ARGUMENT;
  km_assign_kernel<<<grid_for(N, NB_BLOCK), NB_BLOCK, 0, stream>>>(x, (int)N, centroids, (int)K, labels_out, nullptr);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

size_t gsr_kmeans_workspace_bytes(int64_t N, int64_t K) {
  if (N < 1 || N > GSR_NEIGHBOURS_MAX_N || K < 1 || K > GSR_NEIGHBOURS_MAX_N) return 0;
  return km_layout(N, K, nullptr).total;
}

int gsr_kmeans_iter(const float* x, int64_t N, float* centroids, int64_t K, int32_t iters, int64_t* labels_out,
                    void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!km_args_ok(x, N, centroids, K) || !labels_out || iters < 1) return GSR_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < gsr_kmeans_workspace_bytes(N, K)) return GSR_ERR_WORKSPACE_TOO_SMALL;
  const KmWork w = km_layout(N, K, workspace);
  const int n = (int)N, kk = (int)K, bits = bit_length(K - 1);
  for (int it = 0; it < iters; ++it) {
    km_assign_kernel<<<grid_for(N, NB_BLOCK), NB_BLOCK, 0, stream>>>(x, n, centroids, kk,
                                                                     it == iters - 1 ? labels_out : nullptr, w.keys_a);
    GSR_CHECK_LAUNCH();
    const int where = gsr_sort_pairs_u32(w.keys_a, w.vals_a, w.keys_b, w.vals_b, N, 1, 0, bits, w.sort_ws, w.sort_bytes,
                                         nullptr, stream_);
    if (where < 0) return where;
    const uint32_t* skeys = where ? w.keys_b : w.keys_a;
    const uint32_t* svals = where ? w.vals_b : w.vals_a;
    if (hipMemsetAsync(w.range, 0, sizeof(uint32_t) * 2 * K, stream) != hipSuccess) return GSR_ERR_LAUNCH_FAILED;
    const int rc = gsr_tile_ranges(skeys, N, kk, w.range, nullptr, stream_);
    if (rc < 0) return rc;
    km_chunk_sum_kernel<<<grid_for((N + KM_CH - 1) / KM_CH, NB_BLOCK), NB_BLOCK, 0, stream>>>(x, skeys, svals, n,
                                                                                               w.slots);
    GSR_CHECK_LAUNCH();
    km_finish_kernel<<<grid_for(K, NB_BLOCK / 64), NB_BLOCK, 0, stream>>>(w.slots, w.range, kk, centroids);
    GSR_CHECK_LAUNCH();
  }
  return GSR_OK;
}

}  // extern "C"
