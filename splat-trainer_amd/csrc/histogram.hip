// Histograms of [N, C] float32 tensors for the detailed training logs: gather by row, divide by a per-row weight, log10
// and bin in one sweep.  Per-entry maths in gsr_histogram.h; the contract is in include/gsplat_hip.h.
//
// hist_range_kernel     (auto range only) the minimum and maximum of the kept t as ordered integer keys: per-lane, then
//                       a wave's shuffles, the block's waves through LDS, then one integer atomicMax per block on two
//                       words of the workspace (the minimum is kept as the maximum of the complemented key, so a zeroed
//                       workspace is "empty").
// hist_bin_kernel       per-wave LDS counters (num_bins <= 256; one per-block set above that) filled with integer LDS
//                       atomics, then one global 64-bit integer add per non-empty bin and block.  The four tallies
//                       travel the same way.  The sums of t and t^2 are fp64: a lane adds its own entries in grid-stride
//                       order, the 64 lanes are added in the fixed xor tree, the 4 waves in order, and the block writes
//                       its two partials to its own slot.  No float atomics anywhere.
// hist_finalize_kernel  one block: adds the blocks' partials in a fixed order, adds the replicas and writes the counts
//                       and the eight statistics.
// Where the global adds land.  Adds of many blocks to one word are served one after another, and 64 bins share a few
// cache lines: with one set of words a sweep of a few megabytes spends most of its time there.  So the workspace holds
// HIST_REPLICAS sets of (keys, tallies, counts), 8 KiB apart, a block adds to set blockIdx % HIST_REPLICAS, and the
// finalize pass adds the sets -- integers, so the order does not matter.  A thread takes at least HIST_ITEMS work items
// before the grid grows, which keeps the number of blocks, and with it of adds, in proportion to the data.
// The grid is a function of the number of entries alone, so every output is the same bits on every run, and an
// auto-range call -- whose bin kernel reads (lo, hi) from the workspace, with no host wait -- walks exactly as the
// fixed-range call with that (lo, hi) does.
#include "gsr_device.h"
#include "gsr_histogram.h"
#include "gsr_host.h"

namespace {

constexpr int HB = 256;                       // threads per block: 4 waves
constexpr int HB_WAVES = HB / 64;
constexpr int HIST_MAX_BLOCKS = 2048;
constexpr int HIST_WAVE_BINS = 256;           // up to here every wave has its own counters
constexpr int HIST_REPLICAS = 16;             // sets of global words the blocks' adds are spread over
constexpr int HIST_ITEMS = 8;                 // work items a thread takes before the grid grows
constexpr size_t HIST_HEADER_BYTES = 64;      // 4 keys (uint32) + 4 tallies (uint64), padded
constexpr size_t HIST_REPLICA_BYTES = HIST_HEADER_BYTES + sizeof(uint64_t) * GSR_HISTOGRAM_MAX_BINS;

static_assert((HIST_REPLICA_BYTES & 15) == 0 && GSR_HISTOGRAM_MAX_BINS == HB_WAVES * HIST_WAVE_BINS, "the LDS counters are one array for both layouts");

struct HistIn {
  const float* values;
  const int64_t* rows;
  const float* weight;
  int64_t N;             // rows of values (bound of a gathered index)
  int64_t W;             // work items: gathered rows x chunks
  int64_t chunks;        // work items per row, C / VEC
  int64_t C;             // floats per row
  int64_t tail_start;    // flat form only: the last tail_count (< 4) entries, taken one each by the first lanes of block 0
  int tail_count;
  int small;             // W < 2^31: the row of a work item by a 32-bit division
  float eps;
  int mode;
  float min_value;
};

struct HistHeader {                           // the head of one replica; its counts follow at HIST_HEADER_BYTES
  uint32_t range_min_c, range_max;            // hist_range_kernel: ~key(min), key(max)
  uint32_t min_c, max;                        // hist_bin_kernel: the same of what it kept
  unsigned long long tally[4];                // kept, dropped, non-finite, outside
};
static_assert(sizeof(HistHeader) <= HIST_HEADER_BYTES, "header");

__device__ __forceinline__ HistHeader* hist_replica(void* workspace, int r) {
  return reinterpret_cast<HistHeader*>(reinterpret_cast<char*>(workspace) + (size_t)r * HIST_REPLICA_BYTES);
}

__device__ __forceinline__ unsigned long long* hist_replica_counts(void* workspace, int r) {
  return reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + (size_t)r * HIST_REPLICA_BYTES +
                                               HIST_HEADER_BYTES);
}

// f(class, t) for every entry of the input, VEC consecutive entries of a row per work item
template <int VEC, class F>
__device__ __forceinline__ void hist_for_each(const HistIn& in, F&& f) {
  const bool weighted = in.weight != nullptr;
  const int64_t stride = (int64_t)gridDim.x * HB;
  for (int64_t w = (int64_t)blockIdx.x * HB + threadIdx.x; w < in.W; w += stride) {
    int64_t r = w, j = 0;
    if (in.chunks > 1) {
      r = in.small ? (int64_t)((uint32_t)w / (uint32_t)in.chunks) : w / in.chunks;
      j = w - r * in.chunks;
    }
    const int64_t src = in.rows ? in.rows[r] : r;
    if (src < 0 || src >= in.N) {             // an index outside the tensor is never read: its entries count as non-finite
#pragma unroll
      for (int k = 0; k < VEC; ++k) f(GSR_HIST_NONFINITE, 0.f);
      continue;
    }
    const float wt = weighted ? in.weight[src] : 0.f;
    const float* s = in.values + src * in.C + j * VEC;
    float v[VEC];
    if constexpr (VEC == 4) {
      const float4 q = *reinterpret_cast<const float4*>(s);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = *s;
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float t = 0.f;
      const int cls = gsr_hist_entry(v[k], weighted, wt, in.eps, in.mode, in.min_value, &t);
      f(cls, t);
    }
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < in.tail_count) {
    float t = 0.f;
    const int cls = gsr_hist_entry(in.values[in.tail_start + threadIdx.x], false, 0.f, in.eps, in.mode, in.min_value, &t);
    f(cls, t);
  }
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t n = (uint32_t)__shfl_xor((int)v, o, 64);
    v = n > v ? n : v;
  }
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {     // the fixed xor tree: the same bits in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int VEC>
__global__ __launch_bounds__(HB) void hist_range_kernel(HistIn in, void* __restrict__ workspace) {
  uint32_t min_c = 0u, max_k = 0u;
  hist_for_each<VEC>(in, [&](int cls, float t) {
    if (cls == GSR_HIST_KEPT) {
      const uint32_t k = gsr_hist_key(t);
      min_c = ~k > min_c ? ~k : min_c;
      max_k = k > max_k ? k : max_k;
    }
  });
  min_c = wave_max_u32(min_c);
  max_k = wave_max_u32(max_k);
  const auto s = gsr_block_handoff(min_c, max_k);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < HB_WAVES; ++w) {
      min_c = s.a[w] > min_c ? s.a[w] : min_c;
      max_k = s.b[w] > max_k ? s.b[w] : max_k;
    }
    if (max_k != 0u) {                                      // (a key is never 0: a block that kept nothing adds nothing)
      HistHeader* header = hist_replica(workspace, blockIdx.x % HIST_REPLICAS);
      atomicMax(&header->range_min_c, min_c);
      atomicMax(&header->range_max, max_k);
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(HB) void hist_bin_kernel(HistIn in, float lo, float hi, int from_header, int num_bins,
                                                      int trim, void* __restrict__ workspace,
                                                      double* __restrict__ partials) {
  __shared__ uint32_t s_counts[GSR_HISTOGRAM_MAX_BINS];
  __shared__ uint32_t s_tally[4];
  __shared__ uint32_t s_min[HB_WAVES], s_max[HB_WAVES];
  __shared__ double s_sum[HB_WAVES], s_sq[HB_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int b = tid; b < GSR_HISTOGRAM_MAX_BINS; b += HB) s_counts[b] = 0u;
  if (tid < 4) s_tally[tid] = 0u;
  if (from_header) {                                        // written by hist_range_kernel, earlier on this stream
    uint32_t min_c = 0u, max_k = 0u;
#pragma unroll
    for (int r = 0; r < HIST_REPLICAS; ++r) {
      const HistHeader* h = hist_replica(workspace, r);
      min_c = h->range_min_c > min_c ? h->range_min_c : min_c;
      max_k = h->range_max > max_k ? h->range_max : max_k;
    }
    lo = gsr_hist_unkey(~min_c);
    hi = gsr_hist_unkey(max_k);
  }
  __syncthreads();
  uint32_t* mine = s_counts + (num_bins <= HIST_WAVE_BINS ? wave * HIST_WAVE_BINS : 0);
  uint32_t n_kept = 0u, n_dropped = 0u, n_nonfinite = 0u, n_outside = 0u, min_c = 0u, max_k = 0u;
  double sum = 0.0, sq = 0.0;
  hist_for_each<VEC>(in, [&](int cls, float t) {
    n_dropped += cls == GSR_HIST_DROPPED;
    n_nonfinite += cls == GSR_HIST_NONFINITE;
    if (cls == GSR_HIST_KEPT) {
      ++n_kept;
      const uint32_t k = gsr_hist_key(t);
      min_c = ~k > min_c ? ~k : min_c;
      max_k = k > max_k ? k : max_k;
      int outside;
      const int b = gsr_hist_bin(t, lo, hi, num_bins, trim != 0, &outside);
      n_outside += (uint32_t)outside;
      if (b >= 0) {                                         // b < num_bins by gsr_hist_bin
        atomicAdd(&mine[b], 1u);
        const double td = (double)t;
        sum += td;
        sq += td * td;
      }
    }
  });
  n_kept = gsr_wave_sum_u32(n_kept);
  n_dropped = gsr_wave_sum_u32(n_dropped);
  n_nonfinite = gsr_wave_sum_u32(n_nonfinite);
  n_outside = gsr_wave_sum_u32(n_outside);
  min_c = wave_max_u32(min_c);
  max_k = wave_max_u32(max_k);
  sum = wave_sum_f64(sum);
  sq = wave_sum_f64(sq);
  if (lane == 0) {
    atomicAdd(&s_tally[0], n_kept);
    atomicAdd(&s_tally[1], n_dropped);
    atomicAdd(&s_tally[2], n_nonfinite);
    atomicAdd(&s_tally[3], n_outside);
    s_sum[wave] = sum;
    s_sq[wave] = sq;
    s_min[wave] = min_c;
    s_max[wave] = max_k;
  }
  __syncthreads();
  const int replica = blockIdx.x % HIST_REPLICAS;
  HistHeader* header = hist_replica(workspace, replica);
  unsigned long long* counts = hist_replica_counts(workspace, replica);
  for (int b = tid; b < num_bins; b += HB) {
    uint32_t c = s_counts[b];
    if (num_bins <= HIST_WAVE_BINS)
      c += s_counts[HIST_WAVE_BINS + b] + s_counts[2 * HIST_WAVE_BINS + b] + s_counts[3 * HIST_WAVE_BINS + b];
    if (c) atomicAdd(&counts[b], (unsigned long long)c);
  }
  if (tid < 4 && s_tally[tid]) atomicAdd(&header->tally[tid], (unsigned long long)s_tally[tid]);
  if (tid == 0) {
    partials[2 * blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    partials[2 * blockIdx.x + 1] = ((s_sq[0] + s_sq[1]) + s_sq[2]) + s_sq[3];
#pragma unroll
    for (int w = 1; w < HB_WAVES; ++w) {
      min_c = s_min[w] > min_c ? s_min[w] : min_c;
      max_k = s_max[w] > max_k ? s_max[w] : max_k;
    }
    if (max_k != 0u) {
      atomicMax(&header->min_c, min_c);
      atomicMax(&header->max, max_k);
    }
  }
}

// counts[num_bins] = the replicas' counts added; stats[8] = kept, sum t, sum t^2, min, max, dropped, non-finite, outside
__global__ __launch_bounds__(HB) void hist_finalize_kernel(void* __restrict__ workspace, const double* __restrict__ partials,
                                                           int blocks, int num_bins, unsigned long long* __restrict__ counts,
                                                           double* __restrict__ stats) {
  __shared__ double s_sum[HB], s_sq[HB];
  const int tid = threadIdx.x;
  for (int b = tid; b < num_bins; b += HB) {
    unsigned long long c = 0ull;
#pragma unroll
    for (int r = 0; r < HIST_REPLICAS; ++r) c += hist_replica_counts(workspace, r)[b];
    counts[b] = c;
  }
  double sum = 0.0, sq = 0.0;
  for (int b = tid; b < blocks; b += HB) {
    sum += partials[2 * b];
    sq += partials[2 * b + 1];
  }
  s_sum[tid] = sum;
  s_sq[tid] = sq;
  __syncthreads();
  for (int o = HB / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_sum[tid] += s_sum[tid + o];
      s_sq[tid] += s_sq[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    unsigned long long tally[4] = {0ull, 0ull, 0ull, 0ull};
    uint32_t min_c = 0u, max_k = 0u;
    for (int r = 0; r < HIST_REPLICAS; ++r) {
      const HistHeader* h = hist_replica(workspace, r);
      for (int k = 0; k < 4; ++k) tally[k] += h->tally[k];
      min_c = h->min_c > min_c ? h->min_c : min_c;
      max_k = h->max > max_k ? h->max : max_k;
    }
    const bool any = max_k != 0u;
    stats[0] = (double)tally[0];
    stats[1] = s_sum[0];
    stats[2] = s_sq[0];
    stats[3] = any ? (double)gsr_hist_unkey(~min_c) : 0.0;
    stats[4] = any ? (double)gsr_hist_unkey(max_k) : 0.0;
    stats[5] = (double)tally[1];
    stats[6] = (double)tally[2];
    stats[7] = (double)tally[3];
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int hist_blocks(int64_t W) {
  const int64_t per_block = (int64_t)HB * HIST_ITEMS, b = (W + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : b > HIST_MAX_BLOCKS ? HIST_MAX_BLOCKS : b);
}

}  // namespace

extern "C" {

size_t gsr_histogram_workspace_bytes(void) {
  return HIST_REPLICAS * HIST_REPLICA_BYTES + 2 * sizeof(double) * HIST_MAX_BLOCKS;
}

int gsr_histogram(const float* values, int64_t N, int64_t C, const int64_t* rows, int64_t M, const float* weight,
                  float eps, int32_t mode, float min_value, float lo, float hi, int32_t num_bins, int32_t auto_range,
                  int32_t trim, int64_t* counts, double* stats, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!counts || !stats || N < 0 || M < 0 || C < 1 || mode < 0 || mode > 2 || num_bins < 1 ||
      num_bins > GSR_HISTOGRAM_MAX_BINS || N > GSR_NEIGHBOURS_MAX_N || C > 65536)
    return GSR_ERR_INVALID_ARGUMENT;
  if (!auto_range && !(gsr_hist_finite(lo) && gsr_hist_finite(hi) && hi >= lo)) return GSR_ERR_INVALID_ARGUMENT;
  const int64_t R = rows ? M : N;                      // gathered rows
  if (R == 0 || N == 0) {                              // nothing to sweep: zeros, no launch
    if (hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)num_bins, stream) != hipSuccess) return GSR_ERR_LAUNCH_FAILED;
    if (hipMemsetAsync(stats, 0, sizeof(double) * 8, stream) != hipSuccess) return GSR_ERR_LAUNCH_FAILED;
    return GSR_OK;
  }
  if (!values || !workspace || !aligned16(workspace)) return GSR_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < gsr_histogram_workspace_bytes()) return GSR_ERR_WORKSPACE_TOO_SMALL;

  HistIn in;
  in.values = values; in.rows = rows; in.weight = weight; in.N = N; in.C = C;
  in.tail_start = 0; in.tail_count = 0;
  in.eps = eps; in.mode = mode; in.min_value = min_value;
  int vec = 1;
  if (!rows && !weight) {                              // flat: the tensor is one run of N C entries
    const int64_t E = N * C;
    if (aligned16(values) && E >= 4) {
      vec = 4;
      in.N = E / 4; in.C = 4; in.chunks = 1; in.W = E / 4;
      in.tail_start = 4 * (E / 4); in.tail_count = (int)(E - in.tail_start);
    } else {
      in.N = E; in.C = 1; in.chunks = 1; in.W = E;
    }
  } else if (C % 4 == 0 && aligned16(values)) {
    vec = 4;
    in.chunks = C / 4; in.W = R * in.chunks;
  } else {
    in.chunks = C; in.W = R * C;
  }
  in.small = in.W < 0x7FFFFFFF ? 1 : 0;

  const size_t replica_bytes = HIST_REPLICAS * HIST_REPLICA_BYTES;
  double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + replica_bytes);
  if (hipMemsetAsync(workspace, 0, replica_bytes, stream) != hipSuccess) return GSR_ERR_LAUNCH_FAILED;
  const int blocks = hist_blocks(in.W);
  gsr_pick<1, 4>(vec, [&](auto v) {
    if (auto_range) hist_range_kernel<decltype(v)::value><<<blocks, HB, 0, stream>>>(in, workspace);
    hist_bin_kernel<decltype(v)::value><<<blocks, HB, 0, stream>>>(in, lo, hi, auto_range ? 1 : 0, (int)num_bins, (int)trim,
                                                                   workspace, partials);
  });
  GSR_CHECK_LAUNCH();
  hist_finalize_kernel<<<1, HB, 0, stream>>>(workspace, partials, blocks, (int)num_bins,
                                             reinterpret_cast<unsigned long long*>(counts), stats);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
