// The MCMC relocation move: opacity-weighted draws, the opacity / scale correction of a source and its copies, and the
// row move.  The arithmetic is in gsr_relocate.h, the contract in include/gsplat_hip.h.
//
// The prefix of the weights is held per block of 256 rows (one uint64 each: 94 KB at 3 M rows, L2-resident), not per row:
// a full uint64 prefix would be a 24 MB array written and then probed 22 times per draw, and a relocation round draws
// for 5 % of the rows.
//
// reloc_block_totals_kernel  a wave owns a block of 256 rows: lane l loads the four weights 4 l .. 4 l + 3 as one 16-byte
//                            word, the wave's sum in uint64 is the block's total; the block's counts are zero-filled.
// reloc_scan_kernel          ONE workgroup of 1024 turns the totals into inclusive prefixes in place, 1024 per pass with
//                            the carry in a register, and writes S.  12 passes at 3 M rows.
// reloc_draw_kernel          a wave owns a draw.  t is formed in every lane.  The block is found by a 64-way search over
//                            the block prefixes -- every lane probes one pivot, a ballot gives the first whose prefix
//                            exceeds t: four rounds cover 2^23 blocks -- and the row by the wave's prefix of the block's
//                            256 weights and a ballot.  The lane that holds the row stores it and counts it.
// reloc_weights_kernel       one lane per row.
// reloc_rescale_kernel       rows with a count are sparse (5 % in a normal round).  As mcmc_noise_kernel: a wave owns 256
//                            rows in four slots of 64, ballots of "count > 0", then lane j takes the j-th such row, so the
//                            51-term loop runs with every lane busy.
// reloc_rows_kernel          a workgroup owns 256 moves: the index pairs are staged in LDS once, then every column
//                            streams its rows, consecutive lanes on consecutive words of a row.
// No float atomics, no generator state: every output is a function of the inputs alone.
#include "gsr_device.h"
#include "gsr_host.h"
#include "gsr_relocate.h"

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_SCAN_THREADS = 1024;
constexpr int RL_SLOTS = 4;                  // slots of 64 rows a wave of the rescale tests
static_assert(GSR_RELOC_BLOCK == 4 * GSR_WAVE, "a lane holds four weights of a block");

// the weights r .. r + 3 (r a multiple of 4, the array 16-byte aligned), 0 past the end
__device__ __forceinline__ uint4 load_weights4(const uint32_t* __restrict__ w, int64_t r, int64_t N) {
  if (r + 3 < N) return *reinterpret_cast<const uint4*>(w + r);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (r < N) v.x = w[r];
  if (r + 1 < N) v.y = w[r + 1];
  if (r + 2 < N) v.z = w[r + 2];
  return v;
}

__global__ __launch_bounds__(RL_THREADS) void reloc_block_totals_kernel(const uint32_t* __restrict__ weights, int64_t N,
                                                                        int64_t blocks, int32_t* __restrict__ counts,
                                                                        uint64_t* __restrict__ block_total) {
  const int lane = gsr_lane();
  const int64_t b = (int64_t)blockIdx.x * (RL_THREADS / GSR_WAVE) + (threadIdx.x >> 6);
  if (b >= blocks) return;                   // (the whole wave)
  const int64_t r = b * GSR_RELOC_BLOCK + 4 * lane;
  const uint4 w = load_weights4(weights, r, N);
  if (r + 3 < N) {
    *reinterpret_cast<int4*>(counts + r) = make_int4(0, 0, 0, 0);
  } else {
    for (int64_t i = r; i < N; ++i) counts[i] = 0;
  }
  const uint64_t total = gsr_wave_sum_u64(((uint64_t)w.x + w.y) + ((uint64_t)w.z + w.w));
  if (lane == 0) block_total[b] = total;
}

__global__ __launch_bounds__(RL_SCAN_THREADS) void reloc_scan_kernel(uint64_t* __restrict__ block_incl, int64_t blocks,
                                                                     uint64_t* __restrict__ total_out) {
  constexpr int WAVES = RL_SCAN_THREADS / GSR_WAVE;
  const int wave = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (int64_t base = 0; base < blocks; base += RL_SCAN_THREADS) {
    const int64_t i = base + threadIdx.x;
    const uint64_t incl = gsr_wave_scan_incl_u64(i < blocks ? block_incl[i] : 0ull);
    const GsrWaves<uint64_t, WAVES>& s_wave = gsr_block_handoff<63, WAVES>(incl, wave);
    uint64_t before = carry, chunk = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      before += w < wave ? s_wave[w] : 0ull;
      chunk += s_wave[w];
    }
    if (i < blocks) block_incl[i] = before + incl;
    carry += chunk;
    __syncthreads();                         // the hand-off array is written again in the next pass
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(RL_THREADS) void reloc_draw_kernel(const uint32_t* __restrict__ weights, int64_t N,
                                                                const uint64_t* __restrict__ block_incl, int blocks,
                                                                const uint64_t* __restrict__ total, int64_t n,
                                                                uint64_t seed, uint64_t step, uint32_t domain,
                                                                int32_t* __restrict__ sources,
                                                                int32_t* __restrict__ counts) {
  const int lane = gsr_lane();
  const int64_t k = (int64_t)blockIdx.x * (RL_THREADS / GSR_WAVE) + (threadIdx.x >> 6);
  if (k >= n) return;                        // (the whole wave)
  const uint64_t S = *total;
  if (S == 0) {
    if (lane == 0) sources[k] = -1;
    return;
  }
  const uint64_t t = gsr_reloc_target((uint64_t)k, seed, step, domain, S);      // t < S = block_incl[blocks - 1]
  // the first block whose prefix exceeds t lies in [lo, hi)
  int lo = 0, hi = blocks;
  while (hi - lo > 1) {
    const int stride = (hi - lo + 63) >> 6;
    const int pivot = min(lo + (lane + 1) * stride, hi) - 1;                    // the last lanes probe block hi - 1: true
    const uint64_t above = __ballot(block_incl[pivot] > t);
    const int first = above ? __builtin_ctzll(above) : 63;
    hi = min(lo + (first + 1) * stride, hi);
    lo = lo + first * stride;
  }
  const uint64_t base = lo ? block_incl[lo - 1] : 0ull;
  const int64_t r = (int64_t)lo * GSR_RELOC_BLOCK + 4 * lane;
  const uint4 w = load_weights4(weights, r, N);
  const uint64_t p0 = w.x, p1 = p0 + w.y, p2 = p1 + w.z, p3 = p2 + w.w;
  const uint64_t before = base + (gsr_wave_scan_incl_u64(p3) - p3);             // P of the row in front of this lane's
  const uint64_t holds = __ballot(before + p3 > t);
  if (holds == 0) {                          // (weights that changed under the call: no row is named)
    if (lane == 0) sources[k] = -1;
    return;
  }
  if (lane == __builtin_ctzll(holds)) {
    // a row past N has weight 0 and is never the first whose prefix exceeds t
    const int j = before + p0 > t ? 0 : before + p1 > t ? 1 : before + p2 > t ? 2 : 3;
    const int32_t i = (int32_t)(r + j);
    sources[k] = i;
    atomicAdd(counts + i, 1);
  }
}

__global__ __launch_bounds__(RL_THREADS) void reloc_weights_kernel(const float* __restrict__ alpha_logit,
                                                                   const uint8_t* __restrict__ alive, int64_t N,
                                                                   uint32_t* __restrict__ weights) {
  const int64_t i = (int64_t)blockIdx.x * RL_THREADS + threadIdx.x;
  if (i < N) weights[i] = gsr_reloc_weight(alpha_logit[i], alive ? alive[i] != 0 : true);
}

__global__ __launch_bounds__(RL_THREADS) void reloc_rescale_kernel(float* __restrict__ alpha_logit,
                                                                   float* __restrict__ log_scaling,
                                                                   const int32_t* __restrict__ counts, int64_t N,
                                                                   double o_floor) {
  const int lane = gsr_lane();
  const int64_t wave_row0 = ((int64_t)blockIdx.x * RL_THREADS + (threadIdx.x - lane)) * RL_SLOTS;
  if (wave_row0 >= N) return;                // (the whole wave)
  uint64_t mask[RL_SLOTS];
#pragma unroll
  for (int k = 0; k < RL_SLOTS; ++k) {
    const int64_t r = wave_row0 + 64 * k + lane;
    mask[k] = __ballot(r < N && counts[r] > 0);
  }
  const int s1 = __popcll(mask[0]), s2 = s1 + __popcll(mask[1]), s3 = s2 + __popcll(mask[2]), total = s3 + __popcll(mask[3]);
  for (int j = lane; j < total; j += 64) {
    const int k = (j >= s1) + (j >= s2) + (j >= s3);
    const uint64_t m = k == 0 ? mask[0] : k == 1 ? mask[1] : k == 2 ? mask[2] : mask[3];
    const int first = k == 0 ? 0 : k == 1 ? s1 : k == 2 ? s2 : s3;
    const int64_t r = wave_row0 + 64 * k + gsr_nth_set_bit(m, j - first);       // a source row: r < N, counts[r] > 0
    const int32_t c = counts[r];
    const float a = alpha_logit[r], l0 = log_scaling[3 * r], l1 = log_scaling[3 * r + 1], l2 = log_scaling[3 * r + 2];
    float a_new;
    double log_coeff;
    gsr_reloc_rescale(a, c, o_floor, &a_new, &log_coeff);
    alpha_logit[r] = a_new;
    log_scaling[3 * r] = (float)((double)l0 + log_coeff);
    log_scaling[3 * r + 1] = (float)((double)l1 + log_coeff);
    log_scaling[3 * r + 2] = (float)((double)l2 + log_coeff);
  }
}

struct RowColumnSet {
  GsrRowColumnC col[GSR_MAX_COLUMNS];
  int n;
};

// `rows` moves of one column in units of T: `units` of them per row
template <class T>
__device__ __forceinline__ void move_rows(T* __restrict__ data, uint32_t units, bool zero, const int32_t* s_dst,
                                          const int32_t* s_src, uint32_t rows) {
  T nothing;
  memset(&nothing, 0, sizeof(T));
  const uint32_t total = rows * units;       // <= 256 * 2^20: the wrapper bounds the width
  for (uint32_t e = threadIdx.x; e < total; e += RL_THREADS) {
    const uint32_t k = e / units, d = e - k * units;
    const int32_t dst = s_dst[k], src = s_src[k];
    if (dst < 0) continue;
    if (zero) {
      data[(int64_t)dst * units + d] = nothing;
      data[(int64_t)src * units + d] = nothing;
    } else {
      data[(int64_t)dst * units + d] = data[(int64_t)src * units + d];
    }
  }
}

__global__ __launch_bounds__(RL_THREADS) void reloc_rows_kernel(const int32_t* __restrict__ dst_rows,
                                                                const int32_t* __restrict__ src_rows, int64_t n,
                                                                int64_t N, RowColumnSet cs) {
  __shared__ int32_t s_dst[RL_THREADS], s_src[RL_THREADS];
  const int64_t k0 = (int64_t)blockIdx.x * RL_THREADS, k = k0 + threadIdx.x;
  int32_t dst = -1, src = -1;
  if (k < n) {
    dst = dst_rows[k];
    src = src_rows[k];
    if (dst < 0 || dst >= N || src < 0 || src >= N) dst = -1;                   // this k is skipped
  }
  s_dst[threadIdx.x] = dst;
  s_src[threadIdx.x] = src;
  __syncthreads();
  const uint32_t rows = (uint32_t)min((int64_t)RL_THREADS, n - k0);
  for (int c = 0; c < cs.n; ++c) {
    const uint32_t w = (uint32_t)cs.col[c].width_dwords;
    const uintptr_t at = reinterpret_cast<uintptr_t>(cs.col[c].data);
    const bool zero = cs.col[c].zero != 0;
    if ((w & 3u) == 0 && (at & 15) == 0) move_rows(reinterpret_cast<uint4*>(at), w >> 2, zero, s_dst, s_src, rows);
    else if ((w & 1u) == 0 && (at & 7) == 0) move_rows(reinterpret_cast<uint2*>(at), w >> 1, zero, s_dst, s_src, rows);
    else move_rows(reinterpret_cast<uint32_t*>(at), w, zero, s_dst, s_src, rows);
  }
}

}  // namespace

extern "C" {

size_t gsr_weighted_draws_workspace_bytes(int64_t N) { return gsr_reloc_draws_workspace(N); }

int gsr_weighted_draws(const uint32_t* weights, int64_t N, int64_t n, uint64_t seed, uint64_t step, int32_t domain,
                       int32_t* sources_out, int32_t* counts_out, uint64_t* total_out, void* workspace,
                       size_t workspace_bytes, void* stream_) {
  GSR_TRY(gsr_weighted_draws_check(weights, N, n, domain, sources_out, counts_out, total_out, workspace, workspace_bytes));
  hipStream_t stream = gsr_stream(stream_);
  uint64_t* block_incl = reinterpret_cast<uint64_t*>(workspace);
  const int64_t blocks = (N + GSR_RELOC_BLOCK - 1) / GSR_RELOC_BLOCK;           // <= 2^23
  if (blocks > 0) {
    reloc_block_totals_kernel<<<grid_for(blocks, RL_THREADS / GSR_WAVE), RL_THREADS, 0, stream>>>(weights, N, blocks,
                                                                                                  counts_out, block_incl);
    GSR_CHECK_LAUNCH();
  }
  reloc_scan_kernel<<<1, RL_SCAN_THREADS, 0, stream>>>(block_incl, blocks, total_out);
  GSR_CHECK_LAUNCH();
  if (n > 0) {
    reloc_draw_kernel<<<grid_for(n, RL_THREADS / GSR_WAVE), RL_THREADS, 0, stream>>>(
        weights, N, block_incl, (int)blocks, total_out, n, seed, step, (uint32_t)domain, sources_out, counts_out);
    GSR_CHECK_LAUNCH();
  }
  return GSR_OK;
}

int gsr_relocate_weights(const float* alpha_logit, const uint8_t* alive, int64_t N, uint32_t* weights_out, void* stream_) {
  int launch = 0;
  const int rc = gsr_relocate_weights_check(alpha_logit, N, weights_out, &launch);
  if (rc < 0 || !launch) return rc;
  reloc_weights_kernel<<<grid_for(N, RL_THREADS), RL_THREADS, 0, gsr_stream(stream_)>>>(alpha_logit, alive, N, weights_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_relocate_rescale(float* alpha_logit, float* log_scaling, const int32_t* counts, int64_t N, float o_floor,
                         void* stream_) {
  int launch = 0;
  const int rc = gsr_relocate_rescale_check(alpha_logit, log_scaling, counts, N, o_floor, &launch);
  if (rc < 0 || !launch) return rc;
  reloc_rescale_kernel<<<grid_for(N, RL_THREADS * RL_SLOTS), RL_THREADS, 0, gsr_stream(stream_)>>>(
      alpha_logit, log_scaling, counts, N, (double)o_floor);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_relocate_rows(const int32_t* dst_rows, const int32_t* src_rows, int64_t n, int64_t N,
                      const GsrRowColumnC* columns_host, int32_t n_columns, void* stream_) {
  int launch = 0;
  const int rc = gsr_relocate_rows_check(dst_rows, src_rows, n, N, columns_host, n_columns, &launch);
  if (rc < 0 || !launch) return rc;
  RowColumnSet cs;
  cs.n = n_columns;
  for (int c = 0; c < n_columns; ++c) cs.col[c] = columns_host[c];
  reloc_rows_kernel<<<grid_for(n, RL_THREADS), RL_THREADS, 0, gsr_stream(stream_)>>>(dst_rows, src_rows, n, N, cs);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
