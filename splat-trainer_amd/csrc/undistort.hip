// Lens undistortion of interleaved uint8 images: the map of a distorted camera onto a pinhole target, and the bilinear
// remap through such a map.  The arithmetic is in gsr_undistort.h, the contract in include/gsplat_hip.h.
//
// undistort_map_kernel.  One thread per destination pixel, fp64, one 8-byte store per pixel.  Once per camera.
//
// image_remap_kernel<C>.  A workgroup of 256 threads owns `cols` consecutive pixels (64, 128 or 256: the smallest that
// holds a short row) of RM_ITER 256 / cols consecutive destination rows (8, 16 or 32), and a thread one pixel, with its
// C channels, of RM_ITER of them, every 256 / cols-th row.
//   map      a thread reads the entries of its pixels once, as 8-byte loads, and keeps of each the four taps' place
//            inside the box and their weights, in registers, for every image of the batch.
//   box      the smallest rectangle of source pixels that holds every tap of the workgroup, by a min / max over it.
//   sweep    the images b = z RM_SWEEP .. of the batch in turn.  The box of one image goes through LDS: a row's bytes
//            start wherever (b Hs + y) Ws C + x C falls, so a row is fetched as the run of aligned 16-byte words that
//            holds it (a word never leaves the page of a byte it holds) and its skew (0 .. 15) is added back on the LDS
//            side.  Every thread takes up to four words; the loads of the next image are issued before the current one
//            is summed.  The four taps are byte reads from LDS.
//   fallback a box that does not fit the buffer (a map that is not smooth) reads its taps from global memory, a byte
//            at a time: correct, not fast.
//   store    a wave's 64 pixels of a row are one run of 64 C bytes.  The lanes put their bytes into a strip of LDS that
//            belongs to the wave, at the run's own offset from an aligned word; then lane w takes word w of the strip and
//            stores it as a dword, and the lanes of the run's first and last, partial, word store those bytes.
// No float, no atomics, no scratch; every output byte is a function of the inputs alone.
#include "gsr_device.h"
#include "gsr_host.h"
#include "gsr_undistort.h"

namespace {

constexpr int RB = 256;                      // threads per block: 4 waves
constexpr int RM_LDS_WORDS = 1024;           // 16-byte words of the staging buffer
constexpr int RM_LOADS = RM_LDS_WORDS / RB;  // words a thread takes per image
constexpr int RM_ITER = 8;                   // pixels (rows of the tile) per thread
constexpr int RM_STRIP = 208;                // bytes of a wave's output strip: 3 + 64 * 3, rounded up to 16
constexpr int RM_SWEEP = 16;                 // images a workgroup sweeps with its map entries in registers
constexpr int RM_MAX_SLICES = 65535;         // gridDim.z

__global__ __launch_bounds__(RB) void undistort_map_kernel(GsrLens m, int32_t Hs, int32_t Ws, int32_t Wd, int2* map_out) {
  const int u = (int)(blockIdx.x * RB + threadIdx.x), v = (int)blockIdx.y;
  if (u >= Wd) return;
  double xs, ys;
  gsr_undistort_point(m, (double)u, (double)v, &xs, &ys);
  map_out[(int64_t)v * Wd + u] = make_int2(gsr_undistort_quantise(xs, Ws), gsr_undistort_quantise(ys, Hs));
}

struct RemapArgs {
  const uint8_t* src;
  const int2* map;
  uint8_t* dst;
  int32_t B, Hs, Ws, Hd, Wd;
  int32_t log2_cols;     // pixels of a row per workgroup: 64, 128 or 256
};

template <int C>
__global__ __launch_bounds__(RB) void image_remap_kernel(RemapArgs a) {
  __shared__ uint4 s_words[RM_LDS_WORDS];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[4][RM_STRIP];
  const uint8_t* s_bytes = reinterpret_cast<const uint8_t*>(s_words);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cols = 1 << a.log2_cols, rows_per_pass = RB >> a.log2_cols;
  const int j0 = (int)blockIdx.x * cols + (tid & (cols - 1));          // this thread's pixel of a row
  const bool in_row = j0 < a.Wd;
  const int j = in_row ? j0 : a.Wd - 1;
  const int d0 = (int)blockIdx.y * (rows_per_pass * RM_ITER) + (tid >> a.log2_cols);      // this thread's first row

  // pass 1: the entries of this thread's pixels and the smallest box of source pixels that holds the workgroup's taps
  int2 entry[RM_ITER];
  int x_lo = a.Ws, x_hi = -1, y_lo = a.Hs, y_hi = -1;
#pragma unroll
  for (int k = 0; k < RM_ITER; ++k) {
    const int d = d0 + k * rows_per_pass;
    entry[k] = make_int2(0, 0);
    if (in_row && d < a.Hd) {
      entry[k] = a.map[(int64_t)d * a.Wd + j];
      const GsrRemapAxis ax = gsr_remap_axis(entry[k].x, a.Ws), ay = gsr_remap_axis(entry[k].y, a.Hs);
      x_lo = min(x_lo, ax.i0); x_hi = max(x_hi, ax.i1);
      y_lo = min(y_lo, ay.i0); y_hi = max(y_hi, ay.i1);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x_lo = min(x_lo, __shfl_xor(x_lo, o, 64)); x_hi = max(x_hi, __shfl_xor(x_hi, o, 64));
    y_lo = min(y_lo, __shfl_xor(y_lo, o, 64)); y_hi = max(y_hi, __shfl_xor(y_hi, o, 64));
  }
  const GsrWaves<int4>& s_box = gsr_block_handoff(make_int4(x_lo, x_hi, y_lo, y_hi), wave);
#pragma unroll
  for (int w = 0; w < 4; ++w) {                                        // (one pixel of the workgroup at least is live)
    x_lo = min(x_lo, s_box[w].x); x_hi = max(x_hi, s_box[w].y);
    y_lo = min(y_lo, s_box[w].z); y_hi = max(y_hi, s_box[w].w);
  }
  const int seg = (x_hi + 1 - x_lo) * C, nrows = y_hi + 1 - y_lo;      // bytes of a row of the box, and its rows
  const int row_words = (15 + seg + 15) >> 4;                          // with the largest skew in front: >= 1
  const uint32_t piece_bytes = (uint32_t)row_words * 16u;
  const bool staged = (int64_t)row_words * nrows <= RM_LDS_WORDS;      // the same for the whole workgroup

  const uint32_t row_bytes = (uint32_t)a.Ws * C;
  const int b0 = (int)blockIdx.z * RM_SWEEP, b1 = min(b0 + RM_SWEEP, a.B);
  // the wave's first pixel of destination row d of image b starts at byte ((b Hd + d) Wd + j) C of dst; Hd Wd C < 2^32
  const int wave_j = j0 - lane, wave_pixels = min(a.Wd - wave_j, 64);  // (cols is a multiple of 64: one row per wave)
  const uint32_t out0 = ((uint32_t)d0 * (uint32_t)a.Wd + (uint32_t)wave_j) * C, out_step = (uint32_t)rows_per_pass * a.Wd * C;

  // the wave's pixels of a finished destination row, q[c] of each lane's; `at` is where the wave's first byte goes
  auto emit = [&](uint8_t* at, const uint32_t (&q)[C]) {
    const int skew = (int)(reinterpret_cast<uintptr_t>(at) & 3), end = skew + wave_pixels * C;
    uint8_t* strip = s_out[wave];
#pragma unroll
    for (int c = 0; c < C; ++c) strip[skew + lane * C + c] = (uint8_t)q[c];
    __builtin_amdgcn_wave_barrier();                                   // (LDS serves a wave's accesses in order)
    const int lo = 4 * lane;
    if (lo >= skew && lo + 4 <= end) {
      *reinterpret_cast<uint32_t*>(at - skew + lo) = *reinterpret_cast<const uint32_t*>(strip + lo);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (lo + t >= skew && lo + t < end) (at - skew)[lo + t] = strip[lo + t];
    }
    __builtin_amdgcn_wave_barrier();
  };

  if (!staged) {                                                       // taps from global memory, the entries read again
    for (int b = b0; b < b1; ++b) {
      const uint8_t* image = a.src + (uint64_t)b * a.Hs * row_bytes;
      uint8_t* out = a.dst + (uint64_t)b * a.Hd * a.Wd * C;
      for (int k = 0; k < RM_ITER; ++k) {
        const int d = d0 + k * rows_per_pass;
        if (d >= a.Hd) break;                                          // the same for a whole wave
        uint32_t q[C] = {};
        if (in_row) {
          const int2 en = a.map[(int64_t)d * a.Wd + j];
          const GsrRemapAxis ax = gsr_remap_axis(en.x, a.Ws), ay = gsr_remap_axis(en.y, a.Hs);
          const uint8_t* r0 = image + (uint64_t)ay.i0 * row_bytes;
          const uint8_t* r1 = image + (uint64_t)ay.i1 * row_bytes;
#pragma unroll
          for (int c = 0; c < C; ++c)
            q[c] = gsr_remap_round(ay.w0 * (ax.w0 * r0[ax.i0 * C + c] + ax.w1 * r0[ax.i1 * C + c]) +
                                   ay.w1 * (ax.w0 * r1[ax.i0 * C + c] + ax.w1 * r1[ax.i1 * C + c]));
        }
        emit(out + (out0 + (uint32_t)k * out_step), q);
      }
    }
    return;
  }

  // pass 2: of each pixel its place in the staged box and its weights, kept for every image of the sweep
  //   place = byte of tap (y0, x0) in a box without skew | (y0 - y_lo) row_bytes mod 16 << 14 | (y1 - y0) << 18 | (x1 - x0) << 19
  uint32_t place[RM_ITER], w01[RM_ITER], w23[RM_ITER];    // wy0 wx0 | wy0 wx1 << 16, wy1 wx0 | wy1 wx1 << 16
#pragma unroll
  for (int k = 0; k < RM_ITER; ++k) {
    const bool live = in_row && d0 + k * rows_per_pass < a.Hd;
    const GsrRemapAxis ax = gsr_remap_axis(entry[k].x, a.Ws), ay = gsr_remap_axis(entry[k].y, a.Hs);
    const uint32_t r0 = live ? (uint32_t)(ay.i0 - y_lo) : 0u, i0 = live ? (uint32_t)(ax.i0 - x_lo) : 0u;
    place[k] = (r0 * piece_bytes + i0 * C) | (((r0 * row_bytes) & 15u) << 14) |
               ((uint32_t)(ay.i1 - ay.i0) << 18) | ((uint32_t)(ax.i1 - ax.i0) << 19);
    w01[k] = live ? (ay.w0 * ax.w0) | ((ay.w0 * ax.w1) << 16) : 0u;
    w23[k] = live ? (ay.w1 * ax.w0) | ((ay.w1 * ax.w1) << 16) : 0u;
  }

  // the word (row of the box, word of the row) each staging slot of this thread holds; the same for every image
  int slot_r[RM_LOADS], slot_w[RM_LOADS];
#pragma unroll
  for (int k = 0; k < RM_LOADS; ++k) {
    const int idx = tid + k * RB;
    slot_r[k] = idx / row_words;
    slot_w[k] = idx - slot_r[k] * row_words;
  }
  // byte 0 of the box's first row in image b
  auto box_base = [&](int b) {
    return reinterpret_cast<uintptr_t>(a.src) + ((uint64_t)b * a.Hs + (uint64_t)y_lo) * row_bytes + (uint64_t)x_lo * C;
  };
  uint4 v[RM_LOADS];
  auto fetch = [&](int b) {
    const uintptr_t base = box_base(b);
#pragma unroll
    for (int k = 0; k < RM_LOADS; ++k) {
      const uintptr_t row = base + (uint64_t)slot_r[k] * row_bytes;
      const uint32_t skew = (uint32_t)(row & 15), words = (skew + (uint32_t)seg + 15u) >> 4;
      v[k] = make_uint4(0u, 0u, 0u, 0u);
      if (slot_r[k] < nrows && (uint32_t)slot_w[k] < words) v[k] = reinterpret_cast<const uint4*>(row - skew)[slot_w[k]];
    }
  };

  fetch(b0);
  for (int b = b0; b < b1; ++b) {
    __syncthreads();                                                   // the previous image has been read
#pragma unroll
    for (int k = 0; k < RM_LOADS; ++k) s_words[tid + k * RB] = v[k];
    __syncthreads();
    // row r of the box starts (skew0 + r row_bytes) mod 16 bytes into its piece
    const uint32_t skew0 = (uint32_t)(box_base(b) & 15), step1 = row_bytes & 15u;
    if (b + 1 < b1) fetch(b + 1);                                      // in flight while this image is summed
    uint8_t* out = a.dst + (uint64_t)b * a.Hd * a.Wd * C;
#pragma unroll
    for (int k = 0; k < RM_ITER; ++k) {
      if (d0 + k * rows_per_pass >= a.Hd) break;                       // the same for a whole wave
      uint32_t pl = place[k], wa = w01[k], wb = w23[k];
      asm volatile("" : "+v"(pl), "+v"(wa), "+v"(wb));                 // unpacked here, per image: not hoisted into registers
      const uint32_t at = pl & 0x3fffu, m0 = skew0 + ((pl >> 14) & 15u);
      const uint32_t dy = (pl >> 18) & 1u, dx = ((pl >> 19) & 1u) * C;
      const uint32_t at0 = at + (m0 & 15u), at1 = at + dy * piece_bytes + ((m0 + dy * step1) & 15u);
      uint32_t q[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint32_t p00 = s_bytes[at0 + c], p01 = s_bytes[at0 + dx + c], p10 = s_bytes[at1 + c], p11 = s_bytes[at1 + dx + c];
        q[c] = gsr_remap_round((wa & 0xffffu) * p00 + (wa >> 16) * p01 + (wb & 0xffffu) * p10 + (wb >> 16) * p11);
      }
      emit(out + (out0 + (uint32_t)k * out_step), q);
    }
  }
}

}  // namespace

extern "C" {

int gsr_undistort_map(const double* source_host, const double* target_host, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd,
                      int32_t* map_out, void* stream_) {
  int launch = 0;
  const int rc = gsr_undistort_map_check(source_host, target_host, Hs, Ws, Hd, Wd, map_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrLens m = gsr_lens_make(source_host, target_host);
  undistort_map_kernel<<<dim3(grid_for(Wd, RB), (unsigned)Hd), RB, 0, gsr_stream(stream_)>>>(
      m, Hs, Ws, Wd, reinterpret_cast<int2*>(map_out));
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_image_remap_u8(const uint8_t* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, const int32_t* map, uint8_t* dst,
                       int32_t Hd, int32_t Wd, void* stream_) {
  int launch = 0;
  const int rc = gsr_image_remap_check(src, B, Hs, Ws, C, map, dst, Hd, Wd, &launch);
  if (rc < 0 || !launch) return rc;
  hipStream_t stream = gsr_stream(stream_);
  if (Hs == 0 || Ws == 0) {                                            // every tap lies outside an empty source
    if (hipMemsetAsync(dst, 0, (size_t)B * Hd * Wd * C, stream) != hipSuccess) return GSR_ERR_LAUNCH_FAILED;
    return GSR_OK;
  }

  RemapArgs a;
  a.map = reinterpret_cast<const int2*>(map);
  a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
  // a short row takes fewer lanes, and the workgroup more rows of it
  a.log2_cols = Wd <= 64 ? 6 : Wd <= 128 ? 7 : 8;
  const int cols = 1 << a.log2_cols, tile_rows = (RB >> a.log2_cols) * RM_ITER;
  const unsigned gx = grid_for(Wd, cols), gy = grid_for(Hd, tile_rows);
  const int32_t per_launch = RM_MAX_SLICES * RM_SWEEP;
  for (int32_t b0 = 0; b0 < B; b0 += per_launch) {
    a.B = B - b0 < per_launch ? B - b0 : per_launch;
    a.src = src + (uint64_t)b0 * Hs * Ws * C;
    a.dst = dst + (uint64_t)b0 * Hd * Wd * C;
    gsr_pick<1, 3>(C, [&](auto c) {
      image_remap_kernel<decltype(c)::value><<<dim3(gx, gy, grid_for(a.B, RM_SWEEP)), RB, 0, stream>>>(a);
    });
    GSR_CHECK_LAUNCH();
  }
  return GSR_OK;
}

}  // extern "C"
