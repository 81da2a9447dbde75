// Area resize of interleaved uint8 images, (B, Hs, Ws, C) -> (B, Hd, Wd, C) with Hd <= Hs, Wd <= Ws and C in {1, 3}: the
// exact area mean rounded half up, in integers.  The arithmetic is in gsr_image.h, the contract in include/gsplat_hip.h.
//
// image_resize_area_kernel<C>.  A destination row is a run of Wd C bytes ("elements").  A workgroup of 256 threads owns
// 256 / L consecutive elements of `tile_rows` consecutive destination rows of one image, L = 2^log2_lanes lanes to an
// element (L = 1 up to a ratio of 4; more where one output spans many source pixels, so that a span is summed by
// neighbouring lanes and added with xor shuffles).  Its source is the band of rows [first(d0), last(d1 - 1)] and, in
// each, the bytes of the pixels [first(j0), last(j1)]: what it re-reads of its neighbours' is one pixel per side and axis.
//   load     the band goes through LDS, `rows` rows at a time.  A row's bytes start wherever (b Hs + y) Ws C + x C falls,
//            so a row is fetched as the run of aligned 16-byte words that holds it (a word never leaves the page of a
//            byte it holds) and its skew (0 .. 15) is added back on the LDS side.  Every thread takes up to four words
//            of a chunk; the loads of the next chunk are issued before the current one is summed.
//   sum      per staged row, a lane adds weight x byte over its share of the span (bytes read from LDS; the first and
//            the last pixel of a span carry the partial weights, every other one Wd) and the L lanes are added; four
//            rows go through this together, so four LDS reads are in flight and a weight is formed once.  The row
//            sum (< 2^23) goes into a 64-bit accumulator with the row's vertical weight; a source row overlaps at most
//            two destination rows, so a finished row is written out and the accumulator restarts with the remainder.
//   store    the rounded quotient of each element is one byte; lanes whose address is a multiple of 4 fetch the three
//            bytes behind theirs with shuffles and store a word, the bytes in front of the first aligned address of a
//            wave and behind its last whole word go out as bytes.
// A row too long for the LDS buffer (a ratio above about 60) is staged in pieces of 16 KiB, one row at a time.
// No float, no atomics, no scratch; every output byte is a function of the input alone.
#include "gsr_device.h"
#include "gsr_host.h"
#include "gsr_image.h"

namespace {

constexpr int IB = 256;                       // threads per block: 4 waves
constexpr int IMG_LDS_WORDS = 1024;           // 16-byte words of the staging buffer
constexpr int IMG_LOADS = IMG_LDS_WORDS / IB; // words a thread takes per chunk
constexpr int IMG_MAX_ROWS = 16;              // rows staged at a time
constexpr int IMG_GROUP = 4;                  // staged rows a thread sums together
constexpr int IMG_BAND_ROWS = 48;             // source rows a workgroup aims to sweep
constexpr int IMG_MAX_TILE_ROWS = 16;
constexpr int IMG_MAX_BATCH = 65535;          // gridDim.z

struct ImgArgs {
  const uint8_t* src;
  uint8_t* dst;
  int32_t Hs, Ws, Hd, Wd;
  int32_t log2_lanes;      // lanes per element
  int32_t tile_rows;       // destination rows per workgroup
  int32_t row_words;       // 16-byte words per staged row (or piece of one): >= 2
  uint32_t inv_row_words;  // ceil(2^32 / row_words): idx / row_words == umulhi(idx, inv) for idx < IMG_LDS_WORDS
  int32_t rows;            // rows staged at a time; 1 when pieces > 1
  int32_t pieces;          // pieces a row is staged in
  uint64_t m, D;           // gsr_image_divisor
  int32_t shift;
};

template <int C>
__global__ __launch_bounds__(IB) void image_resize_area_kernel(ImgArgs a) {
  __shared__ uint4 s_words[IMG_LDS_WORDS];
  const uint8_t* s_bytes = reinterpret_cast<const uint8_t*>(s_words);
  const int tid = threadIdx.x, lane = tid & 63;
  const int L = 1 << a.log2_lanes, sub = tid & (L - 1);
  const int per_block = IB >> a.log2_lanes, per_wave = 64 >> a.log2_lanes, in_wave = lane >> a.log2_lanes;
  const int n_el = a.Wd * C;
  const int e0 = (int)blockIdx.x * per_block, e1 = min(e0 + per_block, n_el);
  const int e = e0 + (tid >> a.log2_lanes);
  const bool live = e < e1;
  const int ec = live ? e : e1 - 1;
  const int j = ec / C, c = ec - j * C;
  const int i_lo = gsr_area_first(j, a.Ws, a.Wd), i_hi = gsr_area_last(j, a.Ws, a.Wd);
  const uint32_t w_lo = gsr_area_weight(j, i_lo, a.Ws, a.Wd), w_hi = gsr_area_weight(j, i_hi, a.Ws, a.Wd);
  // the block's pixels of a source row, and its rows
  const int x_lo = gsr_area_first(e0 / C, a.Ws, a.Wd), x_hi = gsr_area_last((e1 - 1) / C, a.Ws, a.Wd);
  const int seg = (x_hi + 1 - x_lo) * C;
  const int b = blockIdx.z;
  const int d0 = (int)blockIdx.y * a.tile_rows, d1 = min(d0 + a.tile_rows, a.Hd);
  const int ys0 = gsr_area_first(d0, a.Hs, a.Hd), ys1 = gsr_area_last(d1 - 1, a.Hs, a.Hd) + 1;
  const uint64_t row_bytes = (uint64_t)a.Ws * C;
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.src) + (uint64_t)b * a.Hs * row_bytes + (uint64_t)x_lo * C;
  uint8_t* const out = a.dst + (uint64_t)b * a.Hd * n_el + e;
  const int piece_bytes = a.row_words * 16;

  // the aligned words of rows y0 .. y0 + nrows - 1 (piece p of each) that this thread stages
  uint4 v[IMG_LOADS];
  auto fetch = [&](int y0, int nrows, int p) {
#pragma unroll
    for (int k = 0; k < IMG_LOADS; ++k) {
      const uint32_t idx = (uint32_t)(tid + k * IB), r = __umulhi(idx, a.inv_row_words), wd = idx - r * a.row_words;
      const uintptr_t row = base + (uint64_t)(y0 + (int)r) * row_bytes;
      const uint32_t skew = (uint32_t)(row & 15), words = (skew + (uint32_t)seg + 15u) >> 4, at = wd + (uint32_t)p * a.row_words;
      v[k] = make_uint4(0u, 0u, 0u, 0u);
      if ((int)r < nrows && at < words) v[k] = reinterpret_cast<const uint4*>(row - skew)[at];
    }
  };

  int d = d0;                  // the destination row being summed
  uint64_t acc = 0;
  uint32_t row_sum = 0;        // of the pieces of one row

  // a finished destination row: one byte per element, stored as words where four of a wave's bytes share an aligned word
  auto emit = [&](int row, uint64_t sum) {
    const uint32_t q = gsr_image_round_div(sum, a.m, a.D, a.shift);
    uint8_t* at = out + (uint64_t)row * n_el;
    const int skew = (int)(reinterpret_cast<uintptr_t>(at) & 3);
    const uint32_t q1 = __shfl(q, lane + L, 64), q2 = __shfl(q, lane + 2 * L, 64), q3 = __shfl(q, lane + 3 * L, 64);
    const int head = in_wave - skew;                                   // the element of this wave that starts the word
    const bool in_word = head >= 0 && head + 3 < per_wave && e - skew + 3 < e1;
    if (live && sub == 0) {
      if (!in_word) *at = (uint8_t)q;
      else if (skew == 0) *reinterpret_cast<uint32_t*>(at) = q | (q1 << 8) | (q2 << 16) | (q3 << 24);
    }
  };

  int y0 = ys0, p = 0;
  fetch(y0, min(a.rows, ys1 - y0), p);
  while (y0 < ys1) {
    const int nrows = min(a.rows, ys1 - y0);
    __syncthreads();                                                   // the previous chunk has been read
#pragma unroll
    for (int k = 0; k < IMG_LOADS; ++k) s_words[tid + k * IB] = v[k];
    __syncthreads();
    const int cur_y0 = y0, cur_p = p;
    if (++p == a.pieces) {
      p = 0;
      y0 += a.rows;
    }
    if (y0 < ys1) fetch(y0, min(a.rows, ys1 - y0), p);                  // in flight while this chunk is summed

    // IMG_GROUP rows at a time: their bytes of one pixel are independent loads, and the pixel's weight is formed once
    for (int r0 = 0; r0 < nrows; r0 += IMG_GROUP) {
      int at[IMG_GROUP];             // byte of pixel 0, channel c of each row, relative to the staged piece
#pragma unroll
      for (int k = 0; k < IMG_GROUP; ++k) {
        const int r = min(r0 + k, nrows - 1);                          // (a row past the chunk repeats its last one)
        const int skew = (int)((base + (uint64_t)(cur_y0 + r) * row_bytes) & 15);
        at[k] = r * piece_bytes + skew + c - cur_p * piece_bytes - x_lo * C;
      }
      int first = i_lo + sub, last = i_hi;
      if (a.pieces > 1) {                                              // the pixels of the span that lie in this piece
        const int t = at[0] + x_lo * C;                                // (one row at a time here: r = 0)
        const int lower = x_lo + (t >= 0 ? 0 : (-t + C - 1) / C);
        const int upper = x_lo + (piece_bytes - t + C - 1) / C - 1;    // piece_bytes - t > 0: t < 16 + C
        if (first < lower) first += ((lower - first + L - 1) >> a.log2_lanes) << a.log2_lanes;
        last = min(last, upper);
      }
      uint32_t h[IMG_GROUP] = {};
      for (int i = first, o = first * C; i <= last; i += L, o += L * C) {
        const uint32_t w = i == i_lo ? w_lo : i == i_hi ? w_hi : (uint32_t)a.Wd;
        uint32_t px[IMG_GROUP];
#pragma unroll
        for (int k = 0; k < IMG_GROUP; ++k) px[k] = s_bytes[at[k] + o];
#pragma unroll
        for (int k = 0; k < IMG_GROUP; ++k) h[k] += __umul24(w, px[k]);                   // w <= 2^15, a byte: 24 bits do
      }
      for (int o = L >> 1; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < IMG_GROUP; ++k) h[k] += __shfl_xor(h[k], o, 64);
      }
#pragma unroll
      for (int k = 0; k < IMG_GROUP; ++k) {
        if (r0 + k >= nrows) break;
        const int y = cur_y0 + r0 + k;
        row_sum += h[k];
        if (cur_p != a.pieces - 1) continue;
        const uint32_t whole = row_sum;
        row_sum = 0;
        // row y is whole: into destination row d, and, where it ends d, out with d and into d + 1 with the remainder
        acc += (uint64_t)gsr_area_weight(d, y, a.Hs, a.Hd) * whole;
        if ((uint32_t)(y + 1) * (uint32_t)a.Hd >= (uint32_t)(d + 1) * (uint32_t)a.Hs) {
          emit(d, acc);
          ++d;
          acc = d < d1 ? (uint64_t)gsr_area_weight(d, y, a.Hs, a.Hd) * whole : 0;
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int gsr_image_resize_area_u8(const uint8_t* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, uint8_t* dst, int32_t Hd,
                             int32_t Wd, void* stream_) {
  int launch = 0;
  const int rc = gsr_image_check(src, B, Hs, Ws, C, dst, Hd, Wd, &launch);
  if (rc < 0 || !launch) return rc;
  hipStream_t stream = gsr_stream(stream_);

  ImgArgs a;
  a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
  const GsrImageDivisor dv = gsr_image_divisor(Ws, Hs);
  a.m = dv.m; a.D = dv.D; a.shift = dv.shift;
  // lanes per element: a lane sums about four pixels of a span
  a.log2_lanes = 0;
  while (a.log2_lanes < 6 && (int64_t)Wd * (4 << a.log2_lanes) < Ws) ++a.log2_lanes;
  const int per_block = IB >> a.log2_lanes;
  // the most bytes of a source row a block needs: its elements touch at most `pixels` pixels, those ceil(pixels Ws / Wd) + 1
  const int64_t pixels = (per_block + C - 1) / C + 1;
  int64_t span = (pixels * Ws + Wd - 1) / Wd + 1;
  span = span < Ws ? span : Ws;
  const int64_t row_words = (15 + span * C + 15) / 16;                 // with the largest skew in front
  if (row_words <= IMG_LDS_WORDS) {
    a.row_words = row_words < 2 ? 2 : (int32_t)row_words;
    a.rows = IMG_LDS_WORDS / a.row_words < IMG_MAX_ROWS ? IMG_LDS_WORDS / a.row_words : IMG_MAX_ROWS;
    a.pieces = 1;
  } else {
    a.row_words = IMG_LDS_WORDS;
    a.rows = 1;
    a.pieces = (int32_t)((row_words + IMG_LDS_WORDS - 1) / IMG_LDS_WORDS);
  }
  a.inv_row_words = (uint32_t)((((uint64_t)1 << 32) + a.row_words - 1) / a.row_words);
  const int64_t tile_rows = (int64_t)IMG_BAND_ROWS * Hd / Hs;
  a.tile_rows = tile_rows < 1 ? 1 : tile_rows > IMG_MAX_TILE_ROWS ? IMG_MAX_TILE_ROWS : (int32_t)tile_rows;

  const unsigned gx = grid_for((int64_t)Wd * C, per_block), gy = grid_for(Hd, a.tile_rows);
  for (int32_t b0 = 0; b0 < B; b0 += IMG_MAX_BATCH) {
    const int32_t nb = B - b0 < IMG_MAX_BATCH ? B - b0 : IMG_MAX_BATCH;
    a.src = src + (uint64_t)b0 * Hs * Ws * C;
    a.dst = dst + (uint64_t)b0 * Hd * Wd * C;
    gsr_pick<1, 3>(C, [&](auto c) {
      image_resize_area_kernel<decltype(c)::value><<<dim3(gx, gy, (unsigned)nb), IB, 0, stream>>>(a);
    });
    GSR_CHECK_LAUNCH();
  }
  return GSR_OK;
}

}  // extern "C"
