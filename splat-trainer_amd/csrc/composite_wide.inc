// Wide feature frames (4 <= C <= 16): K6 and K7 for features kept in a second per-splat table.
//
// Included at the end of composite.hip (it reuses that file's walk helpers: eval_q2 / eval_qt / eval_G2 / eval_alpha2 /
// clamp_alpha2, the packed row loads, the visibility fold, seg_alpha_pass and the segment tables).  The geometry row is
// the ordinary 64-byte row with zero colour slots; the features live in feat_rows [M, CW] (splat order, CW in {4, 8, 16},
// zero-padded past C), fetched by splat id through the scalar cache like the row itself.
//
// The forward walk (wide_walk) takes the same contribute / skip decisions with the same expressions as fwd_walk, so every
// channel, T, last, median and the visibility partials are bit-identical to the C <= 3 path for the same splats and the
// same segment plan.
// The backward walk needs the colour only through the scalar gc = dL/dimage(px) . f per (pixel, splat) pair, as K7 does;
// per pixel it keeps T, the suffix g . (colour behind) and the CW floats of dL/dimage.  Each (tile, splat) pair owns one
// slot of 8 + CW floats (mx my mxx mxy myy m0 prune split | df0 .. df(CW-1)): no float atomics, fixed-order reductions.
//
// Segmented frames (the plan of gsr_segment_plan, the same tables and thresholds as for C <= 3).  Without a plan
// composite_fwd_wide walks every tile with one wave.  With one, wide_ckpt_fwd takes every tile that is not heavy -- a
// short tile as composite_fwd_wide does, a long one pausing at each segment end to leave a checkpoint -- and its extra
// blocks run pass A (seg_alpha_pass<1>: geometry only); heavy tiles then go through wide_seg_fwd (pass C, one wave per
// segment) and wide_seg_combine (pass D, one wave per tile).  composite_bwd_wide gives every segment a block of its own,
// entered from the segment's end state; since it carries the colour behind a splat only as ga = g . (colour behind), that
// entry is one prologue: ga = sum_c g_c (image_c - colour up to the segment's end).
// Pixel slots of a segment (lane-major: slot = 64 p + lane for pixel p of the lane):
//   seg_T    [segment][256] float    T after the segment (pass C: -1 when the pixel was dead at the segment's entry)
//   seg_col  [segment][CW / 4][256] float4   channels 4 q .. 4 q + 3 of the colour composited up to the segment's END
//            (heavy tiles: the segment's own colour until pass D turns it into that prefix): every store and load is one
//            coalesced 16-byte access per lane, 1 KB per wave
//   seg_P / seg_last / seg_median [segment][256] as for C <= 3 (heavy tiles only).

namespace {

template <int CW>
struct FeatRow { float f[CW]; };

// wave-uniform splat id: one s_load_dwordx4 / x8 / x16
template <int CW>
__device__ __forceinline__ FeatRow<CW> load_feat(const float* __restrict__ feat, uint32_t packed) {
  const float4* r = reinterpret_cast<const float4*>(feat + (size_t)CW * (packed & 0x3FFFFFFFu));
  FeatRow<CW> out;
#pragma unroll
  for (int q = 0; q < CW / 4; ++q) {
    const float4 v = r[q];
    out.f[4 * q] = v.x; out.f[4 * q + 1] = v.y; out.f[4 * q + 2] = v.z; out.f[4 * q + 3] = v.w;
  }
  return out;
}

__device__ __forceinline__ uint32_t rank_at(const uint32_t* __restrict__ sorted_rank, uint32_t i) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)sorted_rank[i]);
}

// per-lane pixel state of the wide forward walk: pixel p = 2h + i, half h (rows py0 + 8h), side i (cols px0 + 8i)
template <int CW>
struct WidePix {
  v2f T2[2], col2[2][CW], med2[2];
  int lastc[4];
};

template <int CW>
__device__ __forceinline__ void wide_init(WidePix<CW>& px, int px0, int py0, int W, int H) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const bool in_y = (py0 + 8 * h) < H;
    px.T2[h] = (v2f){(in_y && px0 < W) ? 1.f : 0.f, (in_y && (px0 + 8) < W) ? 1.f : 0.f};
    px.med2[h] = GSR_V2(0.f);
#pragma unroll
    for (int c = 0; c < CW; ++c) px.col2[h][c] = GSR_V2(0.f);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) px.lastc[p] = 0;
}

// Front-to-back walk over list positions [begin, end) of one tile: the same mapping, walk and expressions as fwd_walk's
// row-by-row form (PF = false); `tile_start` makes the recorded last-contributor index tile-relative.
// SGPRs: the geometry row of the NEXT pair is prefetched as there, but a CW = 16 feature row would not fit twice next to
// it (2 x (12 + 16) row words); so the feature row of the next pair is fetched at the END of the current pair, once the
// current one has been consumed, and arrives while the next pair's geometry is evaluated.
template <int CW, bool VIS, bool MEDIAN>
__device__ __forceinline__ void wide_walk(WidePix<CW>& px, const float* __restrict__ rec, const float* __restrict__ feat,
                                          const uint32_t* __restrict__ sorted_rank,
                                          const uint32_t* __restrict__ sorted_inst, uint32_t tile_start, uint32_t begin,
                                          uint32_t end, float fx0, float fy0, const GsrRasterParams& rp, int lane,
                                          float* __restrict__ vis_partial, float* __restrict__ pair_vis) {
  const uint32_t vis_slot = (uint32_t)(((lane >> 4) & 1) * 2 + (lane >> 5));
  if (begin >= end) return;
  uint32_t pk = rank_at(sorted_rank, begin);
  Splat nxt = load_splat_packed<1, MEDIAN>(rec, pk);
  FeatRow<CW> fr = load_feat<CW>(feat, pk);
  for (uint32_t i = begin; i < end; i += 4) {
    float wq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (i + m < end) {                                               // wave-uniform
        const Splat s = nxt;
        pk = rank_at(sorted_rank, min(i + m + 1, end - 1u));          // unconditional, as fwd_walk
        nxt = load_splat_packed<1, MEDIAN>(rec, pk);
        const v2f dx2 = (v2f){fx0, fx0 + 8.f} - GSR_V2(s.u);
        const int idx = (int)(i - tile_start) + m + 1;
        v2f wsum2 = GSR_V2(0.f);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (!(s.halves & (1u << h))) continue;
          const float dy = (h ? fy0 + 8.f : fy0) - s.v;
          const v2f q = eval_q2(dx2, dy, s.A, s.B, s.C);
          const bool hit0 = px.T2[h].x >= rp.T_eps && q.x <= s.qlim;
          const bool hit1 = px.T2[h].y >= rp.T_eps && q.y <= s.qlim;
          if (__ballot(hit0 || hit1) != 0ull) {
            const v2f G = eval_G2(q);
            const v2f a_raw = G * s.op;
            v2f alpha = clamp_alpha2(a_raw, rp.clamp_max_alpha);
            alpha = (v2f){hit0 ? alpha.x : 0.f, hit1 ? alpha.y : 0.f};
            const v2f w = alpha * px.T2[h];
#pragma unroll
            for (int c = 0; c < CW; ++c) px.col2[h][c] = __builtin_elementwise_fma(w, GSR_V2(fr.f[c]), px.col2[h][c]);
            wsum2 += w;
            px.T2[h] = px.T2[h] - w;
            if (hit0) px.lastc[2 * h] = idx;
            if (hit1) px.lastc[2 * h + 1] = idx;
            if (MEDIAN) {
              if (hit0 && px.med2[h].x == 0.f && px.T2[h].x < 0.5f) px.med2[h].x = s.depth;
              if (hit1 && px.med2[h].y == 0.f && px.T2[h].y < 0.5f) px.med2[h].y = s.depth;
            }
          }
        }
        wq[m] = wsum2.x + wsum2.y;
        fr = load_feat<CW>(feat, pk);                                  // the next pair's features (see above)
      }
    }
    if (VIS) {
      float r = gsr_swap16_add(gsr_swap32_add(wq[0], wq[1]), gsr_swap32_add(wq[2], wq[3]));
      r = gsr_row_sum_to_lane15(r);
      const uint32_t pos = i + vis_slot;
      if ((lane & 15) == 15 && pos < end) {
        pair_vis[pos] = r;
        if (r > 0.f) vis_partial[sorted_inst[pos]] = r;
      }
    }
    const bool live = px.T2[0].x >= rp.T_eps || px.T2[0].y >= rp.T_eps || px.T2[1].x >= rp.T_eps ||
                      px.T2[1].y >= rp.T_eps;
    if (__ballot(live) == 0ull) break;
  }
}

template <int CW, bool MEDIAN>
__device__ __forceinline__ void wide_write_image(const WidePix<CW>& px, int px0, int py0, int W, int H, int C,
                                                 float* __restrict__ image, float* __restrict__ final_T,
                                                 int* __restrict__ last, float* __restrict__ median) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int x = px0 + 8 * (p & 1), y = py0 + 8 * (p >> 1);
    if (x < W && y < H) {
      const size_t pix = (size_t)y * W + x;
      const int h = p >> 1;
#pragma unroll
      for (int c = 0; c < CW; ++c)
        if (c < C) image[pix * C + c] = (p & 1) ? px.col2[h][c].y : px.col2[h][c].x;
      final_T[pix] = (p & 1) ? px.T2[h].y : px.T2[h].x;
      last[pix] = px.lastc[p];
      if (MEDIAN) median[pix] = (p & 1) ? px.med2[h].y : px.med2[h].x;
    }
  }
}

// The CW colours of the lane's four pixels into the segment's slots (layout: file header)
template <int CW>
__device__ __forceinline__ void wide_store_colours(const WidePix<CW>& px, float4* __restrict__ seg_col, uint32_t sidx,
                                                   int lane) {
  float4* out = seg_col + (size_t)sidx * (CW / 4) * 256 + lane;
#pragma unroll
  for (int q = 0; q < CW / 4; ++q) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int h = p >> 1;
      out[256 * q + 64 * p] = (p & 1) ? make_float4(px.col2[h][4 * q].y, px.col2[h][4 * q + 1].y, px.col2[h][4 * q + 2].y,
                                                    px.col2[h][4 * q + 3].y)
                                      : make_float4(px.col2[h][4 * q].x, px.col2[h][4 * q + 1].x, px.col2[h][4 * q + 2].x,
                                                    px.col2[h][4 * q + 3].x);
    }
  }
}

// K6 wide of a frame without a segment plan: one wave walks the tile's whole list.
template <int CW, bool VIS, bool MEDIAN>
__global__ __launch_bounds__(64) void composite_fwd_wide(const float* __restrict__ rec, const float* __restrict__ feat,
                                                         const uint32_t* __restrict__ sorted_rank,
                                                         const uint32_t* __restrict__ sorted_inst,
                                                         const uint32_t* __restrict__ tile_range, int W, int H, int C,
                                                         int tiles_x, int num_tiles, GsrRasterParams rp,
                                                         float* __restrict__ image, float* __restrict__ final_T,
                                                         int* __restrict__ last, float* __restrict__ median,
                                                         float* __restrict__ vis_partial, float* __restrict__ pair_vis) {
  if ((int)blockIdx.x >= num_tiles) return;
  const int lane = (int)threadIdx.x;
  const int tile = gsr_xcd_remap((int)blockIdx.x, num_tiles);
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int px0 = tx * 16 + (lane & 7), py0 = ty * 16 + (lane >> 3);
  const float fx0 = (float)px0 + 0.5f, fy0 = (float)py0 + 0.5f;
  const uint32_t start = tile_range[2 * tile], end = tile_range[2 * tile + 1];
  WidePix<CW> px;
  wide_init<CW>(px, px0, py0, W, H);
  wide_walk<CW, VIS, MEDIAN>(px, rec, feat, sorted_rank, sorted_inst, start, start, end, fx0, fy0, rp, lane, vis_partial,
                             pair_vis);
  wide_write_image<CW, MEDIAN>(px, px0, py0, W, H, C, image, final_T, last, median);
}

// K6 wide of a frame with a segment plan: every tile that is not heavy (short: the walk above; long: the same walk,
// pausing at the segment ends to leave the checkpoints the backward pass enters from), and -- extra blocks -- pass A of
// the heavy tiles' segments.
template <int CW, bool VIS, bool MEDIAN>
__global__ __launch_bounds__(64) void wide_ckpt_fwd(const float* __restrict__ rec, const float* __restrict__ feat,
                                                    const uint32_t* __restrict__ sorted_rank,
                                                    const uint32_t* __restrict__ sorted_inst,
                                                    const uint32_t* __restrict__ tile_range, int W, int H, int C,
                                                    int tiles_x, int num_tiles, GsrRasterParams rp,
                                                    float* __restrict__ image, float* __restrict__ final_T,
                                                    int* __restrict__ last, float* __restrict__ median,
                                                    float* __restrict__ vis_partial, float* __restrict__ pair_vis,
                                                    SegDev seg, float4* __restrict__ seg_col) {
  if ((int)blockIdx.x >= num_tiles) {                                 // extra blocks: pass A (see composite_fwd_kernel)
    const uint32_t h = blockIdx.x - (uint32_t)num_tiles;
    if (h < seg.seg_total[1]) {
      const uint32_t sidx = (seg.tile_seg + 2 * (size_t)num_tiles)[h];
      if (sidx != 0xFFFFFFFFu) {
        const uint32_t* d = seg.seg_desc + 4 * (size_t)sidx;
        if (d[1] < d[2]) seg_alpha_pass<1>(sidx, rec, sorted_rank, tiles_x, rp, seg);
      }
    }
    return;
  }
  const int lane = (int)threadIdx.x;
  const int tile = gsr_xcd_remap((int)blockIdx.x, num_tiles);
  const uint32_t tseg = seg.tile_seg[2 * tile + 1];
  if (tseg & GSR_SEG_HEAVY) return;                                   // heavy tile: passes A, C, D composite it
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int px0 = tx * 16 + (lane & 7), py0 = ty * 16 + (lane >> 3);
  const float fx0 = (float)px0 + 0.5f, fy0 = (float)py0 + 0.5f;
  const uint32_t start = tile_range[2 * tile], end = tile_range[2 * tile + 1];
  WidePix<CW> px;
  wide_init<CW>(px, px0, py0, W, H);
  if (tseg == 0u) {
    wide_walk<CW, VIS, MEDIAN>(px, rec, feat, sorted_rank, sorted_inst, start, start, end, fx0, fy0, rp, lane,
                               vis_partial, pair_vis);
  } else {
    const uint32_t first = seg.tile_seg[2 * tile];
    float* seg_T = reinterpret_cast<float*>(seg.seg_TC);
    for (uint32_t j = 0; j < tseg; ++j) {
      const uint32_t* d = seg.seg_desc + 4 * (size_t)(first + j);
      wide_walk<CW, VIS, MEDIAN>(px, rec, feat, sorted_rank, sorted_inst, start, d[1], d[2], fx0, fy0, rp, lane,
                                 vis_partial, pair_vis);
      float* t = seg_T + 256 * (size_t)(first + j) + lane;
      t[0] = px.T2[0].x; t[64] = px.T2[0].y; t[128] = px.T2[1].x; t[192] = px.T2[1].y;
      wide_store_colours<CW>(px, seg_col, first + j, lane);
      const bool live = px.T2[0].x >= rp.T_eps || px.T2[0].y >= rp.T_eps || px.T2[1].x >= rp.T_eps ||
                        px.T2[1].y >= rp.T_eps;
      if (__ballot(live) == 0ull) break;            // every pixel saturated: later segments contribute to nothing
    }
  }
  wide_write_image<CW, MEDIAN>(px, px0, py0, W, H, C, image, final_T, last, median);
}

// Pass C wide: the forward walk over one segment of a heavy tile, entered with T_in = product of the preceding segments'
// products (taken in segment order); the segment's own T (-1: the pixel was dead at entry), colours, last and median go
// to its slots.
template <int CW, bool VIS, bool MEDIAN>
__global__ __launch_bounds__(64) void wide_seg_fwd(const float* __restrict__ rec, const float* __restrict__ feat,
                                                   const uint32_t* __restrict__ sorted_rank,
                                                   const uint32_t* __restrict__ sorted_inst,
                                                   const uint32_t* __restrict__ tile_range, int W, int H, int tiles_x,
                                                   int num_tiles, GsrRasterParams rp, float* __restrict__ vis_partial,
                                                   float* __restrict__ pair_vis, SegDev seg,
                                                   float4* __restrict__ seg_col) {
  if (blockIdx.x >= seg.seg_total[1]) return;                         // one block per segment of a HEAVY tile
  const uint32_t sidx = (seg.tile_seg + 2 * (size_t)num_tiles)[blockIdx.x];
  if (sidx == 0xFFFFFFFFu) return;
  const uint32_t* d = seg.seg_desc + 4 * (size_t)sidx;
  const int tile = (int)d[0];
  const uint32_t begin = d[1], end = d[2];
  const uint32_t first = seg.tile_seg[2 * tile];
  const int lane = (int)threadIdx.x;
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int px0 = tx * 16 + (lane & 7), py0 = ty * 16 + (lane >> 3);
  const float fx0 = (float)px0 + 0.5f, fy0 = (float)py0 + 0.5f;

  WidePix<CW> px;
  wide_init<CW>(px, px0, py0, W, H);
  for (uint32_t s = first; s < sidx; ++s) {
    const float* P = seg.seg_P + 256 * (size_t)s + lane;
    px.T2[0] = px.T2[0] * (v2f){P[0], P[64]};
    px.T2[1] = px.T2[1] * (v2f){P[128], P[192]};
  }
  const bool alive[4] = {px.T2[0].x >= rp.T_eps, px.T2[0].y >= rp.T_eps, px.T2[1].x >= rp.T_eps, px.T2[1].y >= rp.T_eps};
  if (__ballot(alive[0] || alive[1] || alive[2] || alive[3]) != 0ull)
    wide_walk<CW, VIS, MEDIAN>(px, rec, feat, sorted_rank, sorted_inst, tile_range[2 * tile], begin, end, fx0, fy0, rp,
                               lane, vis_partial, pair_vis);
  const size_t o = 256 * (size_t)sidx + lane;
  float* seg_T = reinterpret_cast<float*>(seg.seg_TC);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int h = p >> 1;
    const float t = (p & 1) ? px.T2[h].y : px.T2[h].x;
    seg_T[o + 64 * p] = alive[p] ? t : -1.f;
    seg.seg_last[o + 64 * p] = px.lastc[p];
    if (MEDIAN) seg.seg_median[o + 64 * p] = (p & 1) ? px.med2[h].y : px.med2[h].x;
  }
  wide_store_colours<CW>(px, seg_col, sidx, lane);
}

// Pass D wide: one wave per heavy tile takes T / last / median from the segments that saw the pixel alive
// (seg_combine_kernel's rules), then -- four channels at a time, so that the wave stays at 16 colour registers whatever
// the width -- adds the segment colours in list order, writes the image and leaves in each segment's slots the colour
// composited up to that segment's end.
template <int CW, bool MEDIAN>
__global__ __launch_bounds__(64) void wide_seg_combine(int W, int H, int C, int tiles_x, float* __restrict__ image,
                                                       float* __restrict__ final_T, int* __restrict__ last,
                                                       float* __restrict__ median, SegDev seg,
                                                       float4* __restrict__ seg_col) {
  const int tile = (int)blockIdx.x;
  const uint32_t tseg = seg.tile_seg[2 * tile + 1];
  if (!(tseg & GSR_SEG_HEAVY)) return;
  const uint32_t n = tseg & ~GSR_SEG_HEAVY;
  const uint32_t first = seg.tile_seg[2 * tile];
  const int lane = (int)threadIdx.x;
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int px0 = tx * 16 + (lane & 7), py0 = ty * 16 + (lane >> 3);
  const float* seg_T = reinterpret_cast<const float*>(seg.seg_TC);
  float T[4], med[4];
  int lastc[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) { T[p] = 1.f; med[p] = 0.f; lastc[p] = 0; }
  for (uint32_t j = 0; j < n; ++j) {
    const size_t o = 256 * (size_t)(first + j) + lane;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float t = seg_T[o + 64 * p];
      if (t >= 0.f) T[p] = t;
      const int l = seg.seg_last[o + 64 * p];
      if (l != 0) lastc[p] = l;
      if (MEDIAN) {
        const float m = seg.seg_median[o + 64 * p];
        if (med[p] == 0.f && m != 0.f) med[p] = m;
      }
    }
  }
  size_t pix[4];
  bool inside[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int x = px0 + 8 * (p & 1), y = py0 + 8 * (p >> 1);
    inside[p] = x < W && y < H;
    pix[p] = (size_t)y * W + x;
    if (inside[p]) {
      final_T[pix[p]] = T[p];
      last[pix[p]] = lastc[p];
      if (MEDIAN) median[pix[p]] = med[p];
    }
  }
#pragma unroll 1
  for (int q = 0; q < CW / 4; ++q) {
    float4 col[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) col[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t j = 0; j < n; ++j) {
      float4* slot = seg_col + ((size_t)(first + j) * (CW / 4) + q) * 256 + lane;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const float4 v = slot[64 * p];
        col[p].x += v.x; col[p].y += v.y; col[p].z += v.z; col[p].w += v.w;
        slot[64 * p] = col[p];
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (!inside[p]) continue;
      float* out = image + pix[p] * C + 4 * q;
      if (4 * q < C) out[0] = col[p].x;
      if (4 * q + 1 < C) out[1] = col[p].y;
      if (4 * q + 2 < C) out[2] = col[p].z;
      if (4 * q + 3 < C) out[3] = col[p].w;
    }
  }
}

// quad sum with two DPP row steps (K7's reduction tail)
__device__ __forceinline__ float quad_sum_dpp(float tot) {
  asm volatile("s_nop 1\n"
               "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n"
               "s_nop 1\n"
               "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
               : "+v"(tot));
  return tot;
}

#define GSR_WIDE_ROW 68      // LDS words per parked value (64 lanes + 4: conflict-free 16-byte reads, as K7)

// K7 wide: composite_bwd_kernel's reverse walk, colour term through gc = g . f.  A block walks tile-relative list
// positions [lo, hi) in reverse: a whole tile's list, or -- the first seg_blocks blocks of the launch, dealt so that a
// tile's segments share an XCD -- one segment of a longer tile, entered with T from the segment's checkpoint and
// ga = sum_c g_c (image_c - colour up to the segment's end), formed with fmaf over c ascending.
// Registers (hipcc, gfx950): 96 / 134 / 206 VGPRs at CW = 4 / 8 / 16, i.e. 5 / 3 / 2 waves per SIMD; no occupancy is
// forced: capping CW = 4 at 5 waves, 8 at 4 or 16 at 3 spills to scratch (tests/test_isa_budget_wide.py pins the budget).
template <int CW>
__global__ __launch_bounds__(64)
void composite_bwd_wide(const float* __restrict__ rec, const float* __restrict__ feat,
                        const uint32_t* __restrict__ sorted_rank, const uint32_t* __restrict__ sorted_inst,
                        const float* __restrict__ pair_vis, const uint32_t* __restrict__ tile_range, int W, int H, int C,
                        int tiles_x, int num_tiles, GsrRasterParams rp, const float* __restrict__ final_T,
                        const int* __restrict__ last, const float* __restrict__ dL_dimage, float* __restrict__ partial,
                        const float* __restrict__ image, SegDev seg, const float4* __restrict__ seg_col,
                        uint32_t seg_capacity, uint32_t seg_blocks) {
  constexpr int NV = 8 + CW;                  // values per pair: 8 geometry / heuristic sums + CW feature sums
  int tile, lo = 0, seg_hi = 0x7fffffff;
  uint32_t sidx = 0u;
  const bool is_seg = blockIdx.x < seg_blocks;
  if (is_seg) {
    sidx = gsr_xcd_group_remap(blockIdx.x, GSR_K7_SEG_GROUP_LOG2);
    if (sidx >= min(seg.seg_total[0], seg_capacity)) return;     // (the grid is rounded up past the tables' capacity)
    const uint32_t* d = seg.seg_desc + 4 * (size_t)sidx;
    tile = (int)d[0];
    const uint32_t tstart = tile_range[2 * tile];
    lo = (int)(d[1] - tstart);
    seg_hi = (int)(d[2] - tstart);
  } else {
    const int b = (int)(blockIdx.x - seg_blocks);                // (seg_blocks is a multiple of 8: same XCD)
    if (b >= num_tiles) return;
    tile = gsr_xcd_remap(b, num_tiles);
    if (seg.tile_seg && seg.tile_seg[2 * tile + 1] != 0u) return;     // segmented tile: its segment blocks handle it
  }
  const int lane = (int)threadIdx.x;
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int px0 = tx * 16 + (lane & 7), py0 = ty * 16 + (lane >> 3);
  const float fx0 = (float)px0 + 0.5f, fy0 = (float)py0 + 0.5f;
  const uint32_t start = tile_range[2 * tile];

  // per pixel (packed over the two sides of a half): T behind the current splat, g = dL/dC, ga = g . (colour behind)
  v2f T2[2], g2[2][CW], ga2[2];
  int lastc[4];
  int tile_last = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    T2[h] = GSR_V2(1.f); ga2[h] = GSR_V2(0.f);
#pragma unroll
    for (int c = 0; c < CW; ++c) g2[h][c] = GSR_V2(0.f);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int px = px0 + 8 * (p & 1), py = py0 + 8 * (p >> 1);
    const int h = p >> 1;
    lastc[p] = 0;
    if (px < W && py < H) {
      const size_t pix = (size_t)py * W + px;
      float t = final_T[pix];
      if (is_seg) {                                   // T after this segment (dead-at-entry pixels never contribute)
        t = reinterpret_cast<const float*>(seg.seg_TC)[256 * (size_t)sidx + 64 * p + lane];
        t = t < 0.f ? 1.f : t;
      }
      if (p & 1) T2[h].y = t; else T2[h].x = t;
      lastc[p] = last[pix];
      float gb = 0.f;
#pragma unroll
      for (int q = 0; q < CW / 4; ++q) {
        float4 up4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (is_seg) up4 = seg_col[((size_t)sidx * (CW / 4) + q) * 256 + 64 * p + lane];
        const float upto[4] = {up4.x, up4.y, up4.z, up4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = 4 * q + k;
          const float gv = c < C ? dL_dimage[pix * C + c] : 0.f;
          if (p & 1) g2[h][c].y = gv; else g2[h][c].x = gv;
          // colour behind the segment = final colour - colour composited up to the segment's end
          if (is_seg && c < C) gb = fmaf(gv, image[pix * C + c] - upto[k], gb);
        }
      }
      if (p & 1) ga2[h].y = gb; else ga2[h].x = gb;   // g . (colour behind the segment); 0 for a whole tile
    }
    tile_last = max(tile_last, lastc[p]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tile_last = max(tile_last, __shfl_xor(tile_last, o, 64));
  tile_last = __builtin_amdgcn_readfirstlane(tile_last);
  const int hi = min(tile_last, seg_hi);
  if (hi <= lo) return;
  __shared__ float red[NV * GSR_WIDE_ROW];

  for (int cbase = lo + (((hi - lo - 1) >> 6) << 6); cbase >= lo; cbase -= 64) {
    const int n = min(64, hi - cbase);
    const uint32_t li = start + (uint32_t)cbase + (uint32_t)lane;
    const float pv = (lane < n) ? pair_vis[li] : 0.f;
    const int my_rank = (lane < n) ? (int)sorted_rank[li] : 0;
    const int my_inst = (lane < n) ? (int)sorted_inst[li] : 0;
    uint64_t flags = __ballot(pv > 0.f);
    if (flags == 0ull) continue;
    int j = 63 - __builtin_clzll(flags);
    uint32_t pk_nxt = (uint32_t)__builtin_amdgcn_readlane(my_rank, j);
    Splat nxt = load_splat_packed<1, true>(rec, pk_nxt);
    uint32_t inst_nxt = (uint32_t)__builtin_amdgcn_readlane(my_inst, j);
    FeatRow<CW> fr = load_feat<CW>(feat, pk_nxt);
    while (true) {
      const Splat s = nxt;
      const uint32_t inst_j = inst_nxt;
      const int pos = cbase + j;
      flags &= ~(1ull << j);
      const bool more = flags != 0ull;
      if (more) {                                             // prefetch the next contributing pair's geometry row
        j = 63 - __builtin_clzll(flags);
        pk_nxt = (uint32_t)__builtin_amdgcn_readlane(my_rank, j);
        nxt = load_splat_packed<1, true>(rec, pk_nxt);
        inst_nxt = (uint32_t)__builtin_amdgcn_readlane(my_inst, j);
      }
      const v2f dx2 = (v2f){fx0, fx0 + 8.f} - GSR_V2(s.u);
      v2f mx2 = GSR_V2(0.f), my2 = mx2, mxx2 = mx2, mxy2 = mx2, myy2 = mx2, dop2 = mx2, prune2 = mx2, split2 = mx2;
      // feature sums folded over the two sides at once (one VGPR per channel instead of a packed pair: the budget)
      float df[CW];
#pragma unroll
      for (int c = 0; c < CW; ++c) df[c] = 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (!(s.halves & (1u << h))) continue;
        const float dy = (h ? fy0 + 8.f : fy0) - s.v;
        v2f q, tx_, ty_;
        eval_qt(dx2, dy, s.A, s.B, s.C, q, tx_, ty_);
        const bool hit0 = pos < lastc[2 * h] && q.x <= s.qlim;
        const bool hit1 = pos < lastc[2 * h + 1] && q.y <= s.qlim;
        if (__ballot(hit0 || hit1) != 0ull) {
          const v2f a_raw = eval_alpha2(q, s.l2op);
          v2f alpha = clamp_alpha2(a_raw, rp.clamp_max_alpha);
          alpha = (v2f){hit0 ? alpha.x : 0.f, hit1 ? alpha.y : 0.f};
          const v2f om = GSR_V2(1.f) - alpha;
          const v2f inv = {__builtin_amdgcn_rcpf(om.x), __builtin_amdgcn_rcpf(om.y)};
          const v2f Tb = T2[h] * inv;
          T2[h] = Tb;
          const v2f w = alpha * Tb;
          v2f gc = g2[h][0] * fr.f[0];
#pragma unroll
          for (int c = 1; c < CW; ++c) gc = __builtin_elementwise_fma(g2[h][c], GSR_V2(fr.f[c]), gc);
#pragma unroll
          for (int c = 0; c < CW; ++c) df[c] = __builtin_fmaf(w.y, g2[h][c].y, __builtin_fmaf(w.x, g2[h][c].x, df[c]));
          const v2f dLda = Tb * gc - ga2[h] * inv;
          ga2[h] = __builtin_elementwise_fma(gc, w, ga2[h]);
          prune2 = (v2f){__builtin_fmaf(__builtin_fabsf(dLda.x), alpha.x, prune2.x),
                         __builtin_fmaf(__builtin_fabsf(dLda.y), alpha.y, prune2.y)};
          const bool m0 = hit0 && a_raw.x <= rp.clamp_max_alpha;
          const bool m1 = hit1 && a_raw.y <= rp.clamp_max_alpha;
          v2f GdG = a_raw * dLda;
          GdG = (v2f){m0 ? GdG.x : 0.f, m1 ? GdG.y : 0.f};
          dop2 += GdG;
          const v2f px_ = GdG * dx2, py_ = GdG * dy;
          mx2 += px_;
          my2 += py_;
          mxx2 = __builtin_elementwise_fma(px_, dx2, mxx2);
          mxy2 = __builtin_elementwise_fma(px_, GSR_V2(dy), mxy2);
          myy2 = __builtin_elementwise_fma(py_, GSR_V2(dy), myy2);
          const v2f nn = __builtin_elementwise_fma(ty_, ty_, tx_ * tx_);
          split2 = (v2f){__builtin_fmaf(__builtin_fabsf(GdG.x), __builtin_amdgcn_sqrtf(nn.x), split2.x),
                         __builtin_fmaf(__builtin_fabsf(GdG.y), __builtin_amdgcn_sqrtf(nn.y), split2.y)};
        }
      }
      if (more) fr = load_feat<CW>(feat, pk_nxt);            // the next pair's features, once these are consumed
      // park the NV per-lane sums value-major (one 68-word row per value), then lane 4k+p adds quarter p of value
      // 16 r + k (read round r) and two quad DPP steps finish it: the fixed association of composite_bwd_kernel
      {
        float* wr = red + lane;
        wr[0 * GSR_WIDE_ROW] = mx2.x + mx2.y; wr[1 * GSR_WIDE_ROW] = my2.x + my2.y;
        wr[2 * GSR_WIDE_ROW] = mxx2.x + mxx2.y; wr[3 * GSR_WIDE_ROW] = mxy2.x + mxy2.y;
        wr[4 * GSR_WIDE_ROW] = myy2.x + myy2.y; wr[5 * GSR_WIDE_ROW] = dop2.x + dop2.y;
        wr[6 * GSR_WIDE_ROW] = prune2.x + prune2.y; wr[7 * GSR_WIDE_ROW] = split2.x + split2.y;
#pragma unroll
        for (int c = 0; c < CW; ++c) wr[(8 + c) * GSR_WIDE_ROW] = df[c];
        gsr_wave_lds_fence();
        float tot[(NV + 15) / 16];
#pragma unroll
        for (int r = 0; r < (NV + 15) / 16; ++r) {
          const int k = 16 * r + (lane >> 2);
          const float4* rd = reinterpret_cast<const float4*>(red + (k < NV ? k : 0) * GSR_WIDE_ROW + (lane & 3) * 16);
          const float4 a = rd[0], b = rd[1], c = rd[2], d = rd[3];
          const v2f t = (((v2f){a.x, a.y} + (v2f){a.z, a.w}) + ((v2f){b.x, b.y} + (v2f){b.z, b.w})) +
                        (((v2f){c.x, c.y} + (v2f){c.z, c.w}) + ((v2f){d.x, d.y} + (v2f){d.z, d.w}));
          tot[r] = t.x + t.y;
        }
        gsr_wave_lds_fence();                                  // reads done before the next pair parks into the same cells
#pragma unroll
        for (int r = 0; r < (NV + 15) / 16; ++r) {
          const float v = quad_sum_dpp(tot[r]);
          const int k = 16 * r + (lane >> 2);
          if ((lane & 3) == 0 && k < NV) partial[(size_t)NV * inst_j + k] = v;
        }
      }
      if (!more) break;
    }
  }
}

}  // namespace

extern "C" {

int gsr_composite_forward_wide_seg(const float* rows, const float* feat_rows, const uint32_t* sorted_splat,
                                   const uint32_t* sorted_inst, const uint32_t* tile_range, int32_t W, int32_t H,
                                   int32_t C, const GsrRasterParamsC* params_host, float* image_out, float* final_T_out,
                                   int32_t* last_out, float* median_depth_out, float* vis_partial_out,
                                   float* pair_vis_out, const GsrSegmentsC* segments_host, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!params_host || W <= 0 || H <= 0) return GSR_ERR_INVALID_ARGUMENT;
  if (params_host->tile_size != 16 || C < GSR_WIDE_MIN_FEATURES || C > GSR_MAX_FEATURES) return GSR_ERR_UNSUPPORTED;
  if (!tile_range || !image_out || !final_T_out || !last_out) return GSR_ERR_INVALID_ARGUMENT;
  const bool vis = vis_partial_out != nullptr, med = median_depth_out != nullptr;
  if (vis && !pair_vis_out) return GSR_ERR_INVALID_ARGUMENT;
  if (!seg_ok(segments_host, med) || (segments_host && !segments_host->seg_col)) return GSR_ERR_INVALID_ARGUMENT;
  const GsrTiles tiles = gsr_tiles(W, H);
  const int tx = tiles.tx, nt = (int)tiles.n;
  const GsrRasterParams rp = to_params(params_host);
  const SegDev seg = to_segdev(segments_host);
  float4* seg_col = segments_host ? reinterpret_cast<float4*>(segments_host->seg_col) : nullptr;
  const int cap = segments_host ? (int)segments_host->heavy_capacity : 0;   // blocks of the heavy-tile passes
  gsr_pick_wide(C, [&](auto cw) {
    gsr_pick_bool(vis, [&](auto v) {
      gsr_pick_bool(med, [&](auto m) {
        constexpr int CW = decltype(cw)::value;
        constexpr bool VV = decltype(v)::value, MM = decltype(m)::value;
        if (!segments_host) {
          composite_fwd_wide<CW, VV, MM><<<nt, 64, 0, stream>>>(rows, feat_rows, sorted_splat, sorted_inst, tile_range, W, H,
                                                                C, tx, nt, rp, image_out, final_T_out, last_out,
                                                                median_depth_out, vis_partial_out, pair_vis_out);
          return;
        }
        wide_ckpt_fwd<CW, VV, MM><<<nt + cap, 64, 0, stream>>>(rows, feat_rows, sorted_splat, sorted_inst, tile_range, W, H,
                                                               C, tx, nt, rp, image_out, final_T_out, last_out,
                                                               median_depth_out, vis_partial_out, pair_vis_out, seg,
                                                               seg_col);
        if (cap) {
          wide_seg_fwd<CW, VV, MM><<<cap, 64, 0, stream>>>(rows, feat_rows, sorted_splat, sorted_inst, tile_range, W, H, tx,
                                                           nt, rp, vis_partial_out, pair_vis_out, seg, seg_col);
          wide_seg_combine<CW, MM><<<nt, 64, 0, stream>>>(W, H, C, tx, image_out, final_T_out, last_out, median_depth_out,
                                                          seg, seg_col);
        }
      });
    });
  });
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_composite_forward_wide(const float* rows, const float* feat_rows, const uint32_t* sorted_splat,
                               const uint32_t* sorted_inst, const uint32_t* tile_range, int32_t W, int32_t H, int32_t C,
                               const GsrRasterParamsC* params_host, float* image_out, float* final_T_out,
                               int32_t* last_out, float* median_depth_out, float* vis_partial_out, float* pair_vis_out,
                               void* stream_) {
  return gsr_composite_forward_wide_seg(rows, feat_rows, sorted_splat, sorted_inst, tile_range, W, H, C, params_host,
                                        image_out, final_T_out, last_out, median_depth_out, vis_partial_out,
                                        pair_vis_out, nullptr, stream_);
}

int gsr_composite_backward_wide_seg(const float* rows, const float* feat_rows, const uint32_t* sorted_splat,
                                    const uint32_t* sorted_inst, const float* pair_vis, const uint32_t* tile_range,
                                    int32_t W, int32_t H, int32_t C, const GsrRasterParamsC* params_host,
                                    const float* final_T, const int32_t* last, const float* dL_dimage, const float* image,
                                    float* partial_out, const GsrSegmentsC* segments_host, void* stream_) {
  hipStream_t stream = gsr_stream(stream_);
  if (!params_host || W <= 0 || H <= 0) return GSR_ERR_INVALID_ARGUMENT;
  if (params_host->tile_size != 16 || C < GSR_WIDE_MIN_FEATURES || C > GSR_MAX_FEATURES) return GSR_ERR_UNSUPPORTED;
  if (!tile_range || !final_T || !last || !dL_dimage || !pair_vis) return GSR_ERR_INVALID_ARGUMENT;
  if (!seg_ok(segments_host, false) || (segments_host && (!image || !segments_host->seg_col)))
    return GSR_ERR_INVALID_ARGUMENT;
  const GsrTiles tiles = gsr_tiles(W, H);
  const int tx = tiles.tx, nt = (int)tiles.n;
  const GsrRasterParams rp = to_params(params_host);
  const SegDev seg = to_segdev(segments_host);
  const float4* seg_col = segments_host ? reinterpret_cast<const float4*>(segments_host->seg_col) : nullptr;
  // segment blocks: rounded up to the XCD grouping of gsr_xcd_group_remap (blocks past seg_total return)
  const int seg_round = 8 << GSR_K7_SEG_GROUP_LOG2;
  const uint32_t seg_blocks =
      segments_host ? (uint32_t)((segments_host->capacity + seg_round - 1) / seg_round * seg_round) : 0u;
  const uint32_t seg_cap = (uint32_t)(segments_host ? segments_host->capacity : 0);
  const int grid = nt + (int)seg_blocks;
  gsr_pick_wide(C, [&](auto cw) {
    composite_bwd_wide<decltype(cw)::value><<<grid, 64, 0, stream>>>(rows, feat_rows, sorted_splat, sorted_inst, pair_vis,
                                                                    tile_range, W, H, C, tx, nt, rp, final_T, last,
                                                                    dL_dimage, partial_out, image, seg, seg_col, seg_cap,
                                                                    seg_blocks);
  });
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_composite_backward_wide(const float* rows, const float* feat_rows, const uint32_t* sorted_splat,
                                const uint32_t* sorted_inst, const float* pair_vis, const uint32_t* tile_range,
                                int32_t W, int32_t H, int32_t C, const GsrRasterParamsC* params_host,
                                const float* final_T, const int32_t* last, const float* dL_dimage, float* partial_out,
                                void* stream_) {
  return gsr_composite_backward_wide_seg(rows, feat_rows, sorted_splat, sorted_inst, pair_vis, tile_range, W, H, C,
                                         params_host, final_T, last, dL_dimage, nullptr, partial_out, nullptr, stream_);
}

}  // extern "C"
