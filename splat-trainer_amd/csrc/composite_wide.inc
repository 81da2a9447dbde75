// Wide feature frames (4 <= C <= 16): K6 and K7 for features kept in a second per-splat table.
//
// Included at the end of composite.hip (it reuses that file's walk helpers: eval_q2 / eval_qt / eval_G2 / eval_alpha2 /
// clamp_alpha2, the packed row loads, the visibility fold).  The geometry row is the ordinary 64-byte row with zero
// colour slots; the features live in feat_rows [M, CW] (splat order, CW in {4, 8, 16}, zero-padded past C), fetched by
// splat id through the scalar cache like the row itself.
//
// Wide frames run unsegmented (one wave walks a tile's whole list, RasterConfig(segment_pairs=0) for C <= 3): the
// checkpoints of a segmented frame would have to carry (T, C colours) per pixel.  The forward walk takes the same
// contribute / skip decisions with the same expressions as fwd_walk, so every channel, T, last, median and the visibility
// partials are bit-identical to the unsegmented C <= 3 path for the same splats.
// The backward walk needs the colour only through the scalar gc = dL/dimage(px) . f per (pixel, splat) pair, as K7 does;
// per pixel it keeps T, the suffix g . (colour behind) and the CW floats of dL/dimage.  Each (tile, splat) pair owns one
// slot of 8 + CW floats (mx my mxx mxy myy m0 prune split | df0 .. df(CW-1)): no float atomics, fixed-order reductions.

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

// K6 wide.  Same mapping, walk and expressions as composite_fwd_kernel's unsegmented, row-by-row form (PF = false).
// SGPRs: the geometry row of the NEXT pair is prefetched as there, but a CW = 16 feature row would not fit twice next to
// it (2 x (12 + 16) row words); so the feature row of the next pair is fetched at the END of the current pair, once the
// current one has been consumed, and arrives while the next pair's geometry is evaluated.
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

  v2f T2[2], col2[2][CW], med2[2];
  int lastc[4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const bool in_y = (py0 + 8 * h) < H;
    T2[h] = (v2f){(in_y && px0 < W) ? 1.f : 0.f, (in_y && (px0 + 8) < W) ? 1.f : 0.f};
    med2[h] = GSR_V2(0.f);
#pragma unroll
    for (int c = 0; c < CW; ++c) col2[h][c] = GSR_V2(0.f);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) lastc[p] = 0;

  const uint32_t vis_slot = (uint32_t)(((lane >> 4) & 1) * 2 + (lane >> 5));
  if (start < end) {
    uint32_t pk = rank_at(sorted_rank, start);
    Splat nxt = load_splat_packed<1, MEDIAN>(rec, pk);
    FeatRow<CW> fr = load_feat<CW>(feat, pk);
    for (uint32_t i = start; i < end; i += 4) {
      float wq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (i + m < end) {                                               // wave-uniform
          const Splat s = nxt;
          pk = rank_at(sorted_rank, min(i + m + 1, end - 1u));          // unconditional, as fwd_walk
          nxt = load_splat_packed<1, MEDIAN>(rec, pk);
          const v2f dx2 = (v2f){fx0, fx0 + 8.f} - GSR_V2(s.u);
          const int idx = (int)(i - start) + m + 1;
          v2f wsum2 = GSR_V2(0.f);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (!(s.halves & (1u << h))) continue;
            const float dy = (h ? fy0 + 8.f : fy0) - s.v;
            const v2f q = eval_q2(dx2, dy, s.A, s.B, s.C);
            const bool hit0 = T2[h].x >= rp.T_eps && q.x <= s.qlim;
            const bool hit1 = T2[h].y >= rp.T_eps && q.y <= s.qlim;
            if (__ballot(hit0 || hit1) != 0ull) {
              const v2f G = eval_G2(q);
              const v2f a_raw = G * s.op;
              v2f alpha = clamp_alpha2(a_raw, rp.clamp_max_alpha);
              alpha = (v2f){hit0 ? alpha.x : 0.f, hit1 ? alpha.y : 0.f};
              const v2f w = alpha * T2[h];
#pragma unroll
              for (int c = 0; c < CW; ++c) col2[h][c] = __builtin_elementwise_fma(w, GSR_V2(fr.f[c]), col2[h][c]);
              wsum2 += w;
              T2[h] = T2[h] - w;
              if (hit0) lastc[2 * h] = idx;
              if (hit1) lastc[2 * h + 1] = idx;
              if (MEDIAN) {
                if (hit0 && med2[h].x == 0.f && T2[h].x < 0.5f) med2[h].x = s.depth;
                if (hit1 && med2[h].y == 0.f && T2[h].y < 0.5f) med2[h].y = s.depth;
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
      const bool live = T2[0].x >= rp.T_eps || T2[0].y >= rp.T_eps || T2[1].x >= rp.T_eps || T2[1].y >= rp.T_eps;
      if (__ballot(live) == 0ull) break;
    }
  }

#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int x = px0 + 8 * (p & 1), y = py0 + 8 * (p >> 1);
    if (x < W && y < H) {
      const size_t pix = (size_t)y * W + x;
      const int h = p >> 1;
#pragma unroll
      for (int c = 0; c < CW; ++c)
        if (c < C) image[pix * C + c] = (p & 1) ? col2[h][c].y : col2[h][c].x;
      final_T[pix] = (p & 1) ? T2[h].y : T2[h].x;
      last[pix] = lastc[p];
      if (MEDIAN) median[pix] = (p & 1) ? med2[h].y : med2[h].x;
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

// K7 wide: composite_bwd_kernel's reverse walk over a whole tile (no segments), colour term through gc = g . f.
// Registers (hipcc, gfx950): 96 / 134 / 206 VGPRs at CW = 4 / 8 / 16, i.e. 5 / 3 / 2 waves per SIMD; no occupancy is
// forced: capping CW = 4 at 5 waves, 8 at 4 or 16 at 3 spills to scratch (tests/test_isa_budget_wide.py pins the budget).
template <int CW>
__global__ __launch_bounds__(64)
void composite_bwd_wide(const float* __restrict__ rec, const float* __restrict__ feat,
                        const uint32_t* __restrict__ sorted_rank, const uint32_t* __restrict__ sorted_inst,
                        const float* __restrict__ pair_vis, const uint32_t* __restrict__ tile_range, int W, int H, int C,
                        int tiles_x, int num_tiles, GsrRasterParams rp, const float* __restrict__ final_T,
                        const int* __restrict__ last, const float* __restrict__ dL_dimage, float* __restrict__ partial) {
  constexpr int NV = 8 + CW;                  // values per pair: 8 geometry / heuristic sums + CW feature sums
  if ((int)blockIdx.x >= num_tiles) return;
  const int tile = gsr_xcd_remap((int)blockIdx.x, num_tiles);
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
      const float t = final_T[pix];
      if (p & 1) T2[h].y = t; else T2[h].x = t;
      lastc[p] = last[pix];
#pragma unroll
      for (int c = 0; c < CW; ++c) {
        const float gv = c < C ? dL_dimage[pix * C + c] : 0.f;
        if (p & 1) g2[h][c].y = gv; else g2[h][c].x = gv;
      }
    }
    tile_last = max(tile_last, lastc[p]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tile_last = max(tile_last, __shfl_xor(tile_last, o, 64));
  tile_last = __builtin_amdgcn_readfirstlane(tile_last);
  const int hi = tile_last;
  if (hi <= 0) return;
  __shared__ float red[NV * GSR_WIDE_ROW];

  for (int cbase = ((hi - 1) >> 6) << 6; cbase >= 0; cbase -= 64) {
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

inline int wide_width(int C) { return C <= 4 ? 4 : (C <= 8 ? 8 : 16); }

}  // namespace

extern "C" {

int gsr_composite_forward_wide(const float* rows, const float* feat_rows, const uint32_t* sorted_splat,
                               const uint32_t* sorted_inst, const uint32_t* tile_range, int32_t W, int32_t H, int32_t C,
                               const GsrRasterParamsC* params_host, float* image_out, float* final_T_out,
                               int32_t* last_out, float* median_depth_out, float* vis_partial_out, float* pair_vis_out,
                               void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!params_host || W <= 0 || H <= 0) return GSR_ERR_INVALID_ARGUMENT;
  if (params_host->tile_size != 16 || C < GSR_WIDE_MIN_FEATURES || C > GSR_MAX_FEATURES) return GSR_ERR_UNSUPPORTED;
  if (!tile_range || !image_out || !final_T_out || !last_out) return GSR_ERR_INVALID_ARGUMENT;
  const bool vis = vis_partial_out != nullptr, med = median_depth_out != nullptr;
  if (vis && !pair_vis_out) return GSR_ERR_INVALID_ARGUMENT;
  const int tx = (W + 15) / 16, ty = (H + 15) / 16, nt = tx * ty;
  const GsrRasterParams rp = to_params(params_host);
#define GSR_LAUNCH_FWD_WIDE(CW, VV, MM)                                                                                   \
  composite_fwd_wide<CW, VV, MM><<<nt, 64, 0, stream>>>(rows, feat_rows, sorted_splat, sorted_inst, tile_range, W, H, C, \
                                                        tx, nt, rp, image_out, final_T_out, last_out, median_depth_out,  \
                                                        vis_partial_out, pair_vis_out)
#define GSR_DISPATCH_FWD_WIDE(CW)                                  \
  do {                                                             \
    if (vis && med) GSR_LAUNCH_FWD_WIDE(CW, true, true);           \
    else if (vis) GSR_LAUNCH_FWD_WIDE(CW, true, false);            \
    else if (med) GSR_LAUNCH_FWD_WIDE(CW, false, true);            \
    else GSR_LAUNCH_FWD_WIDE(CW, false, false);                    \
  } while (0)
  const int cw = wide_width(C);
  if (cw == 4) GSR_DISPATCH_FWD_WIDE(4);
  else if (cw == 8) GSR_DISPATCH_FWD_WIDE(8);
  else GSR_DISPATCH_FWD_WIDE(16);
#undef GSR_DISPATCH_FWD_WIDE
#undef GSR_LAUNCH_FWD_WIDE
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_composite_backward_wide(const float* rows, const float* feat_rows, const uint32_t* sorted_splat,
                                const uint32_t* sorted_inst, const float* pair_vis, const uint32_t* tile_range,
                                int32_t W, int32_t H, int32_t C, const GsrRasterParamsC* params_host,
                                const float* final_T, const int32_t* last, const float* dL_dimage, float* partial_out,
                                void* stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!params_host || W <= 0 || H <= 0) return GSR_ERR_INVALID_ARGUMENT;
  if (params_host->tile_size != 16 || C < GSR_WIDE_MIN_FEATURES || C > GSR_MAX_FEATURES) return GSR_ERR_UNSUPPORTED;
  if (!tile_range || !final_T || !last || !dL_dimage || !pair_vis) return GSR_ERR_INVALID_ARGUMENT;
  const int tx = (W + 15) / 16, ty = (H + 15) / 16, nt = tx * ty;
  const GsrRasterParams rp = to_params(params_host);
  const int cw = wide_width(C);
#define GSR_LAUNCH_BWD_WIDE(CW)                                                                                          \
  composite_bwd_wide<CW><<<nt, 64, 0, stream>>>(rows, feat_rows, sorted_splat, sorted_inst, pair_vis, tile_range, W, H, \
                                                C, tx, nt, rp, final_T, last, dL_dimage, partial_out)
  if (cw == 4) GSR_LAUNCH_BWD_WIDE(4);
  else if (cw == 8) GSR_LAUNCH_BWD_WIDE(8);
  else GSR_LAUNCH_BWD_WIDE(16);
#undef GSR_LAUNCH_BWD_WIDE
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
