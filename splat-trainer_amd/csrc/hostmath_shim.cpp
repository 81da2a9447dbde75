// CPU unit-test shim: exposes the per-splat maths of gsr_math.h (the very source the HIP kernels compile)
// to the `-m "not gpu"` tests.  It is NOT a product path: nothing in the package calls it, it renders
// nothing, and the rasterizer fails loudly without libgsplat_hip.so.  Its entry points are declared, with the layout of
// their arrays, in hostmath_shim.h: the build rejects a definition that has no declaration there or disagrees with it.
#include "hostmath_shim.h"

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "gsr_math.h"
#include "gsr_bilagrid.h"
#include "gsr_neighbours.h"
#include "gsr_visibility.h"
#include "gsr_filter3d.h"
#include "gsr_sh_fit.h"
#include "gsr_controller.h"
#include "gsr_camera_table.h"
#include "gsr_color.h"
#include "gsr_eval.h"
#include "gsr_histogram.h"
#include "gsr_image.h"
#include "gsr_undistort.h"
#include "gsr_relocate.h"
#include "gsr_fusion.h"
#include "gsr_mesh.h"

extern "C" {

void hm_project_forward(const float* T, const float* proj, const void* params, int64_t M, const float* pos,
                        const float* ls, const float* rot, const float* logit, float* g2d, float* depth,
                        float* sscale) {
  GsrRasterParams rp;
  memcpy(&rp, params, sizeof(rp));
  GsrCam cam = gsr_load_cam(T, proj);
  for (int64_t m = 0; m < M; ++m) {
    GsrProjected o = gsr_project_one(cam, rp, pos + 3 * m, ls + 3 * m, rot + 4 * m, logit[m]);
    float* g = g2d + 6 * m;
    g[0] = o.u; g[1] = o.v; g[2] = o.A; g[3] = o.B; g[4] = o.C; g[5] = o.opacity;
    depth[m] = o.depth;
    sscale[2 * m] = o.s_major; sscale[2 * m + 1] = o.s_minor;
  }
}

void hm_project_backward(const float* T, const float* proj, const void* params, int64_t M, const float* pos,
                         const float* ls, const float* rot, const float* logit, const float* dg2d,
                         const float* ddepth, float* dpos, float* dls, float* drot, float* dlogit) {
  GsrRasterParams rp;
  memcpy(&rp, params, sizeof(rp));
  GsrCam cam = gsr_load_cam(T, proj);
  for (int64_t m = 0; m < M; ++m) {
    GsrProjectGrad o = gsr_project_one_bwd(cam, rp, pos + 3 * m, ls + 3 * m, rot + 4 * m, logit[m], dg2d + 6 * m,
                                           ddepth[m]);
    for (int k = 0; k < 3; ++k) { dpos[3 * m + k] = o.dp[k]; dls[3 * m + k] = o.dls[k]; }
    for (int k = 0; k < 4; ++k) drot[4 * m + k] = o.dq[k];
    dlogit[m] = o.dlogit;
  }
}

void hm_project_backward_camera(const float* T, const float* proj, const void* params, int64_t M, const float* pos,
                                const float* ls, const float* rot, const float* logit, const float* dg2d,
                                const float* ddepth, float* cam) {
  GsrRasterParams rp;
  memcpy(&rp, params, sizeof(rp));
  GsrCam c = gsr_load_cam(T, proj);
  for (int64_t m = 0; m < M; ++m) {
    float* acc = cam + GSR_CAM_GRAD_FLOATS * m;
    for (int k = 0; k < GSR_CAM_GRAD_FLOATS; ++k) acc[k] = 0.f;
    gsr_project_one_bwd<true>(c, rp, pos + 3 * m, ls + 3 * m, rot + 4 * m, logit[m], dg2d + 6 * m, ddepth[m], acc);
  }
}

void hm_fold_camera_position(const float* T, const float* dcam, float* dT) {
  const float proj[4] = {1.f, 1.f, 0.f, 0.f};
  gsr_fold_camera_position(gsr_load_cam(T, proj), dcam, dT);
}

void hm_in_view(const float* T, const float* proj, int64_t N, const float* pos, int W, int H, float near_p,
                float far_p, float margin, uint8_t* mask) {
  GsrCam cam = gsr_load_cam(T, proj);
  for (int64_t i = 0; i < N; ++i)
    mask[i] = gsr_in_view(cam, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], W, H, near_p, far_p, margin) ? 1 : 0;
}

void hm_sh_basis(int K, int64_t M, const float* dirs, float* Y) {
  for (int64_t m = 0; m < M; ++m) {
    const float* d = dirs + 3 * m;
    float* y = Y + (int64_t)K * m;
    switch (K) {
      case 1: gsr_sh_basis<1>(d[0], d[1], d[2], y); break;
      case 4: gsr_sh_basis<4>(d[0], d[1], d[2], y); break;
      case 9: gsr_sh_basis<9>(d[0], d[1], d[2], y); break;
      default: gsr_sh_basis<16>(d[0], d[1], d[2], y); break;
    }
  }
}

void hm_tile_hits(const void* params, int64_t M, const float* g2d, int tiles_x, int tiles_y, uint8_t* hits) {
  GsrRasterParams rp;
  memcpy(&rp, params, sizeof(rp));
  const int64_t nt = (int64_t)tiles_x * tiles_y;
  for (int64_t m = 0; m < M; ++m) {
    const float* g = g2d + 6 * m;
    GsrExtent e = gsr_splat_extent(g[0], g[1], g[2], g[3], g[4], g[5], rp, tiles_x, tiles_y);
    for (int ty = e.y0; ty < e.y1; ++ty)
      for (int tx = e.x0; tx < e.x1; ++tx)
        if (gsr_tile_hit(g[0], g[1], g[2], g[3], g[4], e.qmax, tx, ty)) hits[m * nt + ty * tiles_x + tx] = 1;
  }
}

void hm_splat_extent(const void* params, int64_t M, const float* g2d, int tiles_x, int tiles_y, int32_t* extent,
                     float* qmax) {
  GsrRasterParams rp;
  memcpy(&rp, params, sizeof(rp));
  for (int64_t m = 0; m < M; ++m) {
    const float* g = g2d + 6 * m;
    GsrExtent e = gsr_splat_extent(g[0], g[1], g[2], g[3], g[4], g[5], rp, tiles_x, tiles_y);
    int32_t* o = extent + 4 * m;
    o[0] = e.x0; o[1] = e.x1; o[2] = e.y0; o[3] = e.y1;
    qmax[m] = e.qmax;
  }
}

// K4's verdict per tile (binning.hip): the half mask alone for an extent of up to 32 tiles (tile_count_one's map), the
// whole-tile test in front of it for a larger one (hits_of_large_extent).
void hm_tile_half_masks(const void* params, int64_t M, const float* g2d, int tiles_x, int tiles_y, uint8_t* masks) {
  GsrRasterParams rp;
  memcpy(&rp, params, sizeof(rp));
  const int64_t nt = (int64_t)tiles_x * tiles_y;
  for (int64_t m = 0; m < M; ++m) {
    const float* g = g2d + 6 * m;
    GsrExtent e = gsr_splat_extent(g[0], g[1], g[2], g[3], g[4], g[5], rp, tiles_x, tiles_y);
    const bool large = (e.x1 - e.x0) * (e.y1 - e.y0) > 32;
    for (int ty = e.y0; ty < e.y1; ++ty)
      for (int tx = e.x0; tx < e.x1; ++tx) {
        if (large && !gsr_tile_hit(g[0], g[1], g[2], g[3], g[4], e.qmax, tx, ty)) continue;
        masks[m * nt + ty * tiles_x + tx] = (uint8_t)gsr_tile_half_mask(g[0], g[1], g[2], g[3], g[4], e.qmax, tx, ty);
      }
  }
}

// bilateral-grid slice of one image (gsr_bilagrid.h) with ONE grid [12, L, GH, GW]: the cell's corner columns are gathered
// per pixel into the cols[4][L][12] layout the kernels stage in LDS.
static void hm_bg_cols(const float* grid, int L, int GH, int GW, int cx, int cy, float* cols) {
  for (int q = 0; q < 4; ++q)
    for (int l = 0; l < L; ++l)
      for (int c = 0; c < GSR_BG_CH; ++c)
        cols[(q * L + l) * GSR_BG_CH + c] = grid[((c * L + l) * GH + cy + (q >> 1)) * GW + cx + (q & 1)];
}

void hm_bilagrid_forward(const float* grid, int L, int GH, int GW, const float* rgb, int H, int W, float* out) {
  float cols[4 * 64 * GSR_BG_CH];
  const float inv_2w = 1.f / (2.f * (float)W), inv_2h = 1.f / (2.f * (float)H);
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < W; ++j) {
      const int cx = gsr_bg_cell(j, W, GW), cy = gsr_bg_cell(i, H, GH);
      hm_bg_cols(grid, L, GH, GW, cx, cy, cols);
      const float* p = rgb + 3 * ((int64_t)i * W + j);
      gsr_bg_pixel_fwd(cols, L, gsr_bg_frac(j, cx, W, GW, inv_2w), gsr_bg_frac(i, cy, H, GH, inv_2h), p[0], p[1], p[2],
                       out + 3 * ((int64_t)i * W + j));
    }
}

void hm_bilagrid_backward(const float* grid, int L, int GH, int GW, const float* rgb, int H, int W, const float* d_out,
                          float* d_rgb, float* d_grid) {
  float cols[4 * 64 * GSR_BG_CH];
  const int n_grid = GSR_BG_CH * L * GH * GW;
  double* acc = new double[n_grid]();
  const float inv_2w = 1.f / (2.f * (float)W), inv_2h = 1.f / (2.f * (float)H);
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < W; ++j) {
      const int cx = gsr_bg_cell(j, W, GW), cy = gsr_bg_cell(i, H, GH);
      hm_bg_cols(grid, L, GH, GW, cx, cy, cols);
      const int64_t o = 3 * ((int64_t)i * W + j);
      const float tx = gsr_bg_frac(j, cx, W, GW, inv_2w), ty = gsr_bg_frac(i, cy, H, GH, inv_2h);
      const float* p = rgb + o;
      gsr_bg_pixel_bwd_rgb(cols, L, tx, ty, p[0], p[1], p[2], d_out + o, d_rgb + o);
      const GsrBgZ z = gsr_bg_z(gsr_bg_luma(p[0], p[1], p[2]), L);
      float wxy[4];
      gsr_bg_xy_weights(tx, ty, wxy);
      for (int k = 0; k < 2; ++k) {
        const float wz = k == 0 ? 1.f - z.tz : z.tz;
        for (int q = 0; q < 4; ++q) {
          const float w = wz * wxy[q];
          for (int m = 0; m < 3; ++m) {
            const float v[4] = {p[0], p[1], p[2], 1.f};
            for (int n = 0; n < 4; ++n)
              acc[(((4 * m + n) * L + z.z0 + k) * GH + cy + (q >> 1)) * GW + cx + (q & 1)] += w * (d_out[o + m] * v[n]);
          }
        }
      }
    }
  for (int e = 0; e < n_grid; ++e) d_grid[e] = (float)acc[e];
  delete[] acc;
}

// ---- colour fit of the evaluation pass (gsr_eval.h) -----------------------------------------------------------------
void hm_color_fit_moments(const float* x0, const float* x, const float* ref, int64_t P, float eps, double* sums) {
  const float lo = eps, hi = (float)(1.0 - (double)eps);
  for (int k = 0; k < 3 * GSR_EV_SUMS; ++k) sums[k] = 0.0;
  for (int64_t p = 0; p < P; ++p) {
    double a[GSR_EV_COLS];
    gsr_ev_row(x[3 * p], x[3 * p + 1], x[3 * p + 2], a);
    for (int c = 0; c < 3; ++c) {
      const int64_t o = 3 * p + c;
      if (gsr_ev_unclipped(x0[o], lo, hi) && gsr_ev_unclipped(x[o], lo, hi) && gsr_ev_unclipped(ref[o], lo, hi))
        gsr_ev_accumulate(a, (double)ref[o], sums + GSR_EV_SUMS * c);
    }
  }
}

void hm_color_fit_solve(const double* sums, double* w) {
  double work[GSR_EV_WORK];
  gsr_ev_solve(sums, work, w);
}

void hm_color_fit(const float* x0, const float* ref, int64_t P, int num_iters, float eps, float* out) {
  const float lo = eps, hi = (float)(1.0 - (double)eps);
  const int64_t want = (P + 255) / 256;
  const int blocks = (int)(want < 1024 ? want : 1024);
  float* cur = new float[3 * P];
  float* nxt = new float[3 * P];
  double* lanes = new double[64 * GSR_EV_SUMS];
  double weights[3 * GSR_EV_COLS];
  for (int k = 0; k <= num_iters; ++k) {
    for (int64_t p = 0; p < P; ++p) {
      const float* src = k ? cur : x0;
      if (k) {
        double a[GSR_EV_COLS];
        gsr_ev_row(src[3 * p], src[3 * p + 1], src[3 * p + 2], a);
        for (int c = 0; c < 3; ++c) nxt[3 * p + c] = gsr_ev_warp(a, weights + GSR_EV_COLS * c);
      } else {
        for (int c = 0; c < 3; ++c) nxt[3 * p + c] = src[3 * p + c];
      }
    }
    float* t = cur; cur = nxt; nxt = t;
    if (k == num_iters) break;
    for (int c = 0; c < 3; ++c) {
      double sums[GSR_EV_SUMS];
      for (int s = 0; s < GSR_EV_SUMS; ++s) sums[s] = 0.0;
      for (int b = 0; b < blocks; ++b) {
        double part[4][GSR_EV_SUMS];
        for (int wv = 0; wv < 4; ++wv) {
          for (int i = 0; i < 64 * GSR_EV_SUMS; ++i) lanes[i] = 0.0;
          for (int lane = 0; lane < 64; ++lane)
            for (int64_t p = (int64_t)b * 256 + wv * 64 + lane; p < P; p += (int64_t)blocks * 256) {
              const int64_t o = 3 * p + c;
              if (!(gsr_ev_unclipped(x0[o], lo, hi) && gsr_ev_unclipped(cur[o], lo, hi) && gsr_ev_unclipped(ref[o], lo, hi)))
                continue;
              double a[GSR_EV_COLS];
              gsr_ev_row(cur[3 * p], cur[3 * p + 1], cur[3 * p + 2], a);
              gsr_ev_accumulate(a, (double)ref[o], lanes + GSR_EV_SUMS * lane);
            }
          for (int off = 32; off > 0; off >>= 1)
            for (int lane = 0; lane < off; ++lane)
              for (int s = 0; s < GSR_EV_SUMS; ++s) lanes[GSR_EV_SUMS * lane + s] += lanes[GSR_EV_SUMS * (lane + off) + s];
          for (int s = 0; s < GSR_EV_SUMS; ++s) part[wv][s] = lanes[s];
        }
        for (int s = 0; s < GSR_EV_SUMS; ++s) sums[s] += ((part[0][s] + part[1][s]) + part[2][s]) + part[3][s];
      }
      double work[GSR_EV_WORK];
      gsr_ev_solve(sums, work, weights + GSR_EV_COLS * c);
    }
  }
  for (int64_t i = 0; i < 3 * P; ++i) out[i] = cur[i];
  delete[] cur;
  delete[] nxt;
  delete[] lanes;
}


// brute-force kNN and nearest-centroid assignment (gsr_neighbours.h): the device's results bit for bit.
}  // extern "C"

template <int K>
static void hm_knn_k(const float* p, int64_t N, int64_t i0, int64_t i1, float* dist2, int64_t* idx, float* scale) {
  for (int64_t i = i0; i < i1; ++i) {
    float d[K];
    int32_t j[K];
    gsr_nb_init(d, j);
    for (int64_t c = 0; c < N; ++c)
      if (c != i) gsr_nb_insert(d, j, gsr_nb_dist2(p[3 * i], p[3 * i + 1], p[3 * i + 2], p[3 * c], p[3 * c + 1], p[3 * c + 2]),
                                (int32_t)c);
    for (int t = 0; t < K; ++t) { dist2[(i - i0) * K + t] = d[t]; idx[(i - i0) * K + t] = j[t]; }
    scale[i - i0] = gsr_nb_mean_dist(d);
  }
}

extern "C" {

int hm_knn(const float* p, int64_t N, int k, int64_t i0, int64_t i1, float* dist2, int64_t* idx, float* scale) {
  if (k < 1 || k > 16 || N <= k || i0 < 0 || i1 > N || i0 > i1) return -1;
  switch (k) {
    case 1: hm_knn_k<1>(p, N, i0, i1, dist2, idx, scale); break;
    case 2: hm_knn_k<2>(p, N, i0, i1, dist2, idx, scale); break;
    case 3: hm_knn_k<3>(p, N, i0, i1, dist2, idx, scale); break;
    case 4: hm_knn_k<4>(p, N, i0, i1, dist2, idx, scale); break;
    case 5: hm_knn_k<5>(p, N, i0, i1, dist2, idx, scale); break;
    case 6: hm_knn_k<6>(p, N, i0, i1, dist2, idx, scale); break;
    case 7: hm_knn_k<7>(p, N, i0, i1, dist2, idx, scale); break;
    case 8: hm_knn_k<8>(p, N, i0, i1, dist2, idx, scale); break;
    case 9: hm_knn_k<9>(p, N, i0, i1, dist2, idx, scale); break;
    case 10: hm_knn_k<10>(p, N, i0, i1, dist2, idx, scale); break;
    case 11: hm_knn_k<11>(p, N, i0, i1, dist2, idx, scale); break;
    case 12: hm_knn_k<12>(p, N, i0, i1, dist2, idx, scale); break;
    case 13: hm_knn_k<13>(p, N, i0, i1, dist2, idx, scale); break;
    case 14: hm_knn_k<14>(p, N, i0, i1, dist2, idx, scale); break;
    case 15: hm_knn_k<15>(p, N, i0, i1, dist2, idx, scale); break;
    default: hm_knn_k<16>(p, N, i0, i1, dist2, idx, scale); break;
  }
  return 0;
}

void hm_assign_clusters(const float* x, int64_t N, const float* c, int64_t K, int64_t* labels) {
  for (int64_t i = 0; i < N; ++i) {
    float best = INFINITY;
    int32_t label = 0;
    for (int64_t j = 0; j < K; ++j)
      gsr_nb_argmin_step(best, label, gsr_nb_dist2(x[3 * i], x[3 * i + 1], x[3 * i + 2], c[3 * j], c[3 * j + 1], c[3 * j + 2]),
                         (int32_t)j);
    labels[i] = label;
  }
}

}  // extern "C"

// colour-model row maths (gsr_color.h), one row at a time: the SH basis and its vector-Jacobian product, LayerNorm,
// GLU, the luminance activation and F.normalize, each with its derivative.
template <int S>
static void hm_cm_rsh_s(const float* d, int64_t n, float* out, const float* dsh, float* dd) {
  const int K = (S + 1) * (S + 1);
  for (int64_t i = 0; i < n; ++i) {
    const float* v = d + 3 * i;
    if (out) gsr_cm_rsh<S>(v[0], v[1], v[2], [&](int c, float y) { out[i * K + c] = y; });
    if (dd) {
      float g[3] = {0.f, 0.f, 0.f};
      gsr_cm_rsh<S>(GsrDual3{v[0], 1.f, 0.f, 0.f}, GsrDual3{v[1], 0.f, 1.f, 0.f}, GsrDual3{v[2], 0.f, 0.f, 1.f},
                    [&](int c, GsrDual3 y) {
                      const float k = dsh[i * K + c];
                      g[0] += k * y.dx; g[1] += k * y.dy; g[2] += k * y.dz;
                    });
      for (int k = 0; k < 3; ++k) dd[3 * i + k] = g[k];
    }
  }
}

extern "C" {

int hm_cm_rsh(int S, const float* d, int64_t n, float* out, const float* dsh, float* dd) {
  switch (S) {
    case 0: hm_cm_rsh_s<0>(d, n, out, dsh, dd); return 0;
    case 1: hm_cm_rsh_s<1>(d, n, out, dsh, dd); return 0;
    case 2: hm_cm_rsh_s<2>(d, n, out, dsh, dd); return 0;
    case 3: hm_cm_rsh_s<3>(d, n, out, dsh, dd); return 0;
    case 4: hm_cm_rsh_s<4>(d, n, out, dsh, dd); return 0;
    case 5: hm_cm_rsh_s<5>(d, n, out, dsh, dd); return 0;
    default: return -1;
  }
}

void hm_cm_layernorm(const float* u, int64_t n, int F, const float* dy, float* y, float* du) {
  for (int64_t i = 0; i < n; ++i) {
    const float* r = u + i * F;
    float sum = 0.f, ss = 0.f;
    for (int f = 0; f < F; ++f) sum += r[f];
    const float mean = sum / (float)F;
    for (int f = 0; f < F; ++f) ss += (r[f] - mean) * (r[f] - mean);
    const float rstd = gsr_cm_ln_rstd(ss, F);
    float s1 = 0.f, s2 = 0.f;
    for (int f = 0; f < F; ++f) {
      y[i * F + f] = (r[f] - mean) * rstd;
      s1 += dy[i * F + f];
      s2 += dy[i * F + f] * y[i * F + f];
    }
    for (int f = 0; f < F; ++f) du[i * F + f] = gsr_cm_ln_bwd(y[i * F + f], dy[i * F + f], rstd, s1, s2, F);
  }
}

void hm_cm_glu(const float* a, const float* b, const float* dh, int64_t n, float* h, float* da, float* db) {
  for (int64_t i = 0; i < n; ++i) {
    h[i] = gsr_cm_glu(a[i], b[i]);
    gsr_cm_glu_bwd(a[i], b[i], dh[i], da[i], db[i]);
  }
}

void hm_cm_lum(const float* o, int64_t n, float bias, const float* dout, float* out, float* do_) {
  for (int64_t i = 0; i < n; ++i) {
    gsr_cm_lum(o + 4 * i, bias, out + 3 * i);
    gsr_cm_lum_bwd(o + 4 * i, bias, dout + 3 * i, do_ + 4 * i);
  }
}

void hm_cm_normalize(const float* v, const float* dd, int64_t n, float* d, float* dv) {
  for (int64_t i = 0; i < n; ++i) {
    float inv;
    bool clamped;
    gsr_cm_normalize(v + 3 * i, d + 3 * i, inv, clamped);
    gsr_cm_normalize_bwd(d + 3 * i, inv, clamped, dd + 3 * i, dv + 3 * i);
  }
}

}  // extern "C"

// frustum point queries and view features (gsr_visibility.h): the device's results bit for bit.
extern "C" {

void hm_frustum_counts(const float* p, int64_t N, const float* rec, int64_t V, float depth_below, int32_t* point_counts,
                       int32_t* camera_counts) {
  if (camera_counts) for (int64_t c = 0; c < V; ++c) camera_counts[c] = 0;
  for (int64_t i = 0; i < N; ++i) {
    int32_t seen = 0;
    for (int64_t c = 0; c < V; ++c) {
      const bool in = gsr_vis_inside(rec + GSR_VIS_RECORD_FLOATS * c, p[3 * i], p[3 * i + 1], p[3 * i + 2], depth_below);
      seen += in ? 1 : 0;
      if (camera_counts && in) camera_counts[c] += 1;
    }
    if (point_counts) point_counts[i] = seen;
  }
}

int hm_view_features(const int64_t* labels, int64_t N, int64_t K, const int64_t* idx, const float* vis, int64_t M,
                     float threshold, float* out, int32_t* point_visible) {
  for (int64_t i = 0; i < N; ++i)
    if (labels[i] < 0 || labels[i] >= K) return -1;
  for (int64_t j = 0; j < M; ++j)
    if (idx[j] < 0 || idx[j] >= N) return -1;
  float* dense = new float[N]();
  int64_t* start = new int64_t[K + 1]();
  int64_t* order = new int64_t[N];
  for (int64_t j = 0; j < M; ++j) {
    dense[idx[j]] = gsr_vf_value(vis[j], threshold);
    if (point_visible) point_visible[idx[j]] += 1;
  }
  for (int64_t i = 0; i < N; ++i) start[labels[i] + 1] += 1;
  for (int64_t c = 0; c < K; ++c) start[c + 1] += start[c];
  {
    int64_t* fill = new int64_t[K];
    for (int64_t c = 0; c < K; ++c) fill[c] = start[c];
    for (int64_t i = 0; i < N; ++i) order[fill[labels[i]]++] = i;      // stable: ascending point index per cluster
    delete[] fill;
  }
  for (int64_t c = 0; c < K; ++c) {
    const int64_t s = start[c], e = start[c + 1];
    float lanes[64];
    for (int l = 0; l < 64; ++l) lanes[l] = 0.f;
    int64_t t = 0;
    for (int64_t a = s; a < e; ++t) {
      const int64_t b = (a / GSR_VF_CHUNK + 1) * GSR_VF_CHUNK < e ? (a / GSR_VF_CHUNK + 1) * GSR_VF_CHUNK : e;
      float piece = dense[order[a]];
      for (int64_t q = a + 1; q < b; ++q) piece += dense[order[q]];
      lanes[t & 63] += piece;
      a = b;
    }
    out[c] = gsr_vf_tree64(lanes);
  }
  delete[] dense;
  delete[] start;
  delete[] order;
  return 0;
}

}  // extern "C"

// sampling rate and 3-D smoothing filter (gsr_filter3d.h) on the host's libm: the device's order of operations.
extern "C" {

void hm_sampling_rate(const float* p, int64_t N, const float* rec, const float* focal, int64_t V, float margin,
                      float* rate) {
  for (int64_t i = 0; i < N; ++i) {
    float bf = 0.f, bd = 1.f;
    for (int64_t c = 0; c < V; ++c)
      gsr_f3d_pair(rec + GSR_VIS_RECORD_FLOATS * c, focal[c], margin, p[3 * i], p[3 * i + 1], p[3 * i + 2], &bf, &bd);
    rate[i] = gsr_f3d_rate(bf, bd);
  }
}

void hm_filter3d_forward(const float* ls, const float* a, const float* rate, int64_t N, float strength, float* out_ls,
                         float* out_a) {
  for (int64_t i = 0; i < N; ++i) {
    const float c = gsr_f3d_variance(rate[i], strength);
    if (c != 0.f) {
      gsr_f3d_forward_row(ls + 3 * i, a[i], c, out_ls + 3 * i, out_a + i);
    } else {
      for (int j = 0; j < 3; ++j) out_ls[3 * i + j] = ls[3 * i + j];
      out_a[i] = a[i];
    }
  }
}

void hm_filter3d_backward(const float* ls, const float* a, const float* rate, int64_t N, float strength, const float* g_ls,
                          const float* g_a, float* d_ls, float* d_a) {
  for (int64_t i = 0; i < N; ++i) {
    const float c = gsr_f3d_variance(rate[i], strength);
    if (c != 0.f) {
      gsr_f3d_backward_row(ls + 3 * i, a[i], c, g_ls + 3 * i, g_a[i], d_ls + 3 * i, d_a + i);
    } else {
      for (int j = 0; j < 3; ++j) d_ls[3 * i + j] = g_ls[3 * i + j];
      d_a[i] = g_a[i];
    }
  }
}

}  // extern "C"

// SH export fit (gsr_sh_fit.h): the device's updates and its solve, in its order, one point at a time.
namespace {

template <int K>
void shf_accumulate(const float* pos, int64_t N, const int64_t* idx, int64_t M, const float* col, const float* wts,
                    const float* cam, double* acc) {
  constexpr GsrShfTable<K> tab{};
  constexpr int R = GsrShfTable<K>::R;
  for (int64_t m = 0; m < M; ++m) {
    const int64_t i = idx[m];
    if (i < 0 || i >= N) continue;
    double e[GsrShfTable<K>::E];
    gsr_shf_operands<K>(pos + 3 * i, cam, col + 3 * m, e);
    double* row = acc + i * R;
    for (int j = 0; j < R; ++j) row[j] = gsr_shf_update(row[j], wts[m], e[tab.a[j]], e[tab.b[j]]);
  }
}

template <int K>
void shf_solve(const double* acc, int64_t N, float ridge, float* sh, float* weight) {
  constexpr int R = GsrShfTable<K>::R;
  double work[R];
  for (int64_t n = 0; n < N; ++n) gsr_shf_solve_row<K>(acc + n * R, ridge, work, sh + n * 3 * K, weight + n);
}

}  // namespace

extern "C" {

int hm_sh_fit_row_doubles(int K) { return gsr_shf_row_doubles(K); }

void hm_sh_fit_accumulate(const float* pos, int64_t N, const int64_t* idx, int64_t M, const float* col, const float* wts,
                          const float* cam, int K, double* acc) {
  switch (K) {
    case 1: shf_accumulate<1>(pos, N, idx, M, col, wts, cam, acc); break;
    case 4: shf_accumulate<4>(pos, N, idx, M, col, wts, cam, acc); break;
    case 9: shf_accumulate<9>(pos, N, idx, M, col, wts, cam, acc); break;
    case 16: shf_accumulate<16>(pos, N, idx, M, col, wts, cam, acc); break;
  }
}

void hm_sh_fit_solve(const double* acc, int64_t N, int K, float ridge, float* sh, float* weight) {
  switch (K) {
    case 1: shf_solve<1>(acc, N, ridge, sh, weight); break;
    case 4: shf_solve<4>(acc, N, ridge, sh, weight); break;
    case 9: shf_solve<9>(acc, N, ridge, sh, weight); break;
    case 16: shf_solve<16>(acc, N, ridge, sh, weight); break;
  }
}

}  // extern "C"

// MCMC position noise (gsr_controller.h) on the host's libm: the device's order of operations, one row at a time.
extern "C" {

void hm_philox4x32(const uint32_t* counter, const uint32_t* key, uint32_t* out) { gsr_philox4x32(counter, key, out); }

void hm_mcmc_draws(uint64_t first, int64_t N, uint64_t seed, uint64_t step, uint32_t* words, float* normals) {
  for (int64_t i = 0; i < N; ++i) {
    uint32_t w[4];
    float z[4];
    gsr_mcmc_words(first + (uint64_t)i, seed, step, w);
    gsr_mcmc_normals(w, z);
    for (int j = 0; j < 4 && words; ++j) words[4 * i + j] = w[j];
    for (int j = 0; j < 3 && normals; ++j) normals[3 * i + j] = z[j];
  }
}

void hm_mcmc_level(const float* alpha_logit, int64_t N, float opacity_threshold, float margin, float noise_level,
                   float* level) {
  for (int64_t i = 0; i < N; ++i) level[i] = gsr_mcmc_level(alpha_logit[i], opacity_threshold, margin, noise_level);
}

void hm_mcmc_noise(float* position, const float* log_scaling, const float* rotation_xyzw, const float* alpha_logit,
                   const int16_t* points_in_view, int64_t N, int32_t min_views, float opacity_threshold, float margin,
                   float noise_level, float scale_eps, uint64_t seed, uint64_t step) {
  for (int64_t i = 0; i < N; ++i) {
    if (!(points_in_view[i] > min_views)) continue;
    const float level = gsr_mcmc_level(alpha_logit[i], opacity_threshold, margin, noise_level);
    if (level != 0.f)
      gsr_mcmc_noise_row(position + 3 * i, log_scaling + 3 * i, rotation_xyzw + 4 * i, level, scale_eps, (uint64_t)i, seed,
                         step);
  }
}

}  // extern "C"

// MCMC relocation (gsr_relocate.h): the device's arithmetic and its argument checks in plain loops.
extern "C" {

void hm_reloc_words(uint64_t k, uint64_t seed, uint64_t step, int32_t domain, uint32_t* out) {
  gsr_reloc_words(k, seed, step, (uint32_t)domain, out);
}

int hm_weighted_draws(const uint32_t* weights, int64_t N, int64_t n, uint64_t seed, uint64_t step, int32_t domain,
                      int32_t* sources_out, int32_t* counts_out, uint64_t* total_out, void* workspace,
                      size_t workspace_bytes) {
  const int rc = gsr_weighted_draws_check(weights, N, n, domain, sources_out, counts_out, total_out, workspace,
                                          workspace_bytes);
  if (rc < 0) return rc;
  uint64_t* block_incl = (uint64_t*)workspace;
  const int64_t blocks = (N + GSR_RELOC_BLOCK - 1) / GSR_RELOC_BLOCK;
  uint64_t S = 0;
  for (int64_t b = 0; b < blocks; ++b) {
    for (int64_t i = b * GSR_RELOC_BLOCK; i < N && i < (b + 1) * GSR_RELOC_BLOCK; ++i) {
      S += weights[i];
      counts_out[i] = 0;
    }
    block_incl[b] = S;
  }
  *total_out = S;
  for (int64_t k = 0; k < n; ++k) {
    sources_out[k] = -1;
    if (S == 0) continue;
    const uint64_t t = gsr_reloc_target((uint64_t)k, seed, step, (uint32_t)domain, S);
    int64_t lo = 0, hi = blocks - 1;                                  // block_incl[blocks - 1] = S > t
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (block_incl[mid] > t) hi = mid;
      else lo = mid + 1;
    }
    uint64_t P = lo ? block_incl[lo - 1] : 0;
    for (int64_t i = lo * GSR_RELOC_BLOCK; i < N; ++i) {
      P += weights[i];
      if (P > t) {
        sources_out[k] = (int32_t)i;
        counts_out[i] += 1;
        break;
      }
    }
  }
  return GSR_OK;
}

int hm_relocate_weights(const float* alpha_logit, const uint8_t* alive, int64_t N, uint32_t* weights_out) {
  int launch = 0;
  const int rc = gsr_relocate_weights_check(alpha_logit, N, weights_out, &launch);
  if (rc < 0 || !launch) return rc;
  for (int64_t i = 0; i < N; ++i) weights_out[i] = gsr_reloc_weight(alpha_logit[i], alive ? alive[i] != 0 : true);
  return GSR_OK;
}

int hm_relocate_rescale(float* alpha_logit, float* log_scaling, const int32_t* counts, int64_t N, float o_floor) {
  int launch = 0;
  const int rc = gsr_relocate_rescale_check(alpha_logit, log_scaling, counts, N, o_floor, &launch);
  if (rc < 0 || !launch) return rc;
  for (int64_t r = 0; r < N; ++r) {
    if (!(counts[r] > 0)) continue;
    float a_new;
    double log_coeff;
    gsr_reloc_rescale(alpha_logit[r], counts[r], (double)o_floor, &a_new, &log_coeff);
    alpha_logit[r] = a_new;
    for (int j = 0; j < 3; ++j) log_scaling[3 * r + j] = (float)((double)log_scaling[3 * r + j] + log_coeff);
  }
  return GSR_OK;
}

void hm_reloc_rescale_rows(const float* alpha_logit, const int32_t* counts, int64_t n, float o_floor, float* a_out,
                           double* log_coeff) {
  for (int64_t i = 0; i < n; ++i) gsr_reloc_rescale(alpha_logit[i], counts[i], (double)o_floor, a_out + i, log_coeff + i);
}

int hm_relocate_rows(const int32_t* dst_rows, const int32_t* src_rows, int64_t n, int64_t N, const void* columns,
                     int32_t n_columns) {
  const GsrRowColumnC* cols = (const GsrRowColumnC*)columns;
  int launch = 0;
  const int rc = gsr_relocate_rows_check(dst_rows, src_rows, n, N, cols, n_columns, &launch);
  if (rc < 0 || !launch) return rc;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t dst = dst_rows[k], src = src_rows[k];
    if (dst < 0 || dst >= N || src < 0 || src >= N) continue;
    for (int c = 0; c < n_columns; ++c) {
      uint32_t* data = (uint32_t*)cols[c].data;
      const int64_t w = cols[c].width_dwords;
      for (int64_t d = 0; d < w; ++d) {
        if (cols[c].zero) data[dst * w + d] = data[src * w + d] = 0u;
        else data[dst * w + d] = data[src * w + d];
      }
    }
  }
  return GSR_OK;
}

}  // extern "C"

// ---- pose tables (gsr_camera_table.h) ----

extern "C" {

int hm_pose_forward(const float* q_left, const float* t_left, int64_t A_left, const int64_t* idx_left,
                    const float* q_right, const float* t_right, int64_t A_right, const int64_t* idx_right, int64_t B,
                    float* T) {
  bool bad = false;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t l = gsr_pose_index(idx_left[b], A_left, &bad);
    if (q_right) {
      const int64_t r = gsr_pose_index(idx_right[b], A_right, &bad);
      gsr_pose_forward_image(q_left + 4 * l, t_left + 3 * l, q_right + 4 * r, t_right + 3 * r, T + 16 * b);
    } else {
      gsr_pose_forward_image(q_left + 4 * l, t_left + 3 * l, nullptr, nullptr, T + 16 * b);
    }
  }
  return bad ? -1 : 0;
}

int hm_pose_backward(const float* q_left, const float* t_left, int64_t A_left, const int64_t* idx_left,
                     const float* q_right, const float* t_right, int64_t A_right, const int64_t* idx_right, int64_t B,
                     const float* d_T, float* d_q_left, float* d_t_left, float* d_q_right, float* d_t_right) {
  bool bad = false;
  for (int64_t a = 0; a < A_left && d_q_left; ++a)
    bad |= gsr_pose_backward_row(true, a, q_left, A_left, idx_left, q_right, t_right, A_right, idx_right, B, d_T,
                                 d_q_left + 4 * a, d_t_left + 3 * a);
  for (int64_t a = 0; q_right && a < A_right && d_q_right; ++a)
    bad |= gsr_pose_backward_row(false, a, q_right, A_right, idx_right, q_left, t_left, A_left, idx_left, B, d_T,
                                 d_q_right + 4 * a, d_t_right + 3 * a);
  return bad ? -1 : 0;
}

void hm_hist_entry(const float* v, const float* w, int64_t n, float eps, int32_t mode, float min_value, int32_t* cls,
                   float* t) {
  for (int64_t i = 0; i < n; ++i) cls[i] = gsr_hist_entry(v[i], w != nullptr, w ? w[i] : 0.f, eps, mode, min_value, t + i);
}

void hm_hist_bin(const float* t, int64_t n, float lo, float hi, int32_t num_bins, int32_t trim, int32_t* bin,
                 int32_t* outside) {
  for (int64_t i = 0; i < n; ++i) {
    int o;
    bin[i] = gsr_hist_bin(t[i], lo, hi, num_bins, trim != 0, &o);
    outside[i] = o;
  }
}

void hm_hist_keys(const float* x, int64_t n, uint32_t* key, float* back) {
  for (int64_t i = 0; i < n; ++i) {
    key[i] = gsr_hist_key(x[i]);
    back[i] = gsr_hist_unkey(key[i]);
  }
}

int hm_histogram(const float* values, int64_t N, int64_t C, const int64_t* rows, int64_t M, const float* weight,
                 float eps, int32_t mode, float min_value, float lo, float hi, int32_t num_bins, int32_t auto_range,
                 int32_t trim, int64_t* counts, double* stats) {
  if (!counts || !stats || N < 0 || M < 0 || C < 1 || mode < 0 || mode > 2 || num_bins < 1) return -1;
  if (!auto_range && !(gsr_hist_finite(lo) && gsr_hist_finite(hi) && hi >= lo)) return -1;
  for (int b = 0; b < num_bins; ++b) counts[b] = 0;
  for (int k = 0; k < 8; ++k) stats[k] = 0.0;
  const int64_t R = rows ? M : N;
  uint32_t min_c = 0u, max_k = 0u;
  for (int pass = auto_range ? 0 : 1; pass < 2; ++pass) {
    if (pass == 1 && auto_range) {
      lo = gsr_hist_unkey(~min_c);
      hi = gsr_hist_unkey(max_k);
    }
    for (int64_t r = 0; r < R; ++r) {
      const int64_t src = rows ? rows[r] : r;
      for (int64_t c = 0; c < C; ++c) {
        float t = 0.f;
        const int cls = src < 0 || src >= N ? GSR_HIST_NONFINITE
                                            : gsr_hist_entry(values[src * C + c], weight != nullptr,
                                                             weight ? weight[src] : 0.f, eps, mode, min_value, &t);
        if (pass == 0) {
          if (cls == GSR_HIST_KEPT) {
            const uint32_t k = gsr_hist_key(t);
            min_c = ~k > min_c ? ~k : min_c;
            max_k = k > max_k ? k : max_k;
          }
          continue;
        }
        stats[5] += cls == GSR_HIST_DROPPED;
        stats[6] += cls == GSR_HIST_NONFINITE;
        if (cls != GSR_HIST_KEPT) continue;
        stats[3] = stats[0] == 0.0 || t < stats[3] ? (double)t : stats[3];
        stats[4] = stats[0] == 0.0 || t > stats[4] ? (double)t : stats[4];
        stats[0] += 1.0;
        int outside;
        const int b = gsr_hist_bin(t, lo, hi, num_bins, trim != 0, &outside);
        stats[7] += outside;
        if (b >= 0) {
          ++counts[b];
          stats[1] += (double)t;
          stats[2] += (double)t * (double)t;
        }
      }
    }
  }
  return 0;
}

// ---- area resize of uint8 images (gsr_image.h) ----
int hm_image_resize_area_u8(const uint8_t* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, uint8_t* dst, int32_t Hd,
                            int32_t Wd) {
  int launch = 0;
  const int rc = gsr_image_check(src, B, Hs, Ws, C, dst, Hd, Wd, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrImageDivisor dv = gsr_image_divisor(Ws, Hs);
  const int64_t n_el = (int64_t)Wd * C;
  uint64_t* acc = new uint64_t[n_el];
  for (int64_t b = 0; b < B; ++b) {
    for (int32_t d = 0; d < Hd; ++d) {
      for (int64_t e = 0; e < n_el; ++e) acc[e] = 0;
      for (int32_t y = gsr_area_first(d, Hs, Hd); y <= gsr_area_last(d, Hs, Hd); ++y) {
        const uint64_t wy = gsr_area_weight(d, y, Hs, Hd);
        const uint8_t* row = src + ((b * Hs + y) * (int64_t)Ws) * C;
        for (int32_t j = 0; j < Wd; ++j) {
          const int32_t i_lo = gsr_area_first(j, Ws, Wd), i_hi = gsr_area_last(j, Ws, Wd);
          for (int32_t c = 0; c < C; ++c) {
            uint32_t h = 0;
            for (int32_t i = i_lo; i <= i_hi; ++i) h += gsr_area_weight(j, i, Ws, Wd) * row[(int64_t)i * C + c];
            acc[(int64_t)j * C + c] += wy * h;
          }
        }
      }
      uint8_t* out = dst + (b * Hd + d) * n_el;
      for (int64_t e = 0; e < n_el; ++e) out[e] = (uint8_t)gsr_image_round_div(acc[e], dv.m, dv.D, dv.shift);
    }
  }
  delete[] acc;
  return GSR_OK;
}

void hm_image_round_div(const uint64_t* sum, int64_t n, int32_t Ws, int32_t Hs, uint32_t* out) {
  const GsrImageDivisor dv = gsr_image_divisor(Ws, Hs);
  for (int64_t i = 0; i < n; ++i) out[i] = gsr_image_round_div(sum[i], dv.m, dv.D, dv.shift);
}

// ---- lens undistortion (gsr_undistort.h) ----
int hm_undistort_map(const double* source, const double* target, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd,
                     int32_t* map_out) {
  int launch = 0;
  const int rc = gsr_undistort_map_check(source, target, Hs, Ws, Hd, Wd, map_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrLens m = gsr_lens_make(source, target);
  for (int32_t v = 0; v < Hd; ++v)
    for (int32_t u = 0; u < Wd; ++u) {
      double xs, ys;
      gsr_undistort_point(m, (double)u, (double)v, &xs, &ys);
      int32_t* out = map_out + 2 * ((int64_t)v * Wd + u);
      out[0] = gsr_undistort_quantise(xs, Ws);
      out[1] = gsr_undistort_quantise(ys, Hs);
    }
  return GSR_OK;
}

void hm_undistort_points(const double* source, const double* target, int32_t Hs, int32_t Ws, int64_t n, const double* uv,
                         int32_t* out) {
  const GsrLens m = gsr_lens_make(source, target);
  for (int64_t i = 0; i < n; ++i) {
    double xs, ys;
    gsr_undistort_point(m, uv[2 * i], uv[2 * i + 1], &xs, &ys);
    out[2 * i] = gsr_undistort_quantise(xs, Ws);
    out[2 * i + 1] = gsr_undistort_quantise(ys, Hs);
  }
}

int hm_image_remap_u8(const uint8_t* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, const int32_t* map, uint8_t* dst,
                      int32_t Hd, int32_t Wd) {
  int launch = 0;
  const int rc = gsr_image_remap_check(src, B, Hs, Ws, C, map, dst, Hd, Wd, &launch);
  if (rc < 0 || !launch) return rc;
  const int64_t n_px = (int64_t)Hd * Wd;
  if (Hs == 0 || Ws == 0) {                                            // every tap lies outside an empty source
    memset(dst, 0, (size_t)B * n_px * C);
    return GSR_OK;
  }
  for (int64_t i = 0; i < n_px; ++i) {
    const GsrRemapAxis ax = gsr_remap_axis(map[2 * i], Ws), ay = gsr_remap_axis(map[2 * i + 1], Hs);
    const uint32_t w[4] = {ay.w0 * ax.w0, ay.w0 * ax.w1, ay.w1 * ax.w0, ay.w1 * ax.w1};
    const int64_t at[4] = {((int64_t)ay.i0 * Ws + ax.i0) * C, ((int64_t)ay.i0 * Ws + ax.i1) * C,
                           ((int64_t)ay.i1 * Ws + ax.i0) * C, ((int64_t)ay.i1 * Ws + ax.i1) * C};
    for (int64_t b = 0; b < B; ++b) {
      const uint8_t* image = src + b * Hs * (int64_t)Ws * C;
      for (int32_t c = 0; c < C; ++c) {
        uint32_t sum = 0;
        for (int k = 0; k < 4; ++k)
          if (w[k]) sum += w[k] * image[at[k] + c];
        dst[(b * n_px + i) * C + c] = (uint8_t)gsr_remap_round(sum);
      }
    }
  }
  return GSR_OK;
}

// ---- depth-map fusion (gsr_fusion.h) ----
int hm_fuse_check(const float* ref_depth, int32_t Hr, int32_t Wr, const double* ref_intrinsics, const void* sources_,
                  const double* source_params, int32_t S, const double* tolerances, uint8_t* counts) {
  const GsrFuseSource* sources = reinterpret_cast<const GsrFuseSource*>(sources_);
  int launch = 0;
  const int rc = gsr_fuse_check_args(ref_depth, Hr, Wr, ref_intrinsics, sources, source_params, S, tolerances, counts,
                                     &launch);
  if (rc < 0 || !launch) return rc;
  const GsrFuseRef ref = {ref_intrinsics[0], ref_intrinsics[1], ref_intrinsics[2], ref_intrinsics[3]};
  const GsrFuseView* views = reinterpret_cast<const GsrFuseView*>(source_params);      // 16 doubles each
  for (int32_t i = 0; i < Hr; ++i)
    for (int32_t j = 0; j < Wr; ++j) {
      const int64_t px = (int64_t)i * Wr + j;
      const double d = (double)ref_depth[px];
      if (!gsr_fuse_valid(d)) continue;
      double X, Y;
      gsr_fuse_unproject(ref, i, j, d, &X, &Y);
      uint32_t agree = 0, violate = 0;
      for (int s = 0; s < S; ++s) {
        int32_t is, js;
        double p2;
        if (!gsr_fuse_project(views[s], sources[s].H, sources[s].W, tolerances[0], X, Y, d, &is, &js, &p2)) continue;
        const int vote = gsr_fuse_vote((double)sources[s].depth[(int64_t)is * sources[s].W + js], p2, tolerances[1]);
        agree += vote == GSR_FUSE_AGREE;
        violate += vote == GSR_FUSE_VIOLATE;
      }
      counts[2 * px] = gsr_fuse_saturate(counts[2 * px] + agree);
      counts[2 * px + 1] = gsr_fuse_saturate(counts[2 * px + 1] + violate);
    }
  return GSR_OK;
}

void hm_fuse_votes(const double* ds, const double* p2, int64_t n, const double* rel_tol, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = gsr_fuse_vote(ds[i], p2[i], rel_tol[0]);
}

int hm_fuse_mask(const float* ref_depth, const uint8_t* counts, int32_t Hr, int32_t Wr, int32_t min_agree,
                 int32_t max_violate, uint8_t* keep_out) {
  int launch = 0;
  const int rc = gsr_fuse_mask_args(ref_depth, counts, Hr, Wr, min_agree, max_violate, keep_out, &launch);
  if (rc < 0 || !launch) return rc;
  for (int64_t px = 0; px < (int64_t)Hr * Wr; ++px)
    keep_out[px] = gsr_fuse_keep((double)ref_depth[px], counts[2 * px], counts[2 * px + 1], min_agree, max_violate) ? 1 : 0;
  return GSR_OK;
}

int hm_fuse_emit(const float* ref_depth, const uint8_t* counts, const float* image, int32_t Hr, int32_t Wr,
                 const double* ref_intrinsics, const double* world_t_ref, int32_t min_agree, int32_t max_violate,
                 int64_t base, int64_t capacity, float* points_out, uint8_t* colors_out, uint8_t* agree_out) {
  int launch = 0;
  const uint32_t no_block_offsets = 0;       // the walk below ranks the pixels itself; the check wants a pointer
  const int rc = gsr_fuse_emit_args(ref_depth, counts, Hr, Wr, ref_intrinsics, world_t_ref, min_agree, max_violate,
                                    &no_block_offsets, base, capacity, points_out, colors_out, agree_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrFuseRef ref = {ref_intrinsics[0], ref_intrinsics[1], ref_intrinsics[2], ref_intrinsics[3]};
  int64_t row = base;
  for (int32_t i = 0; i < Hr; ++i)
    for (int32_t j = 0; j < Wr; ++j) {
      const int64_t px = (int64_t)i * Wr + j;
      const double d = (double)ref_depth[px];
      if (!gsr_fuse_keep(d, counts[2 * px], counts[2 * px + 1], min_agree, max_violate)) continue;
      if (row >= capacity) return GSR_OK;
      double X, Y;
      gsr_fuse_unproject(ref, i, j, d, &X, &Y);
      for (int k = 0; k < 3; ++k) {
        points_out[3 * row + k] = (float)gsr_fuse_row(world_t_ref + 4 * k, X, Y, d);
        colors_out[3 * row + k] = image ? gsr_fuse_colour(image[3 * px + k]) : (uint8_t)255;
      }
      agree_out[row] = counts[2 * px];
      ++row;
    }
  return GSR_OK;
}

void hm_voxel_keys(const float* points, int64_t n, const double* grid, uint64_t* keys) {
  const GsrVoxelGrid g = gsr_voxel_grid_make(grid);
  for (int64_t i = 0; i < n; ++i) keys[i] = gsr_voxel_key_of(g, points + 3 * i);
}

int hm_voxel_downsample(const float* points, const uint8_t* colors, int64_t N, const double* grid, float* points_out,
                        uint8_t* colors_out, int32_t* counts_out, int64_t* K_out) {
  int launch = 0;
  const int rc = gsr_voxel_args(points, colors, N, grid, points_out, colors_out, counts_out, K_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrVoxelGrid g = gsr_voxel_grid_make(grid);
  std::vector<std::pair<uint64_t, int64_t>> order((size_t)N);
  for (int64_t i = 0; i < N; ++i) order[(size_t)i] = {gsr_voxel_key_of(g, points + 3 * i), i};
  std::sort(order.begin(), order.end());               // (key, index): the stable order
  int64_t K = 0;
  for (int64_t b = 0; b < N;) {
    int64_t e = b, S[3] = {0, 0, 0}, C[3] = {0, 0, 0};
    for (; e < N && order[(size_t)e].first == order[(size_t)b].first; ++e) {
      const int64_t at = order[(size_t)e].second;
      for (int k = 0; k < 3; ++k) {
        int32_t q;
        int64_t F;
        gsr_voxel_axis(points[3 * at + k], g.origin[k], g.inv, &q, &F);
        S[k] += F;
        C[k] += colors[3 * at + k];
      }
    }
    for (int k = 0; k < 3; ++k) {
      points_out[3 * K + k] = gsr_voxel_mean(g.origin[k], g.voxel, gsr_voxel_key_axis(order[(size_t)b].first, k), S[k], e - b);
      colors_out[3 * K + k] = gsr_voxel_colour(C[k], e - b);
    }
    counts_out[K++] = (int32_t)(e - b);
    b = e;
  }
  K_out[0] = K;
  return GSR_OK;
}

// ---- TSDF meshing (gsr_mesh.h) ----
int hm_tsdf_integrate(int32_t* state, int32_t nx, int32_t ny, int32_t nz, const double* grid, const void* sources_,
                      const double* source_params, int32_t S, const double* tsdf) {
  const GsrTsdfSource* sources = reinterpret_cast<const GsrTsdfSource*>(sources_);
  int launch = 0;
  const int rc = gsr_tsdf_integrate_args(state, nx, ny, nz, grid, sources, source_params, S, tsdf, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  const GsrTsdfParams p = gsr_tsdf_params_make(grid, tsdf);
  GsrTsdfSourceSet set = {};
  gsr_tsdf_source_set_make(sources, source_params, S, &set);
  const int64_t nodes = g.nodes();
  for (int64_t node = 0; node < nodes; ++node) {
    int32_t c[3];
    g.node_coords((uint32_t)node, c);
    const double X = gsr_tsdf_position(p.origin[0], p.voxel, c[0]), Y = gsr_tsdf_position(p.origin[1], p.voxel, c[1]),
                 Z = gsr_tsdf_position(p.origin[2], p.voxel, c[2]);
    GsrTsdfDelta d = {};
    for (int s = 0; s < S; ++s) gsr_tsdf_observe(set, s, p, X, Y, Z, &d);
    state[node] += d.sum_d;
    state[nodes + node] += d.n;
    state[2 * nodes + node] += d.nc;
    for (int k = 0; k < 3; ++k) state[(3 + k) * nodes + node] += d.c[k];
  }
  return GSR_OK;
}

int hm_mesh_vertex_mask(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight, uint8_t* active_out) {
  int launch = 0;
  const int rc = gsr_mesh_vertex_mask_args(state, nx, ny, nz, min_weight, active_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  for (int64_t cell_id = 0; cell_id < g.cells(); ++cell_id) {
    int32_t c[3];
    GsrMeshCell cell;
    g.cell_coords((uint32_t)cell_id, c);
    gsr_mesh_load_cell(state, g, c, &cell);
    active_out[cell_id] = gsr_mesh_active(cell, min_weight) ? 1 : 0;
  }
  return GSR_OK;
}

int hm_mesh_vertex_emit(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, const double* grid, int32_t min_weight,
                        int64_t capacity, int32_t* cell_vertex_out, float* vertices_out, uint8_t* colors_out) {
  int launch = 0;
  const int rc = gsr_mesh_vertex_emit_args(state, nx, ny, nz, grid, min_weight, nullptr, false, capacity, cell_vertex_out,
                                           vertices_out, colors_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  const GsrTsdfParams p = gsr_tsdf_params_make(grid, nullptr);
  const int64_t nodes = g.nodes();
  int64_t row = 0;
  for (int64_t cell_id = 0; cell_id < g.cells(); ++cell_id) {
    int32_t c[3];
    GsrMeshCell cell;
    g.cell_coords((uint32_t)cell_id, c);
    gsr_mesh_load_cell(state, g, c, &cell);
    if (!gsr_mesh_active(cell, min_weight)) {
      cell_vertex_out[cell_id] = -1;
      continue;
    }
    cell_vertex_out[cell_id] = (int32_t)row;
    if (row < capacity) {
      gsr_mesh_vertex(cell, c, p, vertices_out + 3 * row);
      int64_t nc = 0, C[3] = {0, 0, 0};
      for (int k = 0; k < 8; ++k) {
        const uint32_t node = gsr_mesh_corner_node(g, c, k);
        nc += state[2 * nodes + node];
        for (int ch = 0; ch < 3; ++ch) C[ch] += state[(3 + ch) * nodes + node];
      }
      for (int ch = 0; ch < 3; ++ch) colors_out[3 * row + ch] = gsr_mesh_colour(C[ch], nc);
    }
    ++row;
  }
  return GSR_OK;
}

int hm_mesh_face_mask(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                      const int32_t* cell_vertex, uint8_t* keep_out) {
  int launch = 0;
  const int rc = gsr_mesh_face_mask_args(state, nx, ny, nz, min_weight, cell_vertex, keep_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  for (int64_t e = 0; e < 3 * g.nodes(); ++e) {
    bool lower_negative;
    int32_t q[4];
    keep_out[e] = gsr_mesh_edge_kept(state, cell_vertex, g, (uint32_t)e, min_weight, &lower_negative, q) ? 1 : 0;
  }
  return GSR_OK;
}

int hm_mesh_face_emit(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                      const int32_t* cell_vertex, int64_t capacity, int32_t* faces_out) {
  int launch = 0;
  const int rc = gsr_mesh_face_emit_args(state, nx, ny, nz, min_weight, cell_vertex, nullptr, false, capacity, faces_out,
                                         &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  int64_t row = 0;
  for (int64_t e = 0; e < 3 * g.nodes(); ++e) {
    bool lower_negative;
    int32_t q[4], t[6];
    if (!gsr_mesh_edge_kept(state, cell_vertex, g, (uint32_t)e, min_weight, &lower_negative, q)) continue;
    gsr_mesh_quad(q, lower_negative, t);
    for (int k = 0; k < 2; ++k, ++row)
      if (row < capacity)
        for (int j = 0; j < 3; ++j) faces_out[3 * row + j] = t[3 * k + j];
  }
  return GSR_OK;
}

}  // extern "C"
