/* The ABI of the CPU unit-test shim (hostmath_shim.cpp -> libgsr_hostmath.so): every hm_* entry point is declared here and
 * nowhere else.  The shim compiles with -Werror=missing-declarations, so a definition without a declaration here, or one
 * that disagrees with it, does not build; tests/hostmath.py derives the ctypes binding from this text with
 * _lib.parse_header, the reader of include/gsplat_hip.h, so it stays in that dialect: plain C, no conditionals. */
#ifndef GSR_HOSTMATH_SHIM_H
#define GSR_HOSTMATH_SHIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-splat projection, SH basis and tile test (gsr_math.h) ---- */
/* params: 8 x 4 bytes laid out as GsrRasterParams */
void hm_project_forward(const float* T, const float* proj, const void* params, int64_t M, const float* pos,
                        const float* ls, const float* rot, const float* logit, float* g2d, float* depth,
                        float* sscale);
void hm_project_backward(const float* T, const float* proj, const void* params, int64_t M, const float* pos,
                         const float* ls, const float* rot, const float* logit, const float* dg2d,
                         const float* ddepth, float* dpos, float* dls, float* drot, float* dlogit);
/* per-splat camera terms of the K2 backward: cam[M, 16] (gsr_math.h: GSR_CAM_GRAD_FLOATS layout), overwritten */
void hm_project_backward_camera(const float* T, const float* proj, const void* params, int64_t M, const float* pos,
                                const float* ls, const float* rot, const float* logit, const float* dg2d,
                                const float* ddepth, float* cam);
/* dT[12] += the fold of dL/d(camera position) dcam[3] through cam = -R^T t */
void hm_fold_camera_position(const float* T, const float* dcam, float* dT);
void hm_in_view(const float* T, const float* proj, int64_t N, const float* pos, int W, int H, float near_p,
                float far_p, float margin, uint8_t* mask);
void hm_sh_basis(int K, int64_t M, const float* dirs, float* Y);
/* per-splat tile hit mask over the whole tile grid: hits[m * tiles_x * tiles_y + ty * tiles_x + tx] */
void hm_tile_hits(const void* params, int64_t M, const float* g2d, int tiles_x, int tiles_y, uint8_t* hits);
/* gsr_splat_extent per splat: extent [M, 4] int32 = x0 x1 y0 y1 (half-open tile rectangle) and qmax [M] */
void hm_splat_extent(const void* params, int64_t M, const float* g2d, int tiles_x, int tiles_y, int32_t* extent,
                     float* qmax);
/* K4's verdict over the whole tile grid: masks[m * tiles_x * tiles_y + ty * tiles_x + tx] = bit 0 upper / bit 1 lower half
 * (zero-filled by the caller; tiles outside the extent are not written).  Extents above 32 tiles pass the whole-tile
 * test first, as the device's wave path does. */
void hm_tile_half_masks(const void* params, int64_t M, const float* g2d, int tiles_x, int tiles_y, uint8_t* masks);

/* ---- bilateral-grid slice of one image (gsr_bilagrid.h) with ONE grid [12, L, GH, GW] ---- */
void hm_bilagrid_forward(const float* grid, int L, int GH, int GW, const float* rgb, int H, int W, float* out);
/* d_rgb [H, W, 3] and d_grid [12, L, GH, GW] (summed in double, overwritten) */
void hm_bilagrid_backward(const float* grid, int L, int GH, int GW, const float* rgb, int H, int W, const float* d_out,
                          float* d_rgb, float* d_grid);

/* ---- colour fit of the evaluation pass (gsr_eval.h) ---- */
/* sums [3][45]: the moments of iterate x [P, 3] against ref over the pixels unclipped in x0, x and ref, in pixel order */
void hm_color_fit_moments(const float* x0, const float* x, const float* ref, int64_t P, float eps, double* sums);
/* w [10]: the weights of one channel from its 45 sums */
void hm_color_fit_solve(const double* sums, double* w);
/* The whole fit in the device's order of operations (eval.hip): min(ceil(P / 256), 1024) blocks of 256 threads, a thread
 * takes the pixels block * 256 + thread + i * blocks * 256 in ascending order, 64 lanes are added in the shuffle tree
 * v[l] += v[l + off] (off = 32 .. 1), the 4 waves in order, then the blocks' slots in order.  out [P, 3]. */
void hm_color_fit(const float* x0, const float* ref, int64_t P, int num_iters, float eps, float* out);

/* ---- brute-force kNN and nearest-centroid assignment (gsr_neighbours.h): the device's results bit for bit ---- */
/* one sweep over j = 0 .. N-1 per query.  Rows [i0, i1) of dist2 [N, k], idx [N, k] int64 and scale [N], written from
 * row 0 of the outputs; returns -1 for k outside 1..16, N <= k or a bad row range. */
int hm_knn(const float* p, int64_t N, int k, int64_t i0, int64_t i1, float* dist2, int64_t* idx, float* scale);
void hm_assign_clusters(const float* x, int64_t N, const float* c, int64_t K, int64_t* labels);

/* ---- colour-model row maths (gsr_color.h), one row at a time, each with its derivative ---- */
/* out [n, (S+1)^2] (NULL: skipped); dd [n, 3] = sum_c dsh[c] dY_c/dd (NULL: skipped).  Returns -1 for S outside 0..5. */
int hm_cm_rsh(int S, const float* d, int64_t n, float* out, const float* dsh, float* dd);
/* rows u [n, F]: y = LayerNorm(u) and du for an upstream dy */
void hm_cm_layernorm(const float* u, int64_t n, int F, const float* dy, float* y, float* du);
void hm_cm_glu(const float* a, const float* b, const float* dh, int64_t n, float* h, float* da, float* db);
/* o [n, 4] -> out [n, 3]; do_ [n, 4] for an upstream dout [n, 3] */
void hm_cm_lum(const float* o, int64_t n, float bias, const float* dout, float* out, float* do_);
/* v [n, 3] -> d = F.normalize(v) and dv for an upstream dd */
void hm_cm_normalize(const float* v, const float* dd, int64_t n, float* d, float* dv);

/* ---- frustum point queries and view features (gsr_visibility.h): the device's results bit for bit ---- */
/* points [N, 3], records [V, 16]; point_counts [N] / camera_counts [V] int32 (either may be NULL). */
void hm_frustum_counts(const float* p, int64_t N, const float* rec, int64_t V, float depth_below, int32_t* point_counts,
                       int32_t* camera_counts);
/* labels [N] int64 in [0, K); idx [M] int64 distinct in [0, N), vis [M]; out [K]; point_visible [N] int32 (may be NULL)
 * is incremented.  Returns -1 for a label or an index out of range. */
int hm_view_features(const int64_t* labels, int64_t N, int64_t K, const int64_t* idx, const float* vis, int64_t M,
                     float threshold, float* out, int32_t* point_visible);

/* ---- sampling rate and 3-D smoothing filter (gsr_filter3d.h) on the host's libm: the device's order of operations ---- */
/* points [N, 3], records [V, 16], focal [V]; rate [N] */
void hm_sampling_rate(const float* p, int64_t N, const float* rec, const float* focal, int64_t V, float margin,
                      float* rate);
/* ls / out_ls [N, 3], a / rate / out_a [N] */
void hm_filter3d_forward(const float* ls, const float* a, const float* rate, int64_t N, float strength, float* out_ls,
                         float* out_a);
void hm_filter3d_backward(const float* ls, const float* a, const float* rate, int64_t N, float strength, const float* g_ls,
                          const float* g_a, float* d_ls, float* d_a);

/* ---- SH export fit (gsr_sh_fit.h): the device's updates and its solve, in its order, one point at a time ---- */
int hm_sh_fit_row_doubles(int K);
/* pos [N, 3], idx / wts [M], col [M, 3], cam [3]; acc [N, R(K)] is added to */
void hm_sh_fit_accumulate(const float* pos, int64_t N, const int64_t* idx, int64_t M, const float* col, const float* wts,
                          const float* cam, int K, double* acc);
/* acc [N, R(K)]; sh [N, 3, K], weight [N] */
void hm_sh_fit_solve(const double* acc, int64_t N, int K, float ridge, float* sh, float* weight);

/* ---- MCMC position noise (gsr_controller.h) on the host's libm: the device's order of operations, row by row ---- */
void hm_philox4x32(const uint32_t* counter, const uint32_t* key, uint32_t* out);
/* words [N, 4] and normals [N, 3] of rows first .. first + N - 1 (either may be NULL) */
void hm_mcmc_draws(uint64_t first, int64_t N, uint64_t seed, uint64_t step, uint32_t* words, float* normals);
/* level [N] of alpha_logit [N] */
void hm_mcmc_level(const float* alpha_logit, int64_t N, float opacity_threshold, float margin, float noise_level,
                   float* level);
/* the row loop of gsr_mcmc_noise, in place on position [N, 3] */
void hm_mcmc_noise(float* position, const float* log_scaling, const float* rotation_xyzw, const float* alpha_logit,
                   const int16_t* points_in_view, int64_t N, int32_t min_views, float opacity_threshold, float margin,
                   float noise_level, float scale_eps, uint64_t seed, uint64_t step);

/* ---- MCMC relocation (gsr_relocate.h): the device's arithmetic and argument checks in plain loops ---- */
/* out [4]: the Philox words of draw k at (seed, step) in `domain` */
void hm_reloc_words(uint64_t k, uint64_t seed, uint64_t step, int32_t domain, uint32_t* out);
/* gsr_weighted_draws on host memory, with its checks and codes: a binary search over the block prefixes, then the rows of
 * the block in order */
int hm_weighted_draws(const uint32_t* weights, int64_t N, int64_t n, uint64_t seed, uint64_t step, int32_t domain,
                      int32_t* sources_out, int32_t* counts_out, uint64_t* total_out, void* workspace,
                      size_t workspace_bytes);
int hm_relocate_weights(const float* alpha_logit, const uint8_t* alive, int64_t N, uint32_t* weights_out);
int hm_relocate_rescale(float* alpha_logit, float* log_scaling, const int32_t* counts, int64_t N, float o_floor);
/* the new logit and the fp64 log(coeff) of n source rows, counts >= 1 each */
void hm_reloc_rescale_rows(const float* alpha_logit, const int32_t* counts, int64_t n, float o_floor, float* a_out,
                           double* log_coeff);
/* columns: n_columns GsrRowColumnC of include/gsplat_hip.h (16 bytes each: data, width_dwords, zero) */
int hm_relocate_rows(const int32_t* dst_rows, const int32_t* src_rows, int64_t n, int64_t N, const void* columns,
                     int32_t n_columns);

/* ---- pose tables (gsr_camera_table.h): the device's order of operations ---- */
/* q [A, 4], t [A, 3], idx [B]; the right table may be absent (all three NULL).  T [B, 4, 4].  Returns -1 when an index is
 * outside its table (it then reads row 0, as on the device), 0 otherwise. */
int hm_pose_forward(const float* q_left, const float* t_left, int64_t A_left, const int64_t* idx_left,
                    const float* q_right, const float* t_right, int64_t A_right, const int64_t* idx_right, int64_t B,
                    float* T);
/* d_T [B, 4, 4]; d_q / d_t of each table whose pair is given (a pair may be NULL), every row written */
int hm_pose_backward(const float* q_left, const float* t_left, int64_t A_left, const int64_t* idx_left,
                     const float* q_right, const float* t_right, int64_t A_right, const int64_t* idx_right, int64_t B,
                     const float* d_T, float* d_q_left, float* d_t_left, float* d_q_right, float* d_t_right);

/* ---- histogram entry and bin rules (gsr_histogram.h): the device's functions, one entry at a time ---- */
/* cls [n] int32 (0 kept, 1 dropped, 2 non-finite) and t [n] (written where kept) of v [n]; w [n] may be NULL */
void hm_hist_entry(const float* v, const float* w, int64_t n, float eps, int32_t mode, float min_value, int32_t* cls,
                   float* t);
/* bin [n] int32 (-1: outside with trim on) and outside [n] int32 of kept values t [n] */
void hm_hist_bin(const float* t, int64_t n, float lo, float hi, int32_t num_bins, int32_t trim, int32_t* bin,
                 int32_t* outside);
/* gsr_histogram on the host, entries in row order, the sums in fp64 in that order: counts [num_bins], stats [8].
 * Returns -1 for arguments gsr_histogram rejects. */
int hm_histogram(const float* values, int64_t N, int64_t C, const int64_t* rows, int64_t M, const float* weight,
                 float eps, int32_t mode, float min_value, float lo, float hi, int32_t num_bins, int32_t auto_range,
                 int32_t trim, int64_t* counts, double* stats);
/* key [n] uint32 of x [n] and back [n] = unkey(key) */
void hm_hist_keys(const float* x, int64_t n, uint32_t* key, float* back);

/* ---- area resize of uint8 images (gsr_image.h): the device's arithmetic in a plain loop ---- */
/* gsr_image_resize_area_u8 on host memory, with its argument checks and its codes.  (Every name of this header starts
 * with hm_, the prefix its reader takes; the package calls this one when a dataset has no GPU.) */
int hm_image_resize_area_u8(const uint8_t* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, uint8_t* dst, int32_t Hd,
                            int32_t Wd);
/* out [n] = floor((2 sum[i] + D) / (2 D)) by the multiply-shift of gsr_image_divisor(Ws, Hs); sum[i] <= 255 Ws Hs */
void hm_image_round_div(const uint64_t* sum, int64_t n, int32_t Ws, int32_t Hs, uint32_t* out);

/* ---- lens undistortion (gsr_undistort.h): the device's arithmetic in plain loops ---- */
/* gsr_undistort_map on host memory, with its argument checks and its codes: source [9], target [4], map_out [Hd, Wd, 2] */
int hm_undistort_map(const double* source, const double* target, int32_t Hs, int32_t Ws, int32_t Hd, int32_t Wd,
                     int32_t* map_out);
/* the same map at n destination coordinates uv [n, 2] (whole numbers held as doubles): out [n, 2].  No checks. */
void hm_undistort_points(const double* source, const double* target, int32_t Hs, int32_t Ws, int64_t n, const double* uv,
                         int32_t* out);
/* gsr_image_remap_u8 on host memory, with its argument checks and its codes */
int hm_image_remap_u8(const uint8_t* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, const int32_t* map, uint8_t* dst,
                      int32_t Hd, int32_t Wd);

/* ---- depth-map fusion (gsr_fusion.h): the device's arithmetic in plain loops, with its argument checks and codes ---- */
/* gsr_fuse_check on host memory: sources [S] GsrFuseSource of include/gsplat_hip.h (16 bytes each: depth, H, W) */
int hm_fuse_check(const float* ref_depth, int32_t Hr, int32_t Wr, const double* ref_intrinsics, const void* sources,
                  const double* source_params, int32_t S, const double* tolerances, uint8_t* counts);
/* the vote alone, on doubles: out [n] int32 (0 none, 1 agree, 2 violate) of source depths ds [n] against p2 [n] */
void hm_fuse_votes(const double* ds, const double* p2, int64_t n, const double* rel_tol, int32_t* out);
int hm_fuse_mask(const float* ref_depth, const uint8_t* counts, int32_t Hr, int32_t Wr, int32_t min_agree,
                 int32_t max_violate, uint8_t* keep_out);
/* gsr_fuse_emit on host memory; the kept pixels are ranked in a plain row-major walk, so it takes no block offsets */
int hm_fuse_emit(const float* ref_depth, const uint8_t* counts, const float* image, int32_t Hr, int32_t Wr,
                 const double* ref_intrinsics, const double* world_t_ref, int32_t min_agree, int32_t max_violate,
                 int64_t base, int64_t capacity, float* points_out, uint8_t* colors_out, uint8_t* agree_out);
/* gsr_voxel_downsample on host memory: a stable sort of the 63-bit keys, then the runs in order; K_out [1] */
int hm_voxel_downsample(const float* points, const uint8_t* colors, int64_t N, const double* grid, float* points_out,
                        uint8_t* colors_out, int32_t* counts_out, int64_t* K_out);
/* keys [n] of points [n, 3] as uint64 */
void hm_voxel_keys(const float* points, int64_t n, const double* grid, uint64_t* keys);

/* ---- TSDF meshing (gsr_mesh.h): the device's arithmetic in plain loops, with its argument checks and codes ---- */
/* gsr_tsdf_integrate on host memory: sources [S] GsrTsdfSource of include/gsplat_hip.h (24 bytes each: depth, image, H, W) */
int hm_tsdf_integrate(int32_t* state, int32_t nx, int32_t ny, int32_t nz, const double* grid_host, const void* sources_host,
                      const double* source_params_host, int32_t S, const double* tsdf_host);
int hm_mesh_vertex_mask(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight, uint8_t* active_out);
/* the emit twins rank in a plain walk in index order, so they take no block offsets */
int hm_mesh_vertex_emit(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, const double* grid_host,
                        int32_t min_weight, int64_t capacity, int32_t* cell_vertex_out, float* vertices_out,
                        uint8_t* colors_out);
int hm_mesh_face_mask(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                      const int32_t* cell_vertex, uint8_t* keep_out);
int hm_mesh_face_emit(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                      const int32_t* cell_vertex, int64_t capacity, int32_t* faces_out);

#ifdef __cplusplus
}
#endif

#endif
