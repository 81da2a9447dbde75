/* gsplat_hip.h -- C ABI of the MI355X (gfx950) differentiable Gaussian-splat rasterizer.
 *
 * This is the drop-in boundary underneath the three Python calls splat-trainer makes into taichi_splatting
 * (the reference has no C/FFI layer of its own):
 *
 *     project_to_image(gaussians, camera_params, config)            splat_trainer/scene/mlp_scene.py:375,415
 *     render_projected(indexes, gaussians2d, features, depth, ...)  splat_trainer/scene/mlp_scene.py:377-378,418-419
 *     evaluate_sh_at(sh_features, positions, indexes, camera_pos)   splat_trainer/scene/transfer_sh.py:49
 *     loss.backward()  (autograd node of the above)                 splat_trainer/trainer/trainer.py:512
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (torch ``data_ptr()``) unless the name ends in ``_host``;
 *   - all floating-point data is float32, row-major, contiguous; index tensors at the boundary are int64;
 *   - nothing here allocates, frees or synchronises: callers pass workspaces sized by the *_workspace_bytes
 *     queries and a ``hipStream_t`` (as ``void*``; NULL = default stream); calls only enqueue work;
 *   - camera: ``T_camera_world`` = 16 floats (4x4 row-major world->camera), ``projection`` = fx, fy, cx, cy in
 *     pixels (splat_trainer/trainer/trainer.py:291-301); both stay on the device, so no host sync is needed;
 *   - return value: 0 (GSR_OK) or a negative GSR_ERR_* code; the library never throws and never prints;
 *   - M = 0 and O = 0 are valid inputs everywhere (the reference treats "no visible points" as a caller-level
 *     error, splat_trainer/trainer/trainer.py:507-509, not a boundary error).
 *
 * The maths each entry point implements is specified in oracle/torch_oracle.py (header comment).
 *
 * This file is the one place the ABI is written down: the ctypes binding (splat-trainer_amd/_lib.py) reads it at import
 * and derives its prototypes, struct mirrors and constants from it.  Keep declarations in the forms used below --
 * `typedef struct X { ... } X;`, plain `T name`, `T a, b` and `T name[n]` fields, `RET gsr_name(ARGS);`, integer
 * `#define GSR_NAME value`, C comments -- a form the binding cannot read stops its import with the line's number.
 */
#ifndef GSPLAT_HIP_H
#define GSPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_ERR_INVALID_ARGUMENT -1
#define GSR_ERR_WORKSPACE_TOO_SMALL -2
#define GSR_ERR_LAUNCH_FAILED -3
#define GSR_ERR_UNSUPPORTED -4

#define GSR_ROW_FLOATS 16      /* packed per-splat row, 64 bytes, splat order:  u v A B | C op qlim f0 | f1 f2 depth log2(op) | 0 0 0 0
                                  (qlim = min(q_max, 2 ln(op / alpha_threshold)): a pixel contributes iff q <= qlim);
                                  the gradient rows use the same pitch:  mx my mxx mxy | myy dop prune split | df0 df1 df2 vis | 0 0 0 0 */
#define GSR_PARTIAL_FLOATS 12  /* per-(tile,splat) gradient partial: mx my mxx mxy | myy m0 prune split | df0 df1 df2 -
                                  (m* = moments of G dL/dG about the splat's mean, m0 the zeroth; the per-splat sweep turns
                                  their sums into du = A mx + B my, dv = B mx + C my, dA = -mxx/2, dB = -mxy, dC = -myy/2,
                                  dopacity = m0 / opacity) */
#define GSR_MAX_FEATURES 16     /* feature channels of the three-call form: C in 1..GSR_MAX_FEATURES */
#define GSR_WIDE_MIN_FEATURES 4 /* C >= 4 takes the wide path: features in a second table feat_rows [M, CW], CW = 4, 8 or 16
                                   (the smallest that holds C; zero-padded), geometry rows with zero colour slots, and
                                   per-pair partials of 8 + CW floats:  mx my mxx mxy | myy m0 prune split | df0 .. df(CW-1) */

#ifndef GSR_HAVE_RASTER_PARAMS
#define GSR_HAVE_RASTER_PARAMS
/* Mirrors the RasterConfig fields the reference sets (trainer.py:305-310) plus this build's constants. */
typedef struct GsrRasterParamsC {
  float alpha_threshold;  /* 1/255 */
  float clamp_max_alpha;  /* 0.99 */
  float T_eps;            /* 1 - saturate_threshold (1e-4) */
  float q_max;            /* gaussian_scale^2 (9) */
  float blur;             /* blur_cov (+ aa_blur when antialias) */
  int32_t antialias;      /* 0 / 1 */
  int32_t tile_size;      /* must be 16 */
  float margin_px;        /* margin_tiles * tile_size */
} GsrRasterParamsC;
#endif

/* Heavy-tile list segmentation (optional; pass NULL where a GsrSegmentsC* is taken to composite every tile with one
 * wave).  All pointers are device buffers owned by the caller; tile_seg / seg_desc / seg_total are filled by
 * gsr_segment_plan, the seg_* pixel buffers are scratch written by the forward pass and read by the backward pass. */
typedef struct GsrSegmentsC {
  const uint32_t* tile_seg;   /* [num_tiles,2]: first segment, number of segments (0 = light tile); followed by
                                 [heavy_capacity]: the segments of heavy tiles, listed compactly by the plan */
  const uint32_t* seg_desc;   /* [capacity,4]: tile, list start, list end, index within the tile */
  const uint32_t* seg_total;  /* GSR_SEG_TOTAL_WORDS device words: [0] segments of this frame (<= capacity), [1] of them in
                                 heavy tiles, [16 + 32 x + c]: tiles of XCD band x in length class c (the forward pass's launch order) */
  int64_t capacity;           /* from gsr_segment_capacity */
  int64_t heavy_capacity;     /* from gsr_segment_heavy_capacity (<= capacity) */
  float* seg_P;               /* [capacity,256] */
  float* seg_TC;              /* [capacity,256,4], 16-byte aligned: (T, c0, c1, c2) per pixel slot; a wide frame keeps
                                 only T here, [capacity,256], and its colours in seg_col */
  int32_t* seg_last;          /* [capacity,256] */
  float* seg_median;          /* [capacity,256]; NULL unless a median depth image is requested */
  const uint32_t* tile_order; /* [GSR_TILE_ORDER_WORDS(num_tiles)]: the forward pass's launch order (tiles by XCD band and
                                 length class, filled by gsr_segment_plan), or NULL: tiles in image order */
  float* seg_col;             /* wide frames only (NULL otherwise): [capacity, CW/4, 256, 4], 16-byte aligned: channels
                                 4q .. 4q+3 of the colour composited up to the segment's end, per pixel slot */
} GsrSegmentsC;
#define GSR_SEG_TOTAL_WORDS 272
#define GSR_TILE_ORDER_WORDS(num_tiles) (8 * 32 * ((((num_tiles) + 127) / 128) * 16))

/* sizeof of the ABI's structs as the library was compiled: 0 GsrRasterParamsC, 1 GsrSegmentsC, 2 GsrFrameC,
 * 3 GsrFramePlanC, 4 GsrFrameResultC, 5 GsrFrameBackwardC (-1 otherwise) -- for a binding to check its own layout. */
int64_t gsr_struct_bytes(int32_t which);
#define GSR_ABI_VERSION 38                 /* bumped on any signature change; the one place the number is written */
int gsr_abi_version(void);                 /* GSR_ABI_VERSION of the library as it was compiled */
const char* gsr_error_string(int code);

/* ---- device-wide primitives (K5: radix bin + depth sort) ------------------------------------------------ */
size_t gsr_scan_workspace_bytes(int64_t n);
int gsr_exclusive_scan_u32(const uint32_t* in, uint32_t* out, int64_t n, uint32_t* total_dev, void* workspace,
                           size_t workspace_bytes, void* stream);
/* Same scan with an overflow guard: *overflow_dev (zero on entry) is set to 1 when a prefix or the total reaches 2^31
 * (beyond what the 32-bit list positions downstream can address; also raised before any u32 wrap can occur). */
int gsr_exclusive_scan_u32_checked(const uint32_t* in, uint32_t* out, int64_t n, uint32_t* total_dev,
                                   uint32_t* overflow_dev, void* workspace, size_t workspace_bytes, void* stream);
size_t gsr_sort_workspace_bytes(int64_t n);
/* Stable LSD radix sort of (key, value) pairs by key bits [begin_bit, end_bit); ping-pongs a<->b.
 * Returns 0 if the result ends in (keys_a, vals_a), 1 if in (keys_b, vals_b), negative on error.
 * n_dev (may be NULL): device word with the element count when n is only the capacity of the arrays (workspace sized
 * for n): the sort can then be enqueued before the count has reached the host; min(n, *n_dev) elements are sorted.
 * Read-ahead: all n slots of the input arrays -- keys, values and, in gsr_sort_pairs2_u32, the second values -- may be
 * read (never past n); what lies behind the count is not used. */
int gsr_sort_pairs_u32(uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, int64_t n,
                       int vals_are_iota, int begin_bit, int end_bit, void* workspace, size_t workspace_bytes,
                       const uint32_t* n_dev, void* stream);
/* Same, carrying a second value array with every key (the tile sort moves instance id + depth rank). */
int gsr_sort_pairs2_u32(uint32_t* keys_a, uint32_t* vals_a, uint32_t* vals2_a, uint32_t* keys_b, uint32_t* vals_b,
                        uint32_t* vals2_b, int64_t n, int vals_are_iota, int begin_bit, int end_bit, void* workspace,
                        size_t workspace_bytes, const uint32_t* n_dev, void* stream);

/* ---- K1 frustum cull + compaction  (project_to_image, first half) --------------------------------------- */
size_t gsr_cull_workspace_bytes(int64_t N);
/* indexes_out: int64[N] capacity, ascending point order; count_dev: uint32 = M. */
int gsr_frustum_cull(const float* position, int64_t N, const float* T_camera_world, const float* projection,
                     int32_t W, int32_t H, float near_plane, float far_plane, float margin_px,
                     int64_t* indexes_out, uint32_t* count_dev, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K2 3D->2D projection forward / backward  (project_to_image, second half) --------------------------- */
/* gaussians2d_out: [M,6] = u v A B C opacity; depth_out: [M].  count_dev (may be NULL): device word holding the
 * true number of valid entries of ``indexes`` (<= M); lets the call be enqueued right behind gsr_frustum_cull,
 * before the host has read the count back.  depth_keys_out (may be NULL): [M] the depth sort's keys, exactly what
 * gsr_depth_keys(depth_out, bias, max_key) would give (saves that launch when the caller rasterizes next). */
int gsr_project_forward(const float* position, const float* log_scaling, const float* rotation_xyzw,
                        const float* alpha_logit, const int64_t* indexes, int64_t M, const float* T_camera_world,
                        const float* projection, const GsrRasterParamsC* params_host, float* gaussians2d_out,
                        float* depth_out, const uint32_t* count_dev, uint32_t* depth_keys_out, uint32_t depth_key_bias,
                        uint32_t depth_key_max, void* stream);
/* Rows ``indexes`` of the N-sized gradient tensors are written (accumulate = 0: other rows untouched, pass
 * zeros) or added to (accumulate = 1: "+=" straight into the caller's .grad buffers; rows are unique, no atomics). */
int gsr_project_backward(const float* position, const float* log_scaling, const float* rotation_xyzw,
                         const float* alpha_logit, const int64_t* indexes, int64_t M, const float* T_camera_world,
                         const float* projection, const GsrRasterParamsC* params_host, const float* dL_dgaussians2d,
                         const float* dL_ddepth, float* d_position, float* d_log_scaling, float* d_rotation,
                         float* d_alpha_logit, int32_t accumulate, void* stream);

/* ---- camera gradient: dL/dT_camera_world and dL/dprojection (deterministic, no float atomics) -------------------
 * d_camera: 20 device floats = dL/dT_camera_world [16] (4x4 row major, row 3 zero) then dL/d(fx, fy, cx, cy).  Every
 * block of the camera-gradient kernels writes one partial row of 20 floats; camera_partials holds
 * gsr_camera_grad_partial_rows(count) such rows (count: the number of threads the kernel runs, M or N as noted). */
int64_t gsr_camera_grad_partial_rows(int64_t count);
/* gsr_project_backward plus the camera gradient (count = M); M = 0 writes zeros to d_camera.  The parameter gradients
 * are those of gsr_project_backward, bit for bit (the camera terms come from a kernel of their own). */
int gsr_project_backward_camera(const float* position, const float* log_scaling, const float* rotation_xyzw,
                                const float* alpha_logit, const int64_t* indexes, int64_t M, const float* T_camera_world,
                                const float* projection, const GsrRasterParamsC* params_host,
                                const float* dL_dgaussians2d, const float* dL_ddepth, float* d_position,
                                float* d_log_scaling, float* d_rotation, float* d_alpha_logit, int32_t accumulate,
                                float* camera_partials, float* d_camera, void* stream);
/* dL/d(camera position) [3] of the SH colours, from the Jacobian gsr_sh_forward saved (count = M); jacobian NULL
 * (K = 1) writes zeros. */
int gsr_sh_camera_position_grad(const float* dL_dcolors, const float* jacobian, int64_t M, float* camera_partials,
                                float* d_camera_pos, void* stream);
/* Sums `rows` partial rows in order.  T_camera_world given: folds the camera-position columns through cam = -R^T t and
 * writes the 20 floats above; NULL: writes dL/d(camera position) [3] alone. */
int gsr_camera_grad_finish(const float* camera_partials, int64_t rows, const float* T_camera_world, float* d_camera,
                           void* stream);

/* ---- K3 spherical-harmonics colour forward / backward  (evaluate_sh_at) --------------------------------- */
/* sh_features [N,3,K], K in {1,4,9,16}; colour = 0.5 + sum_k sh[c][k] Y_k(normalize(p - camera_pos)). */
/* jacobian_out [M,9] or NULL: d colour / d position (row-major 3x3 per splat), saved for the backward pass.
 * count_dev (may be NULL): device word holding the true row count when M is only an upper bound -- lets the caller
 * enqueue the colours right behind K1/K2, before the visible count has reached the host (as gsr_project_forward). */
int gsr_sh_forward(const float* sh_features, const float* positions, const int64_t* indexes, int64_t M, int32_t K,
                   const float* camera_pos, float* colors_out, float* jacobian_out, const uint32_t* count_dev,
                   void* stream);
/* d_sh_features [N,3,K] and d_positions [N,3] (may be NULL): rows ``indexes`` are written (accumulate = 0, pass
 * zeros) or added to (accumulate = 1).
 * d_positions is the gradient through the view direction normalize(p - camera_pos). */
int gsr_sh_backward(const float* dL_dcolors, const float* sh_features, const float* positions, const int64_t* indexes,
                    int64_t M, int32_t K, const float* camera_pos, const float* jacobian /* [M,9] or NULL */,
                    float* d_sh_features, float* d_positions, int32_t accumulate, void* stream);

/* inverse_out [N] int32: rank m of row r in the ascending list `indexes` [M], or -1 when the row is not in the list. */
int gsr_inverse_map(const int64_t* indexes, int64_t M, int64_t N, int32_t* inverse_out, void* stream);
/* Same gradient as gsr_sh_backward, but d_sh_features [N,3,K] is OVERWRITTEN for every scene row (zeros where the
 * camera saw nothing): the caller needs neither a zero-filled buffer nor a read-modify-write.  inverse [N] from
 * gsr_inverse_map, or NULL when M == N (every row visible, indexes = 0..N-1).  d_positions [N,3] (may be NULL) is
 * accumulated ("+="). */
int gsr_sh_backward_dense(const float* dL_dcolors, const float* sh_features, const float* positions,
                          const int32_t* inverse, int64_t M, int64_t N, int32_t K, const float* camera_pos,
                          const float* jacobian /* [M,9] or NULL */, float* d_sh_features, float* d_positions,
                          void* stream);

/* Multi-camera form for the data-parallel path.  Camera c's colour gradients, scattered to scene rows (all-zero rows
 * = not visible), start at dL_dcolors_dense + c * dense_stride ([N,3] floats each, dense_stride >= 3N); its position
 * (3 floats) at camera_positions + c * camera_stride.  (The strides let one all-gathered block per camera carry both:
 * [N+1,3] with the position in the last row.)  Adds sum_c g_c (x) Y(dir_c) to d_sh_features [N,3,K] -- or overwrites
 * every row when accumulate = 0 -- and adds the view-direction term to d_positions [N,3] (may be NULL), cameras in
 * index order.  Lets ranks exchange the 16x smaller colour gradients instead of all-reducing d_sh. */
int gsr_sh_backward_multi(const float* dL_dcolors_dense, int64_t dense_stride, const float* camera_positions,
                          int64_t camera_stride, int32_t num_cameras, const float* sh_features, const float* positions,
                          int64_t N, int32_t K, float* d_sh_features, float* d_positions, int32_t accumulate,
                          void* stream);

/* ---- K2 + K3 fused  (render_gaussians: project_to_image + evaluate_sh_at in one sweep) ------------------------ */
/* One [M,16] row per visible splat (GSR_ROW_FLOATS), written whole:  u v A B | C opacity qlim f0 | f1 f2 depth 0 | 0 0 0 0,
 * exactly the values gsr_project_forward + gsr_sh_forward return (same device code).  screen_scale_out [M,2];
 * jacobian_out [M,9] or NULL, depth_keys_out [M] or NULL, count_dev or NULL as in the two single calls.
 * Read-ahead: with count_dev the kernel requests `indexes` before it knows the count, at ranks up to M - 1: the array
 * holds M entries (what lies behind the count is never used as an index), and threads past the count read scene row 0. */
int gsr_project_sh_forward(const float* position, const float* log_scaling, const float* rotation_xyzw,
                           const float* alpha_logit, const float* sh_features, int32_t K, const int64_t* indexes, int64_t M,
                           const float* T_camera_world, const float* projection, const float* camera_pos,
                           const GsrRasterParamsC* params_host, float* rows_out, float* screen_scale_out,
                           float* jacobian_out, const uint32_t* count_dev, uint32_t* depth_keys_out,
                           uint32_t depth_key_bias, uint32_t depth_key_max, void* stream);
/* Backward of the geometry half from the packed gradient rows of gsr_reduce_gradients, one sequential sweep in splat
 * order: K2 backward into the N-sized gradient tensors (all four or none -- d_position NULL skips the geometry), plus
 * the position term of the colour gradient when ``jacobian`` [M,9] is given.  mode 0: rows ``indexes`` are written (the
 * others untouched: pass zeros); 1: added to ("+="); 2: EVERY scene row is written, zeros where the camera saw nothing
 * (no zero-fill by the caller, no read-modify-write) -- ``inverse`` [N] from gsr_inverse_map, or NULL when M == N.
 * dL_dgaussians2d_extra [M,6] / dL_ddepth [M] (may be NULL): gradients that reached gaussians2d / depth from outside the
 * rasterizer.  The rows' scalar columns are copied out where asked: d_colors_out [M,3] (input of the gsr_sh_backward*
 * calls), prune_cost_out / split_score_out / visibility_out [M]. */
int gsr_project_backward_rows(const float* position, const float* log_scaling, const float* rotation_xyzw,
                              const float* alpha_logit, const int64_t* indexes, int64_t M, const int32_t* inverse,
                              int64_t N, const float* T_camera_world, const float* projection,
                              const GsrRasterParamsC* params_host, const float* rows /* unused (the conic is recomputed); may be NULL */,
                              const float* grad_rows, const float* dL_dgaussians2d_extra, const float* dL_ddepth,
                              const float* jacobian,
                              float* d_position, float* d_log_scaling, float* d_rotation, float* d_alpha_logit,
                              int32_t mode, float* d_colors_out, float* prune_cost_out, float* split_score_out,
                              float* visibility_out, void* stream);
/* The same sweep plus the camera gradient (gsr_project_backward_camera's d_camera; count = M), with the view-direction
 * term -(d colour / d position)^T dL/dcolour of every splat when `jacobian` is given.  The geometry outputs are
 * required.  The parameter gradients are those of gsr_project_backward_rows, bit for bit. */
int gsr_project_backward_rows_camera(const float* position, const float* log_scaling, const float* rotation_xyzw,
                                     const float* alpha_logit, const int64_t* indexes, int64_t M, const int32_t* inverse,
                                     int64_t N, const float* T_camera_world, const float* projection,
                                     const GsrRasterParamsC* params_host, const float* rows, const float* grad_rows,
                                     const float* dL_dgaussians2d_extra, const float* dL_ddepth, const float* jacobian,
                                     float* d_position, float* d_log_scaling, float* d_rotation, float* d_alpha_logit,
                                     int32_t mode, float* d_colors_out, float* prune_cost_out, float* split_score_out,
                                     float* visibility_out, float* camera_partials, float* d_camera, void* stream);

/* ---- K4 tile overlap count / key emit, tile ranges  (render_projected, binning) ------------------------- */
/* depth -> sortable u32 keys, key = min(bits(depth) - bias, max_key), monotone in depth.  gsr_depth_key_range gives
 * (bias, max_key) for a camera's near / far planes: the keys of a frame then span only bits(far) - bits(near) -- 27
 * bits for 0.1 .. 100 -- and gsr_sort_pairs_u32(0, bit length of max_key) needs three passes instead of four (9-bit
 * digits).  bias 0 / max_key 0xFFFFFFFF (what the range call returns for a non-positive or infinite range): plain keys. */
int gsr_depth_key_range(float near_plane, float far_plane, uint32_t* bias_out, uint32_t* max_key_out);
int gsr_depth_keys(const float* depth, int64_t M, uint32_t bias, uint32_t max_key, uint32_t* keys_out, void* stream);
/* The three-call form's (M,6) gaussians2d + (M) depth + (M,C) features packed into the [M,16] rows everything downstream
 * reads (GSR_ROW_FLOATS; written whole, 64 bytes per splat, splat order); also screen_scale_out [M,2] =
 * (sigma_major, sigma_minor) in pixels, sqrt of the eigenvalues of the blurred 2D covariance.  The one-call form gets
 * the same rows straight from gsr_project_sh_forward. */
int gsr_pack_rows(const float* gaussians2d, const float* depth, const float* features, int64_t M, int32_t C,
                  const GsrRasterParamsC* params_host, float* rows_out, float* screen_scale_out, void* stream);
/* The same for GSR_WIDE_MIN_FEATURES <= C <= GSR_MAX_FEATURES, in one launch: rows_out [M,16] with zero colour slots and
 * feat_rows_out [M,CW] (CW = 4, 8 or 16, see GSR_WIDE_MIN_FEATURES; columns C..CW-1 zero). */
int gsr_pack_rows_wide(const float* gaussians2d, const float* depth, const float* features, int64_t M, int32_t C,
                       const GsrRasterParamsC* params_host, float* rows_out, float* feat_rows_out, float* screen_scale_out,
                       void* stream);
/* For rank k in depth order (order[k] = splat id): gathers the splat's row -- the one crossing of the depth-order
 * permutation on the forward side, one 64-byte line per splat -- and writes the number of tiles its support touches (a
 * tile counts when the support reaches the pixel centres of its upper or lower half) and tile_hits_out [M,4] uint32:
 * which tiles of the splat's extent were counted and which halves of each, for gsr_tile_emit (opaque to the caller). */
int gsr_tile_count(const float* rows, const uint32_t* order, int64_t M, int32_t W, int32_t H,
                   const GsrRasterParamsC* params_host, uint32_t* count_out, uint32_t* tile_hits_out,
                   const uint32_t* M_dev /* NULL, or the device word with the visible count when M is a capacity: ranks at
                                            or beyond it get count 0.  Read-ahead: order[] is requested before the
                                            count is known, at ranks up to M - 1: it holds M words, and what lies
                                            behind the count is never used as a row number (gsr_tile_count_offsets
                                            alike) */, void* stream);
/* gsr_tile_count followed by the exclusive scan of the counts in TWO launches instead of three (the count pass leaves
 * per-block totals in the workspace, the scan pass adds them up itself): offsets_out [M], total_dev = the pair count O,
 * overflow_flag raised when O reaches 2^31 (as gsr_exclusive_scan_u32_checked does).  M <= GSR_TILE_COUNT_OFFSETS_MAX
 * (beyond that the totals in front of a block are too many to add up per block: use gsr_tile_count + the scan). */
#define GSR_TILE_COUNT_OFFSETS_MAX 4194304
size_t gsr_tile_count_offsets_workspace_bytes(int64_t M);
int gsr_tile_count_offsets(const float* rows, const uint32_t* order, int64_t M, int32_t W, int32_t H,
                           const GsrRasterParamsC* params_host, uint32_t* count_out, uint32_t* tile_hits_out,
                           const uint32_t* M_dev, uint32_t* offsets_out, uint32_t* total_dev, uint32_t* overflow_flag,
                           void* workspace, size_t workspace_bytes, void* stream);
/* offsets = exclusive scan of count.  Instance i of rank k gets keys[offsets[k]+i] = tile id and
 * inst2splat[...] = order[k] | (half mask << 30): instances are emitted rank-major (already depth-sorted), the value they
 * carry is the splat id the composite kernels fetch the row by.
 * capacity = number of entries the two output arrays hold: instances at or beyond it are dropped, so the call may be
 * enqueued into buffers sized from a guess while the exact total is still on its way to the host (the caller compares
 * the total with the capacity afterwards and emits again if it was too small). */
int gsr_tile_emit(const float* rows, const uint32_t* order, const uint32_t* offsets, const uint32_t* tile_hits, int64_t M,
                  int32_t W, int32_t H, const GsrRasterParamsC* params_host, uint32_t* keys_out, uint32_t* inst2splat_out,
                  int64_t capacity, const uint32_t* M_dev /* as gsr_tile_count */, void* stream);
/* From the tile-sorted keys: per-tile [start, end).  tile_range must be zero-filled by the caller:
 * [num_tiles, 2] uint32. */
int gsr_tile_ranges(const uint32_t* sorted_keys, int64_t O, int32_t num_tiles, uint32_t* tile_range,
                    const uint32_t* O_dev /* NULL, or the device word with the count when O is a capacity */, void* stream);

/* ---- heavy-tile list segmentation ----------------------------------------------------------------------- */
/* One wave walks one tile's depth-sorted list serially.  A tile with more than seg_pairs pairs is cut into segments of
 * max(seg_pairs, ~len / 32) pairs: its forward walk (still one wave) leaves a checkpoint at every segment end and its
 * backward pass runs one wave per segment; a tile with more than heavy_min (>= seg_pairs) pairs is composited forward by
 * one wave per segment as well.
 *
 * seg_pairs_cfg / heavy_min_cfg > 0 fix the two thresholds; <= 0 selects them from the frame's pair count O (and
 * needs_grad): gsr_segment_thresholds returns the values a frame with O pairs is cut with.  The plan kernel evaluates
 * the same rule, from O or -- O_dev != NULL -- from the device word holding the count, so the plan can be enqueued
 * before the count has reached the host.
 * gsr_segment_capacity: host-side bound on the number of segments (sizes the buffers) of a frame with exactly O pairs
 * (O_is_bound = 0) or with at most O pairs (O_is_bound = 1). */
int gsr_segment_thresholds(int32_t seg_pairs_cfg, int32_t heavy_min_cfg, int64_t O, int32_t num_tiles, int32_t needs_grad,
                           int32_t* seg_pairs_out, int32_t* heavy_min_out);
int64_t gsr_segment_capacity(int64_t O, int32_t O_is_bound, int32_t seg_pairs_cfg, int32_t heavy_min_cfg, int32_t num_tiles,
                             int32_t needs_grad);
/* ... and on the number of those that belong to heavy tiles (the forward passes A and C launch one block each). */
int64_t gsr_segment_heavy_capacity(int64_t O, int32_t O_is_bound, int32_t seg_pairs_cfg, int32_t heavy_min_cfg,
                                   int32_t num_tiles, int32_t needs_grad);
/* tile_seg_out [2 num_tiles + heavy_capacity], seg_desc_out [capacity,4], seg_total_out [GSR_SEG_TOTAL_WORDS],
 * tile_order_out [GSR_TILE_ORDER_WORDS(num_tiles)] or NULL (see GsrSegmentsC); seg_total_out must be ZERO on entry
 * (tiles reserve their slots with integer atomics on it). */
int gsr_segment_plan(const uint32_t* tile_range, int32_t num_tiles, int32_t seg_pairs_cfg, int32_t heavy_min_cfg,
                     int32_t needs_grad, int64_t O, const uint32_t* O_dev, int64_t capacity, int64_t heavy_capacity,
                     uint32_t* tile_seg_out, uint32_t* seg_desc_out, uint32_t* seg_total_out, uint32_t* tile_order_out,
                     void* stream);
/* The same four with the frame's kind: wide = 1 for a frame of GSR_WIDE_MIN_FEATURES or more channels (0: the entry
 * points above).  Explicit thresholds mean the same for both kinds; only the automatic segment length with gradients
 * differs (256 pairs for a wide frame, whose checkpoints are 1 + CW floats per pixel), and it does not depend on the
 * channel count. */
int gsr_segment_thresholds_wide(int32_t seg_pairs_cfg, int32_t heavy_min_cfg, int64_t O, int32_t num_tiles,
                                int32_t needs_grad, int32_t wide, int32_t* seg_pairs_out, int32_t* heavy_min_out);
int64_t gsr_segment_capacity_wide(int64_t O, int32_t O_is_bound, int32_t seg_pairs_cfg, int32_t heavy_min_cfg,
                                  int32_t num_tiles, int32_t needs_grad, int32_t wide);
int64_t gsr_segment_heavy_capacity_wide(int64_t O, int32_t O_is_bound, int32_t seg_pairs_cfg, int32_t heavy_min_cfg,
                                        int32_t num_tiles, int32_t needs_grad, int32_t wide);
int gsr_segment_plan_wide(const uint32_t* tile_range, int32_t num_tiles, int32_t seg_pairs_cfg, int32_t heavy_min_cfg,
                          int32_t needs_grad, int32_t wide, int64_t O, const uint32_t* O_dev, int64_t capacity,
                          int64_t heavy_capacity, uint32_t* tile_seg_out, uint32_t* seg_desc_out, uint32_t* seg_total_out,
                          uint32_t* tile_order_out, void* stream);

/* ---- K6 alpha-composite forward ------------------------------------------------------------------------- */
/* image [H,W,C]; final_T [H,W]; last [H,W] int32 = 1 + list position of the last contributing splat;
 * median_depth [H,W] or NULL; vis_partial [O] (indexed by instance id; must be zero-filled) and pair_vis [O]
 * (the same per-(tile,splat) visibility sum_px T*alpha, indexed by sorted list position) or both NULL. */
int gsr_composite_forward(const float* rows /* [M,16] */, const uint32_t* sorted_splat, const uint32_t* sorted_inst,
                          const uint32_t* tile_range, int32_t W, int32_t H, int32_t C,
                          const GsrRasterParamsC* params_host, float* image_out, float* final_T_out,
                          int32_t* last_out, float* median_depth_out, float* vis_partial_out, float* pair_vis_out,
                          const GsrSegmentsC* segments_host /* or NULL */,
                          int32_t prefetch_rows /* speed only: touch the rows 32-64 pairs ahead of the walk (pays once the
                                                   row table has outgrown the caches: GSR_PREFETCH_MIN_ROWS).  With it
                                                   the walk fetches sorted_splat four words at a time and may read up
                                                   to THREE WORDS PAST the O-th entry (values unused): the buffer must be
                                                   readable that far (gsr_frame_plan sizes it so) */,
                          void* stream);
/* Wide frames (GSR_WIDE_MIN_FEATURES <= C <= GSR_MAX_FEATURES): the features come from feat_rows [M,CW]
 * (gsr_pack_rows_wide); image [H,W,C], the other outputs as gsr_composite_forward.  Channels, final_T, last, median and
 * the visibility partials are bit-identical to gsr_composite_forward for the same splats and the same segments.
 * gsr_composite_forward_wide composites every tile with one wave (no segments); the _seg form takes the segment tables
 * of gsr_segment_plan with the wide pixel slots (GsrSegmentsC: seg_TC holds T only, seg_col the colours), or NULL. */
int gsr_composite_forward_wide_seg(const float* rows /* [M,16] */, const float* feat_rows /* [M,CW] */,
                                   const uint32_t* sorted_splat, const uint32_t* sorted_inst, const uint32_t* tile_range,
                                   int32_t W, int32_t H, int32_t C, const GsrRasterParamsC* params_host, float* image_out,
                                   float* final_T_out, int32_t* last_out, float* median_depth_out, float* vis_partial_out,
                                   float* pair_vis_out, const GsrSegmentsC* segments_host /* or NULL */, void* stream);
int gsr_composite_forward_wide(const float* rows /* [M,16] */, const float* feat_rows /* [M,CW] */,
                               const uint32_t* sorted_splat, const uint32_t* sorted_inst, const uint32_t* tile_range,
                               int32_t W, int32_t H, int32_t C, const GsrRasterParamsC* params_host, float* image_out,
                               float* final_T_out, int32_t* last_out, float* median_depth_out, float* vis_partial_out,
                               float* pair_vis_out, void* stream);
#ifndef GSR_PREFETCH_MIN_ROWS
#define GSR_PREFETCH_MIN_ROWS 1000000
#endif

/* ---- K7 alpha-composite backward (per-pixel reverse walk) ----------------------------------------------- */
/* partial_out [O,12]: written only for pairs with pair_vis > 0 (the others are never read). */
int gsr_composite_backward(const float* rows /* [M,16] */, const uint32_t* sorted_splat, const uint32_t* sorted_inst,
                           const float* pair_vis, const uint32_t* tile_range, int32_t W, int32_t H, int32_t C,
                           const GsrRasterParamsC* params_host, const float* final_T, const int32_t* last,
                           const float* dL_dimage, const float* image /* the forward output; needed with segments */,
                           float* partial_out, const GsrSegmentsC* segments_host /* the forward pass's, or NULL */,
                           void* stream);
/* Wide frames: partial_out [O, 8 + CW] (see GSR_WIDE_MIN_FEATURES), written only for pairs with pair_vis > 0.  The _seg
 * form takes the forward pass's segments (or NULL) and, with them, the forward image: every segment gets a wave of its
 * own, entered from its checkpoint. */
int gsr_composite_backward_wide_seg(const float* rows /* [M,16] */, const float* feat_rows /* [M,CW] */,
                                    const uint32_t* sorted_splat, const uint32_t* sorted_inst, const float* pair_vis,
                                    const uint32_t* tile_range, int32_t W, int32_t H, int32_t C,
                                    const GsrRasterParamsC* params_host, const float* final_T, const int32_t* last,
                                    const float* dL_dimage, const float* image /* the forward output; needed with segments */,
                                    float* partial_out, const GsrSegmentsC* segments_host /* the forward pass's, or NULL */,
                                    void* stream);
int gsr_composite_backward_wide(const float* rows /* [M,16] */, const float* feat_rows /* [M,CW] */,
                                const uint32_t* sorted_splat, const uint32_t* sorted_inst, const float* pair_vis,
                                const uint32_t* tile_range, int32_t W, int32_t H, int32_t C,
                                const GsrRasterParamsC* params_host, const float* final_T, const int32_t* last,
                                const float* dL_dimage, float* partial_out, void* stream);

/* ---- deterministic per-splat reductions of the per-(tile,splat) partials -------------------------------- */
/* visibility_out [M] indexed by splat (not rank).  capacity = slots vis_partial holds (the pair count, or the bound
 * the buffers were sized with: slots at or beyond it are not read). */
int gsr_reduce_visibility(const float* vis_partial, const uint32_t* offsets, const uint32_t* count,
                          const uint32_t* order, int64_t M, float* visibility_out, int64_t capacity,
                          const uint32_t* M_dev /* as gsr_tile_count */, void* stream);
/* grad_rows_out [M,16] indexed by splat, each row written whole (the one crossing of the depth-order permutation on the
 * backward side):  mx my mxx mxy | myy dop prune_cost split_score | df0 df1 df2 visibility | 0 0 0 0  (m*: the summed
 * moments of GSR_PARTIAL_FLOATS; gsr_project_backward_rows / gsr_unpack_grad_rows turn them into d(u, v, A, B, C) with
 * the conic of the forward row).  The visibility column holds the same bits gsr_reduce_visibility returns. */
int gsr_reduce_gradients(const float* partial, const float* vis_partial, const uint32_t* offsets,
                         const uint32_t* count, const uint32_t* order, int64_t M, float* grad_rows_out, void* stream);
/* The same for the [O, 8 + CW] partials of gsr_composite_backward_wide, summed in the same order: grad_rows_out [M,16]
 * as above with df0..df2 = 0, and d_features_out [M,C] written directly (indexed by splat). */
int gsr_reduce_gradients_wide(const float* partial, const float* vis_partial, const uint32_t* offsets,
                              const uint32_t* count, const uint32_t* order, int64_t M, int32_t C, float* grad_rows_out,
                              float* d_features_out, void* stream);
/* The rows taken apart for the three-call form: d_gaussians2d [M,6], d_features [M,C]; prune_cost / split_score /
 * visibility [M] (each may be NULL).  d_features may be NULL (any C up to GSR_MAX_FEATURES): the feature gradient of a
 * wide frame comes from gsr_reduce_gradients_wide. */
int gsr_unpack_grad_rows(const float* rows /* the forward rows [M,16] */, const float* grad_rows, int64_t M, int32_t C,
                         float* d_gaussians2d, float* d_features, float* prune_cost_out, float* split_score_out,
                         float* visibility_out, void* stream);

/* ---- frame driver: the forward half of render_gaussians(use_sh = True) behind one call ---------------------
 * (scene.render -> project_to_image + evaluate_sh_at + render_projected, splat_trainer/scene/mlp_scene.py:410-427 /
 * scripts/test_split.py:30.)  The same launches as the single entry points above, chained with the two data-dependent
 * sizes of a frame left on the device: kernels run over the N scene rows and stop at the visible count M (counts[0]),
 * pair buffers hold `pair_capacity` pairs and every kernel reads the pair count O (counts[1]) on the device.  The host
 * receives counts[0..2] = [M, O, overflow flag] from the middle of the chain; when O > pair_capacity the frame is run again with a
 * larger capacity (nothing in the results depends on the capacity or on N as a bound). */
typedef struct GsrFrameC {
  const float* position;        /* [N,3] */
  const float* log_scaling;     /* [N,3] */
  const float* rotation_xyzw;   /* [N,4] */
  const float* alpha_logit;     /* [N]   */
  const float* sh_features;     /* [N,3,K] */
  int64_t N;
  int32_t K;                    /* 1, 4, 9 or 16 */
  int32_t W, H;
  const float* T_camera_world;  /* 16 floats */
  const float* projection;      /* fx fy cx cy */
  const float* camera_pos;      /* 3 floats */
  float near_plane, far_plane;
  GsrRasterParamsC params;
  int32_t want_jacobian;        /* save d colour / d position [M,9] for the backward pass */
  int32_t want_median;
  int32_t compute_visibility;
  int32_t needs_grad;           /* a backward pass will follow: per-pair visibility + checkpoints are kept */
  int32_t seg_pairs, seg_min_pairs;   /* RasterConfig.segment_pairs / segment_min_pairs */
  int64_t pair_capacity;
  /* Projected mode (position == NULL): the K4..K6 half of the three-call form, render_projected(indexes, gaussians2d,
   * features, depth, ...) (mlp_scene.py:418-419) -- the rows are packed from the caller's tensors, N is the exact number
   * of splats (nothing is culled here), C their feature channels, counts[0] is not used. */
  const float* gaussians2d;     /* [N,6] */
  const float* depth;           /* [N]   */
  const float* features;        /* [N,C] */
  int32_t C;                    /* 1..3, or up to GSR_MAX_FEATURES with feature_table (3 in the one-call form) */
  const uint32_t* depth_order;  /* [N] or NULL: the depth order when the caller has it already (skips the depth sort) */
  /* Projected mode: 1 = the caller takes C >= GSR_WIDE_MIN_FEATURES through the wide path (the plan lays out the
   * feature table feat_rows and, with seg_pairs != 0, the wide segment slots); 0 = C <= 3 only. */
  int32_t feature_table;
} GsrFrameC;
/* Byte offsets of the frame's buffers inside the two caller-owned arenas (-1: not present in this frame).  `out`:
 * everything the Rendering or the backward pass still needs after the forward pass; the first zero_bytes bytes are
 * zero-filled by the driver.  `work`: scratch that may be freed as soon as the forward pass has run. */
typedef struct GsrFramePlanC {
  int64_t out_bytes, work_bytes;
  int64_t zero_begin, zero_bytes;
  /* out arena */
  int64_t prune_cost, split_score, counts, tile_range, vis_partial, indexes, rows, screen_scale, jacobian, visibility,
      image, final_T, last, median, count, offsets, vals_a, vals_b, tvals_a, tvals_b, trank_a, trank_b, pair_vis,
      seg_tables, seg_pix, seg_last;
  int64_t seg_capacity, seg_heavy_capacity;
  /* work arena */
  int64_t cull_ws, sort_ws, scan_ws, tsort_ws, keys_a, keys_b, tile_hits, tkeys_a, tkeys_b;
  int64_t cull_ws_bytes, sort_ws_bytes, scan_ws_bytes, tsort_ws_bytes;
  int64_t feat_rows;            /* out arena: [N,CW] feature table of a wide frame, -1 otherwise */
  int64_t seg_col;              /* out arena: [seg_capacity, CW/4, 256, 4] colour checkpoints of a segmented wide frame (its
                                   seg_pix holds T, the alpha products and the median: one plane each), -1 otherwise */
} GsrFramePlanC;
/* Where the ping-pong sorts left their results (byte offsets into `out`) and the segment tables of the frame. */
typedef struct GsrFrameResultC {
  int64_t order;          /* [N] u32: splat id by depth rank (first M valid) */
  int64_t sorted_inst;    /* [pair_capacity] u32, or -1 when pair_capacity == 0 */
  int64_t sorted_splat;   /* [pair_capacity] u32 */
  GsrSegmentsC segments;  /* device pointers into `out`; valid when has_segments */
  int32_t has_segments;
} GsrFrameResultC;
int gsr_frame_plan(const GsrFrameC* frame_host, GsrFramePlanC* plan_out_host);
/* counts_host (pinned host memory, 3 words; may be NULL) receives [M, O, overflow] by an asynchronous copy issued right
 * behind the scan that finalises them -- the rest of the chain is enqueued behind it -- and event_counts (hipEvent_t, may
 * be NULL) is recorded after that copy: the caller waits on the event, not on the stream.
 * event_k6_begin / event_k6_end: hipEvent_t recorded around the composite launch (bench.py's roofline leg), or NULL. */
int gsr_frame_forward(const GsrFrameC* frame_host, const GsrFramePlanC* plan_host, void* out_arena, void* work_arena,
                      GsrFrameResultC* result_out_host, uint32_t* counts_host, void* event_counts, void* event_k6_begin,
                      void* event_k6_end, void* stream);

/* The backward half of the same frame behind one call (loss.backward() through the node of scene.render,
 * splat_trainer/trainer/trainer.py:512): K7 -> gsr_reduce_gradients -> (gsr_inverse_map) -> gsr_project_backward_rows ->
 * gsr_sh_backward(_dense), with the arguments those entry points take.  All buffers are the caller's. */
typedef struct GsrFrameBackwardC {
  /* scene and camera of the forward call */
  const float* position; const float* log_scaling; const float* rotation_xyzw; const float* alpha_logit;
  const float* sh_features;       /* [N,3,K]; only read when sh_mode != 0 */
  int64_t N; int32_t K; int32_t W, H, C;
  const float* T_camera_world; const float* projection; const float* camera_pos;
  GsrRasterParamsC params;
  /* what the forward pass left (gsr_frame_forward's out arena) */
  int64_t M, O;
  const int64_t* indexes; const float* rows; const uint32_t* order; const uint32_t* count; const uint32_t* offsets;
  const uint32_t* sorted_splat; const uint32_t* sorted_inst; const float* pair_vis; const float* vis_partial;
  const uint32_t* tile_range; const float* final_T; const int32_t* last; const float* image;
  const float* jacobian;          /* [M,9] or NULL */
  const GsrSegmentsC* segments;   /* host pointer, or NULL */
  /* incoming gradients: d_image [H,W,C] (NULL: nothing reached the image), and what reached gaussians2d / depth */
  const float* d_image; const float* d_gaussians2d; const float* d_depth;
  /* scratch */
  float* partial;                 /* [O, GSR_PARTIAL_FLOATS] */
  float* grad_rows;               /* [M, GSR_ROW_FLOATS] */
  int32_t* inverse;               /* [N]; needed when M < N and (mode == 2 or sh_mode == 1) */
  float* d_colors;                /* [M,3]; needed when sh_mode != 0 (may be given otherwise: the colour gradient) */
  /* outputs: geometry gradients [N,*] with gsr_project_backward_rows' mode; the SH coefficient gradient [N,3,K] with
   * sh_mode 0: none, 1: every row overwritten (gsr_sh_backward_dense), 2: rows of `indexes` accumulated; the per-point
   * outputs [M] (each may be NULL) */
  float* d_position; float* d_log_scaling; float* d_rotation; float* d_alpha_logit; int32_t mode;
  float* d_sh; int32_t sh_mode;
  float* prune_cost; float* split_score; float* visibility;
  /* camera gradient: d_camera [20] as gsr_project_backward_camera, or NULL for none; camera_partials
   * [gsr_camera_grad_partial_rows(M), 20] scratch.  The view-direction term is included when `jacobian` is given
   * (K > 1). */
  float* camera_partials; float* d_camera;
} GsrFrameBackwardC;
/* event_k7_begin / event_k7_end: hipEvent_t recorded around the composite backward launch, or NULL. */
int gsr_frame_backward(const GsrFrameBackwardC* backward_host, void* event_k7_begin, void* event_k7_end, void* stream);
/* The same in two halves: stages bit 0 = K7 + per-splat reduction (grad_rows complete behind it), bit 1 = the rest; 3 = all.
 * A data-parallel caller packs and starts exchanging the colour-gradient factors (grad_rows columns 8..10) in between. */
int gsr_frame_backward_stages(const GsrFrameBackwardC* backward_host, int32_t stages, void* event_k7_begin,
                              void* event_k7_end, void* stream);

/* ---- loss stage next to the path: fused SSIM, replaces the CUDA-only fused_ssim package
 *      the reference imports (splat_trainer/trainer/trainer.py:17,112,450-462; trainer/evaluation.py:7,42) ------------ */
size_t gsr_ssim_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
/* Mean SSIM (11x11 Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2) of img1 vs img2, both
 * [B,C,H,W] with arbitrary element strides (4 x int64 on the host: batch, channel, row, column -- NCHW,
 * channels_last and (H,W,C) views all work).  crop = 0: mean over the whole map ("same"); crop = 5: mean over the map
 * without its 5-pixel border ("valid", what the reference uses).  mean_out: device float.  dm_* ([B,C,H,W]
 * contiguous, all three or none): derivative maps consumed by gsr_ssim_backward. */
int gsr_ssim_forward(const float* img1, const float* img2, const int64_t* strides1_host, const int64_t* strides2_host,
                     int32_t B, int32_t C, int32_t H, int32_t W, int32_t crop, float* mean_out, float* dm_dmu1,
                     float* dm_dm11, float* dm_dm12, void* workspace, size_t workspace_bytes, void* stream);
/* d_img1 (element strides strides_out_host) = grad_scale * d mean / d img1; grad_scale_dev: device float. */
int gsr_ssim_backward(const float* img1, const float* img2, const int64_t* strides1_host, const int64_t* strides2_host,
                      const int64_t* strides_out_host, int32_t B, int32_t C, int32_t H, int32_t W, const float* dm_dmu1,
                      const float* dm_dm11, const float* dm_dm12, const float* grad_scale_dev, float* d_img1,
                      void* stream);

/* Pixel losses of the same stage (splat_trainer/trainer/trainer.py:465-488: l1 / mse on the image clamped to [0, 1]):
 * loss_out[0] = mean(f(clamp(image, lo, hi) - target)), f = square (kind 0) or abs (kind 1), over n contiguous floats
 * (16-byte aligned); fixed-order sums.  The backward writes grad_scale_dev[0] * d loss / d image, zero where the clamp
 * is active (torch.clamp's rule). */
size_t gsr_pixel_loss_workspace_bytes(int64_t n);
int gsr_pixel_loss_forward(const float* image, const float* target, int64_t n, int32_t kind, float lo, float hi,
                           float* loss_out, void* workspace, size_t workspace_bytes, void* stream);
int gsr_pixel_loss_backward(const float* image, const float* target, int64_t n, int32_t kind, float lo, float hi,
                            const float* grad_scale_dev, float* d_image, void* stream);

/* ---- optimizer stage next to the path: sparse visibility-aware Adam / LaProp step on the
 *      rows a batch has seen; replaces the Taichi kernels behind taichi_splatting.optim.ParameterClass.step
 *      (splat_trainer/scene/mlp_scene.py:214-230, options :58-60, groups config/scene/mlp.yaml:8-14).  Arithmetic:
 *      oracle/optim_oracle.py. ------------------------------------------------------------------------------------ */
/* Once per step.  indexes [M] int64, unique; visibility [M] or NULL (weight 1, no normalisation; vis_avg unused);
 * step [N] and vis_avg [N] are per-point state updated in place; row_scale_out [M,4] feeds gsr_opt_step. */
int gsr_opt_point_weights(const int64_t* indexes, const float* visibility, int64_t M, float* step, float* vis_avg,
                          float beta1, float beta2, float vis_beta, float vis_smooth, int32_t bias_correction,
                          float* row_scale_out, void* stream);
/* Once per parameter group, in place on rows `indexes` of param / exp_avg [N,D] and exp_avg_sq ([N,D] for type 0,
 * [N] otherwise).  type: 0 scalar, 1 vector (one second moment per row), 2 local_vector (D = 3, basis [M,3,3]
 * row-major: gradient and update expressed in the splat's own axes).  algo: 0 Adam, 1 LaProp.  grad_clip <= 0: off. */
int gsr_opt_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const int64_t* indexes,
                 const float* row_scale, const float* basis, int64_t M, int32_t D, int32_t type, int32_t algo, float lr,
                 float beta1, float beta2, float eps, float grad_clip, void* stream);
/* basis_out [M,3,3] row-major = R(normalize(rotation[i])) * diag(max(exp(log_scaling[i]), eps)), i = indexes[m] (NULL:
 * i = m): the frame local_vector groups step in (gaussians/split.py:16-20, mlp_scene.py:219-225). */
int gsr_point_basis(const float* log_scaling, const float* rotation_xyzw, const int64_t* indexes, int64_t M, float eps,
                    float* basis_out, void* stream);

/* ---- densify / prune support next to the path ------------------------------------------
 *      deterministic top-n mask replacing take_n = argsort(t)[:n] -> mask (splat_trainer/controller/target_controller.py:
 *      150-160) and fused keep-mask compaction + append of all per-point columns (scene.split_and_prune,
 *      splat_trainer/scene/mlp_scene.py:301-310; controller/point_state.py:76-110). -------------------------------- */
size_t gsr_select_workspace_bytes(int64_t N);
/* mask_out [N] bytes (0/1): the n smallest values (descending = 0) or the n largest (descending = 1); among equal
 * values the lowest indexes are taken (what a stable argsort gives); NaN orders above +inf, -0 equals +0. */
int gsr_select_n(const float* values, int64_t N, int64_t n, int32_t descending, uint8_t* mask_out, void* workspace,
                 size_t workspace_bytes, void* stream);

#define GSR_MAX_COLUMNS 32
typedef struct GsrColumnC {
  const void* src;       /* [N, width] 4-byte words: the column before compaction */
  void* dst;             /* [kept + n_tail, width]: kept rows in order, then the appended rows */
  const void* tail;      /* [n_tail, width] appended rows, or NULL: the appended rows are zero-filled */
  int32_t width_dwords;
} GsrColumnC;
#define GSR_COMPACT_BLOCK 256             /* source rows per block offset: a consumer ranks inside blocks of this size */
size_t gsr_compact_workspace_bytes(int64_t N);
/* keep_mask [N] bytes.  block_offsets_out [ceil(N/256)] = kept rows before each block of 256 source rows;
 * kept_total_dev = number of kept rows (read it back to size the destination columns). */
int gsr_compact_offsets(const uint8_t* keep_mask, int64_t N, uint32_t* block_offsets_out, uint32_t* kept_total_dev,
                        void* workspace, size_t workspace_bytes, void* stream);
/* One launch moves every column: kept rows to dst[0, kept), tail rows (or zeros) to dst[kept, kept + n_tail). */
int gsr_compact_columns(const uint8_t* keep_mask, int64_t N, const uint32_t* block_offsets, int64_t kept_total,
                        int64_t n_tail, const GsrColumnC* columns_host, int32_t n_columns, void* stream);

/* PointState.add_rendering (splat_trainer/controller/point_state.py:34-50) for one camera, fused: for every row m of
 * the camera's list, with i = idx[m]:  max_scale_px[i] = max(., max over the scale_cols (1 or 2) columns of
 * screen_scale[m]);  points_in_view[i] += visibility[m] > 0;  visibility[i] += visibility[m];
 * split_score[i] = exp_lerp(split_alpha, ., split_score[m]);  prune_cost[i] = exp_lerp(prune_alpha, ., prune_cost[m]).
 * idx rows are unique (one camera; NULL = rows are the points 0..M-1); the state arrays have N entries (points_in_view
 * int16).  Each input group is optional: a NULL screen_scale / visibility / split_score / prune_cost leaves the
 * corresponding state untouched (the data-parallel exchange replays only the two EMAs per camera and reduces the rest).
 * visible_sum (may be NULL): a second N-sized accumulator that also receives += visibility on the same rows -- the
 * scene's own `visible` statistic (mlp_scene.py:244), so that it does not cost an index_add launch of its own. */
int gsr_point_state_add(const int64_t* idx, const float* screen_scale, int32_t scale_cols, const float* visibility,
                        const float* split_score, const float* prune_cost, int64_t M, float split_alpha,
                        float prune_alpha, float* state_prune_cost, float* state_split_score, float* state_max_scale_px,
                        int16_t* state_points_in_view, float* state_visibility, float* visible_sum, void* stream);

/* The reference's per-camera loss mix (trainer.py:448-488 without reg_loss) behind one call per direction:
 *   loss = w_l1 mean|x - t| + w_mse mean (x - t)^2 + w_ssim / levels * sum_l (1 - ssim_valid(pool^l x, pool^l t)),
 * x = clamp(image, lo, hi), pool = 2 x 2 average pooling (floor sizes), image / target [H, W, C] contiguous, C <= 4,
 * levels 1..4 (the coarsest level must be more than 10 pixels per side).  metrics_out (device floats): [loss, l1, mse,
 * ssim_0 .. ssim_{levels-1}].  The workspace carries the forward pass's state to gsr_msloss_backward, which writes
 * d_image = grad_scale_dev[0] * d loss / d image (zero where the clamp is active). */
size_t gsr_msloss_workspace_bytes(int32_t H, int32_t W, int32_t C, int32_t levels);
int gsr_msloss_forward(const float* image, const float* target, int32_t H, int32_t W, int32_t C, int32_t levels,
                       float w_l1, float w_mse, float w_ssim, float lo, float hi, float* metrics_out, void* workspace,
                       size_t workspace_bytes, void* stream);
int gsr_msloss_backward(const float* image, const float* target, int32_t H, int32_t W, int32_t C, int32_t levels,
                        float w_l1, float w_mse, float w_ssim, float lo, float hi, const float* grad_scale_dev,
                        void* workspace, size_t workspace_bytes, float* d_image, void* stream);

/* ---- bilateral-grid colour correction (color_corrector/bilateral_corrector.py) ----------------------------- */
/* grids [N, 12, L, GH, GW] float32 contiguous, one grid per image, 2 <= L, GH, GW <= 64; rgb, out, d_out, d_rgb
 * [H, W, 3] float32 contiguous, 1 <= H, W <= GSR_BILAGRID_MAX_SIDE.  Image k samples grid k trilinearly at
 * x = (j + 0.5) / W (GW - 1), y = (i + 0.5) / H (GH - 1), z = clamp(luma(rgb) (L - 1), 0, L - 1) (grid_sample,
 * align_corners, border padding) and applies the sampled 3x4 affine to rgb.
 * gsr_bilagrid_slice_backward writes d_rgb (NULL: skipped) and slice k of d_grids (NULL: skipped; the other slices are
 * left alone); the grid gradient needs gsr_bilagrid_workspace_bytes of workspace.  gsr_bilagrid_tv writes
 * tv_out[0] = weight * tv, tv = (1/N) sum_axes sum (G shifted - G)^2 / (12 L GH GW), and (d_grids not NULL) weight * dtv/dG,
 * added to d_grids when accumulate != 0.  No float atomics: every result is bit-reproducible. */
#define GSR_BILAGRID_MAX_SIDE 32768
size_t gsr_bilagrid_workspace_bytes(int32_t L, int32_t GH, int32_t GW);
int gsr_bilagrid_slice_forward(const float* grids, int64_t N, int32_t L, int32_t GH, int32_t GW, int64_t k,
                               const float* rgb, int32_t H, int32_t W, float* out, void* stream);
int gsr_bilagrid_slice_backward(const float* grids, int64_t N, int32_t L, int32_t GH, int32_t GW, int64_t k,
                                const float* rgb, int32_t H, int32_t W, const float* d_out, float* d_rgb, float* d_grids,
                                void* workspace, size_t workspace_bytes, void* stream);
int gsr_bilagrid_tv(const float* grids, int64_t N, int32_t L, int32_t GH, int32_t GW, float weight, float* tv_out,
                    float* d_grids, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ---- neighbour searches over 3-D points (gaussians/loading.py estimate_scale, visibility/cluster.py k-means) ------
 * points / x [N, 3] and centroids [K, 3] float32 contiguous, 1 <= N, K <= GSR_NEIGHBOURS_MAX_N.  Squared distance
 * d = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), dx = q.x - c.x, ...  Brute force (every pair), no float atomics: every result
 * is bit-reproducible.
 * gsr_knn: for each i the k (1 <= k <= GSR_KNN_MAX_K, N >= k + 1) smallest distances over j != i, ascending, equal
 *   distances by lower j: dist2_out [N, k], idx_out [N, k] int64; scale_out [N] (may be NULL) = the mean of sqrt(dist2)
 *   over the k, summed in ascending order.  NaN distances never enter a list.  Workspace: gsr_knn_workspace_bytes.
 * gsr_assign_clusters: labels_out [N] int64 = argmin_j d(x_i, c_j), ties to the lowest j, all-NaN distances to 0.
 * gsr_kmeans_iter: `iters` (>= 1) Lloyd iterations enqueued at once: assign, then every centroid with at least one point
 *   becomes the float32 mean of its points (sums in a fixed order; an empty cluster keeps its centroid).  centroids is
 *   updated in place; labels_out receives the LAST assignment, made before the last update.  Workspace:
 *   gsr_kmeans_workspace_bytes. */
#define GSR_KNN_MAX_K 16
#define GSR_NEIGHBOURS_MAX_N 0x7FFFFFFF
size_t gsr_knn_workspace_bytes(int64_t N, int32_t k);
int gsr_knn(const float* points, int64_t N, int32_t k, float* dist2_out, int64_t* idx_out, float* scale_out,
            void* workspace, size_t workspace_bytes, void* stream);
int gsr_assign_clusters(const float* x, int64_t N, const float* centroids, int64_t K, int64_t* labels_out, void* stream);
size_t gsr_kmeans_workspace_bytes(int64_t N, int64_t K);
int gsr_kmeans_iter(const float* x, int64_t N, float* centroids, int64_t K, int32_t iters, int64_t* labels_out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- frustum point queries and view features (visibility/query_points.py, visibility/cluster.py PointClusters) ------
 * gsr_frustum_counts: points [N, 3] float32 against V camera records [V, 16] float32 (rows 0..2 of image_t_world =
 *   expand_proj(K) @ camera_t_world, row-major, then w, h, near, far).  With h_r = fmaf(M[r][2], z, fmaf(M[r][1], y,
 *   fmaf(M[r][0], x, M[r][3]))) and d = h_2 a point is inside a camera when h_0 >= 0 && h_0 < w d && h_1 >= 0 &&
 *   h_1 < h d && d > near && d < min(far, depth_below) (depth_below: +inf when unused).  point_counts_out [N] int32 =
 *   cameras that see point i, camera_counts_out [V] int32 = points camera c sees; either may be NULL, not both.  Exact.
 *   1 <= N <= GSR_NEIGHBOURS_MAX_N, 1 <= V <= GSR_VISIBILITY_MAX_CAMERAS.
 * gsr_view_features: features_out [K] float32 = per cluster the sum of vis[j] over the listed points idx[j] of that
 *   cluster with vis[j] > threshold (strict), in a fixed order: a function of the SET of (idx, vis) pairs, bit-reproducible.
 *   point_idx [M] int64 holds DISTINCT indices in [0, N) (an index outside the range is skipped; duplicates are not
 *   supported: the last writer wins); M may be 0.  sorted_labels / sorted_points [N] uint32: the points in stable label
 *   order (gsr_sort_pairs_u32 of (label, point index)); cluster_range [K, 2] uint32 from gsr_tile_ranges.
 *   dense_scratch [N] and slot_scratch [N] float32 are the caller's, reused by every call (the call zero-fills the first).
 *   point_visible [N] int32 (may be NULL) is incremented at every listed index. */
#define GSR_VISIBILITY_MAX_CAMERAS 65536
int gsr_frustum_counts(const float* points, int64_t N, const float* records, int64_t V, float depth_below,
                       int32_t* point_counts_out, int32_t* camera_counts_out, void* stream);
int gsr_view_features(const int64_t* point_idx, const float* point_vis, int64_t M, float threshold,
                      const uint32_t* sorted_labels, const uint32_t* sorted_points, const uint32_t* cluster_range,
                      int64_t N, int64_t K, float* dense_scratch, float* slot_scratch, float* features_out,
                      int32_t* point_visible, void* stream);

/* ---- 3-D smoothing filter (Mip-Splatting, Yu et al. CVPR 2024, section 5.1; no reference counterpart) ---------------
 * gsr_sampling_rate: rate_out [N] float32 = max over the cameras that sample point i of focal[c] / d, 0 when none does.
 *   points [N, 3], records [V, 16] and h_r, d as for gsr_frustum_counts; focal [V] float32, the camera's max(fx, fy) in
 *   pixels; margin >= 0 a fraction of the image: camera c samples a point when h_0 >= (-margin w) d && h_0 < (w + margin w) d
 *   && h_1 >= (-margin h) d && h_1 < (h + margin h) d && d > near && d < far.  One lane owns its points and walks the
 *   cameras in ascending order, no atomics: a function of the inputs alone.  1 <= N <= GSR_NEIGHBOURS_MAX_N,
 *   1 <= V <= GSR_VISIBILITY_MAX_CAMERAS.
 * gsr_filter3d_forward: per row, c = strength / rate^2 (0 when rate is not > 0, strength >= 0) is added to the variance of
 *   every axis and the opacity is scaled by prod_j sigma_j / sigma'_j: u_j = c exp(-2 ls_j), ls'_j = ls_j + log1p(u_j) / 2,
 *   lc = -sum_j log1p(u_j) / 2, a' = log sigmoid(a) + lc - log(sigmoid(-a) + sigmoid(a) (-expm1(lc))).  A row with c == 0
 *   is copied: its output bits are its input bits.  log_scaling / out_log_scaling [N, 3], alpha_logit / out_alpha_logit
 *   and rate [N], float32 contiguous and 16-byte aligned (rows travel four at a time); outputs distinct from inputs.
 * gsr_filter3d_backward recomputes the forward's terms (nothing is saved) and writes d_log_scaling [N, 3] and
 *   d_alpha_logit [N] from the gradients of the two outputs (overwritten, not added); a row with c == 0 passes its
 *   incoming gradients through bit for bit.  The rate receives no gradient.  Same layout and alignment. */
int gsr_sampling_rate(const float* points, int64_t N, const float* records, const float* focal, int64_t V, float margin,
                      float* rate_out, void* stream);
int gsr_filter3d_forward(const float* log_scaling, const float* alpha_logit, const float* rate, int64_t N, float strength,
                         float* out_log_scaling, float* out_alpha_logit, void* stream);
int gsr_filter3d_backward(const float* log_scaling, const float* alpha_logit, const float* rate, int64_t N, float strength,
                          const float* d_out_log_scaling, const float* d_out_alpha_logit, float* d_log_scaling,
                          float* d_alpha_logit, void* stream);

/* ---- MCMC controller: position noise (controller/mcmc_controller.py:93-100, made to reach the scene) --------------------
 * gsr_mcmc_noise, in place on position [N, 3]; log_scaling [N, 3], rotation_xyzw [N, 4], alpha_logit [N] float32 and
 *   points_in_view [N] int16, contiguous.  Row i with points_in_view[i] > min_views:  o = sigmoid(alpha_logit[i]), h = opacity_threshold / 2,
 *   level = sigmoid(-(o - h) margin / h) noise_level (soft_lt(o, h, margin) of util/misc.py), sigma_j =
 *   max(exp(log_scaling[i][j]), scale_eps);  position[i] += R(q / max(|q|, 1e-12)) (sigma * (xi level)) with xi the first
 *   three of the four normals that Box-Muller makes of the Philox4x32-10 words at key (seed lo, seed hi), counter
 *   (i lo, i hi, step lo, step hi): u = ((w >> 8) + 0.5) 2^-24 per word, sqrt(-2 ln u_a) (cos, sin)(2 pi u_b) on the pairs
 *   (0, 1) and (2, 3).  A row with too few views, or whose level max_j sigma_j is 0 in float32, is neither read beyond
 *   points_in_view and alpha_logit nor written.  No atomics, no generator state: row i depends on its own inputs, seed,
 *   step and i alone.  0 <= N <= GSR_NEIGHBOURS_MAX_N (0: nothing is launched), opacity_threshold > 0, margin,
 *   noise_level and scale_eps >= 0.
 * gsr_mcmc_draws: the words [N, 4] uint32 (16-byte aligned) and the three normals [N, 3] float32 of rows 0..N-1 from the
 *   same device functions; either may be NULL. */
int gsr_mcmc_noise(float* position, const float* log_scaling, const float* rotation_xyzw, const float* alpha_logit,
                   const int16_t* points_in_view, int64_t N, int32_t min_views, float opacity_threshold, float margin,
                   float noise_level, float scale_eps, uint64_t seed, uint64_t step, void* stream);
int gsr_mcmc_draws(int64_t N, uint64_t seed, uint64_t step, uint32_t* words_out, float* normals_out, void* stream);

/* ---- MCMC relocation (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", 2024; no reference
 *      counterpart; csrc/relocate.hip) -------------------------------------------------------------------------------
 * Dead Gaussians are moved onto live ones drawn with probability proportional to opacity, and the opacity and scale of a
 * source and its copies are corrected so that the rendered distribution stays (Eq. 9).  csrc/gsr_relocate.h is the one
 * statement of the arithmetic, shared with the host shim.  Every call is enqueued on the stream without a host wait.
 *
 * gsr_weighted_draws (integers only).  weights [N] uint32, 0 = cannot be drawn; P_i the inclusive prefix sum of the
 *   weights in uint64, S = P_{N-1} (0 for N == 0).  Draw k = 0..n-1 takes the Philox4x32-10 words at key (seed lo, seed hi),
 *   counter (k lo, k hi, step lo, (step hi & 0x00FFFFFF) | domain << 24) -- gsr_mcmc_noise's counter is domain 0 for every
 *   step below 2^56, relocation uses 1 and growth 2, so the streams of one seed never share a counter --,
 *   r = word0 2^32 + word1, t = floor(r S / 2^64) (the high half of the 128-bit product), and
 *   sources_out[k] = the smallest i with P_i > t.  counts_out [N] int32 is zero-filled by the call and then
 *   counts_out[i] = the number of draws that gave i (integer atomics: order cannot change the result);
 *   total_out[0] = S, a device uint64.  S == 0: every source is -1, every count 0, GSR_OK.  The result is a function of
 *   (weights, seed, step, domain, k) alone -- not of n, of the launch shape or of the device -- and equals an integer
 *   oracle bit for bit.  t takes every value of [0, S) floor(2^64 / S) or one more time: a weight's share of the draws is
 *   off by at most S / 2^64 of itself, below 2^-18 at 3 M rows of weight 2^24.  S < 2^56 is the caller's to keep (any
 *   weights of gsr_relocate_weights do).  weights and counts_out 16-byte aligned; workspace (16-byte aligned) of
 *   gsr_weighted_draws_workspace_bytes(N): one uint64 per 256 rows, the prefix at the end of each block of rows.
 *   Checked in this order: N, n outside [0, GSR_NEIGHBOURS_MAX_N] or domain outside [0, 255] GSR_ERR_INVALID_ARGUMENT; a
 *   NULL total_out, a NULL weights or counts_out with N > 0, a NULL sources_out with n > 0, or weights / counts_out not
 *   16-byte aligned GSR_ERR_INVALID_ARGUMENT; a NULL or short workspace GSR_ERR_WORKSPACE_TOO_SMALL; a workspace not
 *   16-byte aligned GSR_ERR_INVALID_ARGUMENT.
 * gsr_relocate_weights: weights_out[i] = 0 where alive[i] == 0 (alive [N] bytes; NULL: every row is alive), else
 *   max(1, floor(2^24 sigmoid(alpha_logit[i]))), the sigmoid in fp64 from the float32 logit (a NaN logit gives 1).  Device
 *   and host libm differ in the last bits of exp: within 1 of an exact oracle.  0 <= N <= GSR_NEIGHBOURS_MAX_N (0: GSR_OK,
 *   no launch, before any pointer is looked at).
 * gsr_relocate_rescale, in place on alpha_logit [N] and log_scaling [N, 3] float32.  A row with counts[i] = c >= 1 is the
 *   source of c copies; a row with c <= 0 is neither read beyond its count nor written.  n = min(c + 1, 51),
 *   o = sigmoid(a), o' = 1 - (1 - o)^(1/n), D = sum_{k=0..n-1} C(n, k+1) (-1)^k o'^(k+1) / sqrt(k+1), coeff = o / D, in fp64;
 *   alpha_logit <- float32(logit(clamp(o', o_floor, 1 - 2^-24))), log_scaling_j <- float32(double(log_scaling_j) +
 *   log(coeff)).  The coefficient uses the unclamped o'.  0 < o_floor < 1; N as above (0: GSR_OK before the pointers).
 * gsr_relocate_rows: one launch over n_columns <= GSR_MAX_COLUMNS columns of N rows.  For k < n, row dst_rows[k] of every
 *   column with zero == 0 takes row src_rows[k]; rows dst_rows[k] and src_rows[k] of every column with zero != 0 are
 *   zero-filled.  PRECONDITION: the dst rows are unique and disjoint from the src rows; then the result does not depend
 *   on order.  A k whose dst or src index lies outside [0, N) (the -1 of S == 0 included) is skipped.  data 4-byte aligned;
 *   a column whose width and address allow it moves 16 or 8 bytes at a time.  Checked in this order: a negative or too
 *   large n, N or n_columns GSR_ERR_INVALID_ARGUMENT; n, N or n_columns == 0 GSR_OK; a NULL dst_rows, src_rows or
 *   columns_host, or a column with NULL or misaligned data or width_dwords outside [1, 2^20], GSR_ERR_INVALID_ARGUMENT. */
typedef struct GsrRowColumnC {
  void* data;            /* [N, width] 4-byte words, moved in place */
  int32_t width_dwords;
  int32_t zero;          /* 0: row dst takes row src; otherwise both rows are zero-filled */
} GsrRowColumnC;
size_t gsr_weighted_draws_workspace_bytes(int64_t N);
int gsr_weighted_draws(const uint32_t* weights, int64_t N, int64_t n, uint64_t seed, uint64_t step, int32_t domain,
                       int32_t* sources_out, int32_t* counts_out, uint64_t* total_out, void* workspace,
                       size_t workspace_bytes, void* stream);
int gsr_relocate_weights(const float* alpha_logit, const uint8_t* alive, int64_t N, uint32_t* weights_out, void* stream);
int gsr_relocate_rescale(float* alpha_logit, float* log_scaling, const int32_t* counts, int64_t N, float o_floor,
                         void* stream);
int gsr_relocate_rows(const int32_t* dst_rows, const int32_t* src_rows, int64_t n, int64_t N,
                      const GsrRowColumnC* columns_host, int32_t n_columns, void* stream);

/* ---- SH export fit: per-point least squares of SH coefficients to view-dependent colours (no reference counterpart) ----
 * One row of gsr_sh_fit_row_doubles(K) = K (K + 1) / 2 + 3 K + 1 doubles per point (0 for a K outside {1, 4, 9, 16}): the
 * lower triangle of G = sum w Y Y^T, b_c = sum w Y (y_c - 0.5) channel-major, W = sum w, with Y the basis of gsr_sh_forward
 * at normalize(position - camera_pos) in float32 and every product and sum after it fp64 (csrc/gsr_sh_fit.h).
 * gsr_sh_fit_accumulate adds one view: positions [N, 3], indexes [M] int64 DISTINCT indices in [0, N) (an index outside
 *   the range is skipped; duplicates are not detected and lose updates), colors [M, 3] and weights [M] >= 0 float32,
 *   camera_pos [3] float32 on the device, acc [N, row doubles] fp64.  Only the listed rows are read and written, without
 *   atomics: calls on one stream add their views in order, bit-reproducibly.  1 <= M <= N <= GSR_NEIGHBOURS_MAX_N.
 * gsr_sh_fit_solve: (G + ridge W Y0^2 diag(0, 1, ..., 1)) s_c = b_c per point by fp64 Cholesky, Y0 the constant basis
 *   term; sh_out [N, 3, K] and weight_out [N] = W, float32.  A row with W == 0 gives zeros.  ridge >= 1e-6, finite. */
int gsr_sh_fit_row_doubles(int32_t K);
int gsr_sh_fit_accumulate(const float* positions, int64_t N, const int64_t* indexes, int64_t M, const float* colors,
                          const float* weights, const float* camera_pos, int32_t K, double* acc, void* stream);
int gsr_sh_fit_solve(const double* acc, int64_t N, int32_t K, float ridge, float* sh_out, float* weight_out, void* stream);

/* ---- neural colour model (scene/color_model.py ColorModel, scene/mlp/torch_mlp.py MLP / AffineMLP) ----------
 * Per row: x = LayerNorm_F([point_features, glo]) (no affine, eps 1e-5); diffuse = lum(base(x), 0); d = normalize(
 * position - cam_pos) (eps 1e-12); [a, b] = encode(rsh_S(d)); specular = lum(dir(x a + b), -2), lum(o, c)_k =
 * sigmoid(o_{k+1}) exp(o_0 + c).  base and dir are GLU-MLPs (L hidden layers Linear(in, 2H) -> a sigmoid(b), then
 * Linear(H, 4)).  Every Linear rounds its input and weight to f16 once and adds the fp32 bias to fp32 products.
 * Parameters (fp32, row-major [out, in]) by index: 0 base.layers.0.m, 1 base.layers.1.m (L = 2), 2 base.layers.L,
 * 3 directional_model.encode_dir.mlp.layers.0 [2F, (S+1)^2], 4 directional_model.mlp.layers.0.m, 5 ... .layers.1.m
 * (L = 2), 6 directional_model.mlp.layers.L; unused entries NULL.  Supported: H = 32, L in {1, 2}, S in 2..5,
 * 1 <= F = P + G <= 64, color_channels = 3 (anything else: GSR_ERR_UNSUPPORTED).
 * point_features [M, P], positions [M, 3], diffuse_out / specular_out / d_diffuse / d_specular / d_point_features
 * [M, 3] or [M, P]; cam_pos [3]; glo_feature [G]; all float32 contiguous.  Both calls first pack the parameters into
 * the workspace (one launch), so they may change between calls.  gsr_color_backward recomputes the forward; d_diffuse
 * or d_specular may be NULL (zero); it writes d_point_features and every gradient of `grads` (overwritten, not added);
 * d_cam_pos NULL skips the camera path.  The workspace holds one gradient slot per workgroup, the grid depends on M
 * only and there are no float atomics: every result is bit-reproducible. */
typedef struct GsrColorModel {
  int32_t P, G, H, L, S, color_channels;
  const float* weight[7];
  const float* bias[7];
} GsrColorModel;
typedef struct GsrColorGrads {
  float* d_weight[7];
  float* d_bias[7];
  float* d_glo;       /* [G] */
  float* d_cam_pos;   /* [3] or NULL */
} GsrColorGrads;
/* sizeof GsrColorModel (0), GsrColorGrads (1), -1 otherwise */
int64_t gsr_color_struct_bytes(int32_t which);
int gsr_color_supported(const GsrColorModel* model);
size_t gsr_color_forward_workspace_bytes(const GsrColorModel* model);
size_t gsr_color_backward_workspace_bytes(const GsrColorModel* model, int64_t M);
int gsr_color_forward(const GsrColorModel* model, const float* point_features, const float* positions,
                      const float* cam_pos, const float* glo_feature, int64_t M, float* diffuse_out, float* specular_out,
                      void* workspace, size_t workspace_bytes, void* stream);
int gsr_color_backward(const GsrColorModel* model, const float* point_features, const float* positions,
                       const float* cam_pos, const float* glo_feature, int64_t M, const float* d_diffuse,
                       const float* d_specular, float* d_point_features, const GsrColorGrads* grads, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- scene regulariser and post-step projection (scene/mlp_scene.py:246-288 compute_reg / reg_loss, :236-237) ----
 * Per row i of the M culled points, j = idx[i]: s = exp(log_scaling[j]); norm = (s . s) / depths[i]^2; aspect =
 * max(s) / min(s); op = (1 - exp(-4 opacity[i]))^2 norm; spec = sum_k |specular[i,k]| (0 when specular is NULL);
 * w = visibility[i] when visibility_weighted, else 1.  The four terms scale, opacity, aspect, specular are the means of
 * {norm, op, aspect, spec} w over the rows with visibility[i] > 0 (the mask is applied in the kernel over all M rows and
 * the count stays on the device; no such row: every term 0); loss = sum_k weight[k] term[k], a zero weight dropping
 * its term.  gsr_reg_forward writes loss_out[0] and terms_out[5] = the four unweighted terms and the count; fixed-order
 * sums, no float atomics: bit-reproducible.  gsr_reg_backward takes the forward's terms and the device scalar d_loss,
 * writes d_opacity [M], d_depths [M], d_specular [M,3] for every row (zero where masked; each may be NULL) and ADDS the
 * log_scaling term into rows idx[i] of d_log_scaling [N,3] (may be NULL; the rows of idx are unique).  visibility is a
 * constant.  M = 0 is valid (loss 0).
 * gsr_scene_post_step, in place over N rows: rotation_xyzw[i] /= max(|rotation_xyzw[i]|, eps) (16-byte aligned) and
 * log_scaling[i] = clamp(log_scaling[i], lo, hi). */
typedef struct GsrReg {
  const int64_t* idx;          /* [M] */
  const float* log_scaling;    /* [N, 3] */
  const float* depths;         /* [M] */
  const float* opacity;        /* [M] */
  const float* specular;       /* [M, 3] or NULL */
  const float* visibility;     /* [M] */
  int64_t M, N;
  float weight[4];             /* scale, opacity, aspect, specular */
  int32_t visibility_weighted;
} GsrReg;
int64_t gsr_reg_struct_bytes(void);
size_t gsr_reg_workspace_bytes(int64_t M);
int gsr_reg_forward(const GsrReg* args, float* loss_out, float* terms_out, void* workspace, size_t workspace_bytes,
                    void* stream);
int gsr_reg_backward(const GsrReg* args, const float* terms, const float* d_loss, float* d_opacity, float* d_depths,
                     float* d_specular, float* d_log_scaling, void* stream);
int gsr_scene_post_step(float* rotation_xyzw, float* log_scaling, int64_t N, float eps, float lo, float hi, void* stream);

/* ---- evaluation pass (trainer/evaluation.py Evaluation, util/colors.py fit_colors_batch) --------------------------
 * gsr_color_fit: out [P, 3] = the iterative affine-quadratic colour fit of image [P, 3] to ref [P, 3] (float32,
 * contiguous, out distinct from both).  Design row a = [r^2, rg, rb, g^2, gb, b^2, r, g, b, 1]; iteration k solves, per
 * channel c, min_w sum_p m_c (a . w - ref_c)^2 over the pixels with image_c, iterate_c and ref_c all in [eps, 1 - eps]
 * (compared in float32), from 45 fp64 sums (the normal equations), and the next iterate is clip(a . W, 0, 1) rounded to
 * float32.  The solve scales to unit diagonal, takes the symmetric eigendecomposition and drops eigenvalues <= 1e-9 of
 * the largest: a rank-deficient system (a grey image, a constant channel) gets its minimum-norm solution, no unmasked
 * pixel gives w = 0.  num_iters in 0..64 (0 copies), eps in [0, 0.5).  num_iters + 1 passes and num_iters one-block
 * solves, all on the device; fixed-order sums, no atomics: bit-reproducible.
 * gsr_image_metrics: metrics_out[0..2] (device floats, e.g. a row of a table) = mean squared error, mean absolute error
 * (no clamp) and mean SSIM with valid padding of image against source, both [H, W, 3] float32 contiguous and 16-byte
 * aligned, H and W > 10. */
size_t gsr_color_fit_workspace_bytes(int64_t P);
int gsr_color_fit(const float* image, const float* ref, int64_t P, int32_t num_iters, float eps, float* out,
                  void* workspace, size_t workspace_bytes, void* stream);
size_t gsr_image_metrics_workspace_bytes(int32_t H, int32_t W);
int gsr_image_metrics(const float* image, const float* source, int32_t H, int32_t W, float* metrics_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- pose tables (camera_table/pose_table.py PoseTable, RigPoseTable) ------------------------------------------------
 * A table is q [A, 4] (XYZW, not necessarily unit) and t [A, 3], float32 contiguous.  gsr_pose_forward writes, for image
 * b of B, T_out[b] (4x4 row-major, T_out 16-byte aligned) = pose(left[idx_left[b]]) when the right table is absent
 * (q_right, t_right, idx_right all NULL) and pose(left[idx_left[b]]) pose(right[idx_right[b]]) otherwise (a rig: left =
 * camera_t_rig, right = rig_t_world), with pose(q, t) = [R(q / max(|q|, 1e-12)) t; 0 0 0 1].  One launch; B = 0 returns
 * GSR_OK without one.  gsr_pose_backward takes d_T [B, 4, 4] (row 3 ignored) and writes d_q [A, 4], d_t [A, 3] of each
 * table whose pair of outputs is given (a pair may be NULL; not both): every row, zeros for a row no image selects, and
 * for a selected row the sum over its images in increasing b, chained through the rotation and the normalisation.  One
 * launch, no float atomics: bit-reproducible.  The order of every operation is in csrc/gsr_camera_table.h.
 * An index outside [0, A) is no fault: it reads row 0, and the kernel ORs 1 into status[0] (device int32, the caller
 * zeroes it once and reads it when it chooses to wait).  A and B at most GSR_POSE_MAX_ROWS.
 * gsr_pose_block_size: the threads per block of both launches. */
#define GSR_POSE_MAX_ROWS 16777216
int gsr_pose_forward(const float* q_left, const float* t_left, int64_t A_left, const int64_t* idx_left,
                     const float* q_right, const float* t_right, int64_t A_right, const int64_t* idx_right, int64_t B,
                     float* T_out, int32_t* status, void* stream);
int gsr_pose_backward(const float* q_left, const float* t_left, int64_t A_left, const int64_t* idx_left,
                      const float* q_right, const float* t_right, int64_t A_right, const int64_t* idx_right, int64_t B,
                      const float* d_T, float* d_q_left, float* d_t_left, float* d_q_right, float* d_t_right,
                      int32_t* status, void* stream);
int gsr_pose_block_size(void);

/* ---- histograms of the detailed training logs (logger/histogram.py Histogram, scene/mlp_scene.py log_gradients,
 * hist_log_nonzero, controller/point_state.py log_histograms) -------------------------------------------------------
 * gsr_histogram bins the entries of values [N, C] (float32, contiguous) in one sweep.  rows [M] int64 (NULL: all N rows,
 * M ignored) gathers rows, repeats and any order allowed; an index outside [0, N) is never read and its C entries count
 * as non-finite.  weight [N] float32 (NULL: none) divides: the entry of row r is x = v / (eps + weight[r]), r the index
 * into values.  mode 0: t = x.  mode 1: t = log10(x) for x > min_value, every other x is dropped.  mode 2:
 * t = log10(max(x, min_value)).  An entry is kept when it passes the mode's threshold and both x and t are finite; the
 * non-finite ones are counted apart.
 * Range: auto_range = 0 takes (lo, hi), finite with hi >= lo; auto_range != 0 ignores them and a first pass takes lo and
 * hi as the minimum and maximum of the kept t (integer atomics on ordered keys: exact, order-independent); the binning
 * pass reads them on the device, so the call never waits for the host, and its results equal, bit for bit, those of the
 * fixed-range call with the (lo, hi) it reports in stats[3], stats[4].
 * Bin (float32, no contraction; csrc/gsr_histogram.h is the one statement of it, shared with the host shim):
 * p = (t - lo) * (num_bins / (hi - lo)), b = floor(p); t == hi takes the last bin; hi == lo puts every kept entry in bin
 * 0; a b outside [0, num_bins) is "outside": left out with trim != 0, clamped in with trim == 0.
 * Outputs: counts [num_bins] int64 and stats [8] double, both device memory, both overwritten: 0 kept entries, 1 sum of t
 * and 2 sum of t^2 over the BINNED entries (the kept ones less, with trim, the outside ones: what counts holds), 3 minimum
 * and 4 maximum of the kept t (0 when nothing was kept), 5 dropped by the threshold, 6 non-finite, 7 outside.
 * Counts and tallies are integer atomics (LDS counters per wave, then one global add per bin and block, spread over 16
 * sets of words in the workspace that a last pass adds up), the two sums fp64 partials per block added in a fixed order;
 * no float atomics: every output is the same bits on every run.
 * num_bins in 1..GSR_HISTOGRAM_MAX_BINS.  N == 0 or (rows and M == 0) launches nothing and leaves zeros.  workspace: device
 * memory, 16-byte aligned, gsr_histogram_workspace_bytes() bytes, not shared between calls in flight on two streams. */
#define GSR_HISTOGRAM_MAX_BINS 1024
size_t gsr_histogram_workspace_bytes(void);
int gsr_histogram(const float* values, int64_t N, int64_t C, const int64_t* rows, int64_t M, const float* weight,
                  float eps, int32_t mode, float min_value, float lo, float hi, int32_t num_bins, int32_t auto_range,
                  int32_t trim, int64_t* counts, double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- area resize of uint8 images (the loader's cv2.resize(..., INTER_AREA); csrc/image.hip) ------------- */
/* src (B, Hs, Ws, C) -> dst (B, Hd, Wd, C), both contiguous with interleaved channels, C in {1, 3}, Hd <= Hs, Wd <= Ws.
 * The exact area mean in integers (csrc/gsr_image.h is the one statement of the arithmetic, shared with the host shim):
 * on an axis of Ws Wd units source pixel i covers [i Wd, (i + 1) Wd) and destination pixel j covers [j Ws, (j + 1) Ws);
 * wx(j, i) is the length of their overlap, wy likewise, S = sum_y sum_x wy wx src, D = Ws Hs and
 * out = floor((2 S + D) / (2 D)): round half up.  No floating point: the result is a function of the input alone, the
 * same bits on every run.  Equal sizes give a copy.
 * Checked before any HIP call, in this order: a negative size is GSR_ERR_INVALID_ARGUMENT; C outside {1, 3}, or Ws or Hs
 * above 32768, GSR_ERR_UNSUPPORTED; Wd > Ws, Hd > Hs (upscaling is left to the caller) or a zero destination size with a
 * non-zero source GSR_ERR_INVALID_ARGUMENT; B == 0 or an empty image is GSR_OK with no launch and dst untouched; a NULL
 * src or dst, looked at last, GSR_ERR_INVALID_ARGUMENT.  Neither pointer needs any alignment. */
int gsr_image_resize_area_u8(const uint8_t* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, uint8_t* dst, int32_t Hd,
                             int32_t Wd, void* stream);

/* ---- lens undistortion (the scan loader's cv2.undistort; csrc/undistort.hip) ---------------------------- */
/* Two calls: the map of a distorted camera onto a pinhole target, once per camera, and the bilinear remap of images
 * through a map.  csrc/gsr_undistort.h is the one statement of the arithmetic of both, shared with the host shim.
 * Pixel centres sit at integer coordinates (OpenCV's convention; COLMAP's are half a pixel further).
 *
 * gsr_undistort_map.  source_host [9] = fx fy cx cy k1 k2 p1 p2 k3 (OpenCV's five-coefficient model) and target_host [4]
 * = fx' fy' cx' cy' are HOST memory, read before the call returns.  map_out [Hd, Wd, 2] int32, device memory, 8-byte
 * aligned: for destination pixel (u, v) the source position (X, Y) in units of 1/32 pixel.  In fp64, every product and
 * sum rounded on its own, in this order (ifx' = 1 / fx', ify' = 1 / fy' formed once on the host):
 *   x = (u - cx') * ifx'            y = (v - cy') * ify'
 *   xx = x*x   yy = y*y   xy = x*y   r2 = xx + yy
 *   t = r2*k3; t = k2 + t; t = r2*t; t = k1 + t; t = r2*t; rad = 1 + t
 *   a = (2*p1)*xy; b = 2*xx; b = r2 + b; b = p2*b; dx = a + b
 *   a = 2*yy; a = r2 + a; a = p1*a; b = (2*p2)*xy; dy = a + b
 *   xd = x*rad; xd = xd + dx        yd = y*rad; yd = yd + dy
 *   xs = fx*xd; xs = xs + cx        ys = fy*yd; ys = ys + cy
 * then xs is clamped to [-1, Ws] and ys to [-1, Hs] (NaN becomes -1) and X = floor(xs*32 + 0.5), Y likewise.
 * Checked before any HIP call, in this order: a negative size is GSR_ERR_INVALID_ARGUMENT; a side above 32768
 * GSR_ERR_UNSUPPORTED; a NULL source_host or target_host, a parameter that is not finite, or fx, fy, fx', fy' not above
 * 0 GSR_ERR_INVALID_ARGUMENT; Hd == 0 or Wd == 0 is GSR_OK with no launch; a NULL map_out, looked at last,
 * GSR_ERR_INVALID_ARGUMENT.
 *
 * gsr_image_remap_u8.  src (B, Hs, Ws, C) -> dst (B, Hd, Wd, C) through map [Hd, Wd, 2] (8-byte aligned), one map for
 * the whole batch; both images contiguous with interleaved channels, C in {1, 3}, no alignment asked of either; src and
 * dst must not overlap (not checked).  An entry (X, Y), any int32, is first clamped to [-32, 32 Ws] x [-32, 32 Hs];
 * x0 = X >> 5 (floor) and ax = X & 31 give the taps x0 with weight 32 - ax and x0 + 1 with weight ax, likewise in y; a
 * tap outside the source, or one of weight 0, contributes 0, and out = (sum of wy wx byte + 512) >> 10.  All integer:
 * the result is a function of the inputs alone, the same bits on every run.  An empty source (Hs == 0 or Ws == 0) has
 * every tap outside: dst is zero-filled.
 * Checked before any HIP call, in this order: a negative size is GSR_ERR_INVALID_ARGUMENT; C outside {1, 3}, or a side
 * above 32768, GSR_ERR_UNSUPPORTED; B == 0, Hd == 0 or Wd == 0 is GSR_OK with no launch and dst untouched; a NULL map or
 * dst, or a NULL src of a source that has pixels, looked at last, GSR_ERR_INVALID_ARGUMENT. */
int gsr_undistort_map(const double* source_host, const double* target_host, int32_t Hs, int32_t Ws, int32_t Hd,
                      int32_t Wd, int32_t* map_out, void* stream);
int gsr_image_remap_u8(const uint8_t* src, int32_t B, int32_t Hs, int32_t Ws, int32_t C, const int32_t* map,
                       uint8_t* dst, int32_t Hd, int32_t Wd, void* stream);

/* ---- depth-map fusion (no reference counterpart): multi-view consistency, point emission, voxel-grid mean -------
 * The arithmetic is csrc/gsr_fusion.h, shared with the host shim: fp64 throughout, every product and sum rounded on its
 * own in the order given here, one IEEE division per projection.  Pixel (row i, column j) has its centre at
 * (j + 0.5, i + 0.5).  A depth is valid when it is above 0 and finite.  Every double travels in a host array (the
 * binding's type rule has no double by value); the arrays are read before the call returns.
 *
 * gsr_fuse_check.  ref_depth [Hr, Wr] float; ref_intrinsics_host [4] = ifx ify cx cy with ifx = 1 / fx, ify = 1 / fy;
 * sources_host [S] name each source's depth map [H, W]; source_params_host [S, 16] = the rows of src_t_ref (3 x 4), then
 * fx fy cx cy of the source; tolerances_host [2] = near, rel_tol; counts [Hr, Wr, 2] uint8 = agree, violate.  Per valid
 * reference pixel of depth d and per source:
 *   x = ((j + 0.5) - cx) ifx, y = ((i + 0.5) - cy) ify, X = x d, Y = y d, Z = d
 *   p_k = ((r_k0 X + r_k1 Y) + r_k2 Z) + t_k;  !(p_2 > near): no vote;  iz = 1 / p_2
 *   us = fx_s (p_0 iz) + cx_s, vs likewise; outside [0, Ws) x [0, Hs) or NaN: no vote; ds = src[floor(vs), floor(us)]
 *   ds not valid: no vote;  tol = rel_tol p_2, diff = ds - p_2: |diff| <= tol agree, else diff > tol violate, else none.
 * The pixel's two counters are read, incremented with saturation at 255 and written once; a pixel without a valid
 * depth keeps its counters.  More than GSR_FUSE_MAX_SOURCES sources are several calls.
 *   Checked in this order: a negative Hr or Wr GSR_ERR_INVALID_ARGUMENT; one above 32768 GSR_ERR_UNSUPPORTED; S outside
 *   [1, GSR_FUSE_MAX_SOURCES], a NULL host array, a host value that is not finite or rel_tol < 0
 *   GSR_ERR_INVALID_ARGUMENT; a source side below 0 GSR_ERR_INVALID_ARGUMENT, above 32768 GSR_ERR_UNSUPPORTED; Hr == 0 or
 *   Wr == 0 GSR_OK; a NULL ref_depth or counts, or a NULL depth of a source that has pixels, GSR_ERR_INVALID_ARGUMENT.
 *
 * gsr_fuse_mask writes keep_out [Hr Wr] bytes: 1 where the depth is valid, agree >= min_agree and violate <=
 * max_violate -- the input of gsr_compact_offsets, whose blocks of GSR_COMPACT_BLOCK pixels the emit kernel ranks inside.  gsr_fuse_emit writes the kept pixels in row-major order: the r-th
 * kept pixel goes to row base + r of points_out [capacity, 3] float, colors_out [capacity, 3] uint8 and agree_out
 * [capacity] uint8; a row at or beyond capacity is not written.  The point is ((w_k0 X + w_k1 Y) + w_k2 Z) + t_k of
 * world_t_ref_host [12] (3 x 4 rows) rounded to float; the colour floor(clamp(c, 0, 1) 255 + 0.5) of image [Hr, Wr, 3]
 * float (NaN -> 0), 255 without an image; agree the pixel's agree count.  block_offsets: what gsr_compact_offsets made of
 * the mask.
 *   Checked in this order: a negative size, base or capacity GSR_ERR_INVALID_ARGUMENT; a side above 32768
 *   GSR_ERR_UNSUPPORTED; min_agree or max_violate outside [0, 255], a NULL or non-finite host array
 *   GSR_ERR_INVALID_ARGUMENT; Hr == 0, Wr == 0 or (emit) base >= capacity GSR_OK; a NULL device pointer other than image
 *   GSR_ERR_INVALID_ARGUMENT.
 *
 * gsr_voxel_downsample.  points [N, 3] float, colors [N, 3] uint8, grid_host [4] = voxel ox oy oz.  Per axis:
 * s = (p - origin) inv with inv = 1 / voxel; q = floor(s) clamped to [-2^20, 2^20 - 1] (NaN -> -2^20); f = s - q clamped
 * to [0, 1] (NaN -> 0); F = floor(f 2^20 + 0.5); key = (qz + 2^20) << 42 | (qy + 2^20) << 21 | (qx + 2^20), 63 bits.  Per occupied
 * voxel of n points, with the int64 sums S = sum F and C = sum of a colour byte: mean = (float)(origin + (q + (S / n)
 * 2^-20) voxel), colour = (2 C + n) / (2 n) in integer division.  points_out [K, 3], colors_out [K, 3], counts_out [K]
 * int32 (capacity N each) in ascending key order, K_dev[0] = K.  The sums are integers: the result does not depend on
 * the order of addition.
 *   Checked in this order: N outside [0, 2^31 - 1], a NULL or non-finite grid_host, voxel not above 0 (or 1 / voxel not
 *   finite) GSR_ERR_INVALID_ARGUMENT; N == 0 GSR_OK before any pointer is looked at (nothing is written, K_dev
 *   included); a NULL array or K_dev GSR_ERR_INVALID_ARGUMENT; a NULL or short workspace (gsr_voxel_workspace_bytes)
 *   GSR_ERR_WORKSPACE_TOO_SMALL. */
#define GSR_FUSE_MAX_SOURCES 16
typedef struct GsrFuseSource {
  const float* depth;    /* [H, W] */
  int32_t H, W;
} GsrFuseSource;
int gsr_fuse_check(const float* ref_depth, int32_t Hr, int32_t Wr, const double* ref_intrinsics_host,
                   const GsrFuseSource* sources_host, const double* source_params_host, int32_t S,
                   const double* tolerances_host, uint8_t* counts, void* stream);
int gsr_fuse_mask(const float* ref_depth, const uint8_t* counts, int32_t Hr, int32_t Wr, int32_t min_agree,
                  int32_t max_violate, uint8_t* keep_out, void* stream);
int gsr_fuse_emit(const float* ref_depth, const uint8_t* counts, const float* image, int32_t Hr, int32_t Wr,
                  const double* ref_intrinsics_host, const double* world_t_ref_host, int32_t min_agree,
                  int32_t max_violate, const uint32_t* block_offsets, int64_t base, int64_t capacity, float* points_out,
                  uint8_t* colors_out, uint8_t* agree_out, void* stream);
size_t gsr_voxel_workspace_bytes(int64_t N);
int gsr_voxel_downsample(const float* points, const uint8_t* colors, int64_t N, const double* grid_host,
                         float* points_out, uint8_t* colors_out, int32_t* counts_out, uint32_t* K_dev, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- TSDF meshing (no reference counterpart): depth maps -> truncated signed distance volume -> surface-nets mesh ----
 * The arithmetic and the full statement of the contract are csrc/gsr_mesh.h, shared with the host shim: fp64, every
 * operation rounded on its own, integer accumulation, no atomics.  The volume has nx x ny x nz nodes (at most 2^29), node
 * (i, j, k) at index (k ny + j) nx + i and position o + idx voxel; grid_host [4] = voxel ox oy oz.  state [6, nodes]
 * int32 in planes: sum_d, n, colour count, three colour byte sums.  Every double travels in a host array, read before
 * the call returns.
 *
 * gsr_tsdf_integrate adds S <= GSR_FUSE_MAX_SOURCES views in one launch; each thread owns one node.  sources_host [S]
 * name each view's depth map [H, W] and, optionally, its image [H, W, 3] float (NULL: white);  source_params_host
 * [S, 16] = the rows of src_t_world (3 x 4), then fx fy cx cy;  tsdf_host [3] = near, trunc, 1 / trunc.  Per node and
 * source: the projection of gsr_fuse_check; ds = the depth at the pixel, skipped unless valid; diff = ds - p_2, skipped
 * unless diff >= -trunc; Q = floor(clamp(diff / trunc, -1, 1) 32768 + 0.5) is added to sum_d and 1 to n; where diff <=
 * trunc the colour count grows by 1 and the colour sums by the pixel's bytes (the rule of gsr_fuse_emit).  A volume
 * takes at most 65535 views in all (the caller counts them).
 *   Checked in this order: a negative nx, ny or nz GSR_ERR_INVALID_ARGUMENT; a side or the node count above 2^29
 *   GSR_ERR_UNSUPPORTED (a side alone, even where another side is 0); S
 *   outside [1, GSR_FUSE_MAX_SOURCES], a NULL host array, a host value that is not finite, voxel not above 0 (or 1 / voxel
 *   not finite), trunc or 1 / trunc not above 0 GSR_ERR_INVALID_ARGUMENT; a source side below 0
 *   GSR_ERR_INVALID_ARGUMENT, above 32768 GSR_ERR_UNSUPPORTED; no node GSR_OK; a NULL state, or a NULL depth of a
 *   source that has pixels, GSR_ERR_INVALID_ARGUMENT.
 *
 * Extraction (surface nets; valid = n >= min_weight, negative = sum_d < 0, m = sum_d / n).  A cell, the box between
 * eight nodes, is active when all corners are valid and their signs are mixed.  gsr_mesh_vertex_mask writes active_out
 * [cells] bytes, the input of gsr_compact_offsets;  gsr_mesh_vertex_emit writes cell_vertex_out [cells] int32 (the
 * cell's vertex index, ascending with the cell index, or -1) whatever the capacity, and row r of vertices_out
 * [capacity, 3] float and colors_out [capacity, 3] uint8 for vertex r < capacity: the mean of the cell's edge
 * crossings and the rounded mean colour of its corners.  gsr_mesh_face_mask writes keep_out [3 nodes] bytes: lattice
 * edge e = 3 node + axis is kept when its upper node is in the grid, both ends are valid and differ in sign and the
 * four cells around it are in range and active (cell_vertex >= 0);  gsr_mesh_face_emit writes rows 2 r and 2 r + 1 of
 * faces_out [capacity, 3] int32 for the r-th kept edge, each row only where it is below capacity.  block_offsets: what
 * gsr_compact_offsets made of the mask before it.
 *   Checked in this order: a negative nx, ny, nz or capacity GSR_ERR_INVALID_ARGUMENT; a side or the node count above
 *   2^29 GSR_ERR_UNSUPPORTED; min_weight below 1, (vertex emit) a NULL or non-finite grid_host or a voxel not above 0
 *   GSR_ERR_INVALID_ARGUMENT; no cell, or (face emit) capacity == 0, GSR_OK and nothing is written; a NULL device
 *   pointer GSR_ERR_INVALID_ARGUMENT, except vertices_out and colors_out where capacity == 0. */
typedef struct GsrTsdfSource {
  const float* depth;    /* [H, W] */
  const float* image;    /* [H, W, 3], or NULL */
  int32_t H, W;
} GsrTsdfSource;
int gsr_tsdf_integrate(int32_t* state, int32_t nx, int32_t ny, int32_t nz, const double* grid_host,
                       const GsrTsdfSource* sources_host, const double* source_params_host, int32_t S,
                       const double* tsdf_host, void* stream);
int gsr_mesh_vertex_mask(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                         uint8_t* active_out, void* stream);
int gsr_mesh_vertex_emit(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, const double* grid_host,
                         int32_t min_weight, const uint32_t* block_offsets, int64_t capacity, int32_t* cell_vertex_out,
                         float* vertices_out, uint8_t* colors_out, void* stream);
int gsr_mesh_face_mask(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                       const int32_t* cell_vertex, uint8_t* keep_out, void* stream);
int gsr_mesh_face_emit(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                       const int32_t* cell_vertex, const uint32_t* block_offsets, int64_t capacity, int32_t* faces_out,
                       void* stream);

/* ---- normal consistency (no reference counterpart; 2DGS section 4.2): splat normals, depth normals, the loss --------
 * The arithmetic and the full statement of the contract are csrc/gsr_normals.h: fp32, pixel centres at +0.5, projection
 * [4] = fx fy cx cy and T_camera_world [4, 4] row-major on the device.  No atomics, one writer per element; the loss is a
 * fixed-order sum, so two runs give the same bits.  A side is at most 32768.
 *
 * gsr_splat_normals_forward.  Per visible row i = indexes[m] (unique, inside [0, N); a row outside gets the normal 0) the
 * column of the rotation matrix that belongs to the smallest log_scaling (the lowest index on ties), in camera space,
 * turned towards the camera.  depth NULL: out [M, 3].  depth [M]: out [M, 5] = n, depth, 1, the feature rows of the
 * geometry image.  gsr_splat_normals_backward recomputes the forward and writes row i of d_rotation [N, 4] from
 * d_out [M, stride] (stride 3 or 5); the other rows are untouched: pass zeros.  d_depth [M] (stride 5 only, may be NULL)
 * gets column 3 of d_out.  Position, log_scaling and the camera receive no gradient: the axis and the flip are constants.
 *   Checked in this order: M or N outside [0, GSR_NEIGHBOURS_MAX_N], a stride other than 3 and 5, d_depth with stride 3
 *   GSR_ERR_INVALID_ARGUMENT; M == 0 GSR_OK; a NULL pointer other than depth / d_depth, a rotation or d_rotation that is
 *   not 16-byte aligned GSR_ERR_INVALID_ARGUMENT.
 *
 * gsr_depth_normals.  depth [H, W] -> normals_out [H, W, 3]: the unit normal of the back-projected central differences,
 * (0, 0, -1) for a fronto-parallel surface; exactly 0 on the border and wherever the pixel's depth or one of its four
 * taps' is not finite and above 0.
 *
 * gsr_normal_loss_forward.  geometry [H, W, 5] = N^x N^y N^z D A (the composite of the rows above).  d = D / A where
 * A >= alpha_min, else not valid; normals_out [H, W, 3] = the depth normals of d; loss_out [1] = sum over the valid pixels
 * of A - N^ . n_d, divided by H W.  partials: gsr_normal_loss_blocks(H, W) floats of workspace (0 for sides outside
 * [1, 32768]).  gsr_normal_loss_backward recomputes the forward and writes d_geometry [H, W, 5], every element, from the
 * device scalar d_loss [1]: D and A also receive what passes through d into the normals of the four neighbours, gathered
 * in the order left, right, up, down.  The projection receives no gradient.
 *   Checked in this order: a negative side or a NaN alpha_min GSR_ERR_INVALID_ARGUMENT; a side above 32768
 *   GSR_ERR_UNSUPPORTED; H == 0 or W == 0 GSR_OK and nothing is written; a NULL pointer GSR_ERR_INVALID_ARGUMENT. */
int gsr_splat_normals_forward(const float* rotation_xyzw, const float* log_scaling, const float* position, int64_t N,
                              const int64_t* indexes, int64_t M, const float* T_camera_world, const float* depth,
                              float* out, void* stream);
int gsr_splat_normals_backward(const float* rotation_xyzw, const float* log_scaling, const float* position, int64_t N,
                               const int64_t* indexes, int64_t M, const float* T_camera_world, const float* d_out,
                               int32_t stride, float* d_rotation, float* d_depth, void* stream);
int gsr_depth_normals(const float* depth, int32_t H, int32_t W, const float* projection, float* normals_out,
                      void* stream);
int64_t gsr_normal_loss_blocks(int32_t H, int32_t W);
int gsr_normal_loss_forward(const float* geometry, int32_t H, int32_t W, const float* projection, float alpha_min,
                            float* normals_out, float* partials, float* loss_out, void* stream);
int gsr_normal_loss_backward(const float* geometry, int32_t H, int32_t W, const float* projection, float alpha_min,
                             const float* d_loss, float* d_geometry, void* stream);

/* ---- data-parallel exchange helpers (no reference counterpart: the reference is single-GPU) ------------- */
/* One fixed-size block per camera, GSR_DP_BLOCK_FLOATS(N) = 6N + 3 floats: [0,3N) colour-gradient rows (0 where the
 * camera saw nothing), [3N,3N+3) camera position, [3N+3,4N+3) split_score and [4N+3,5N+3) prune_cost (NaN where
 * unseen), [5N+3,6N+3) larger screen-space sigma (0 where unseen).  The first 3N+3 floats are the per-camera input of
 * gsr_sh_backward_multi.  gsr_dp_pack fills one block from a camera's rows (idx NULL: rows are the points 0..M-1);
 * gsr_dp_replay applies the two order-dependent exp_lerp EMAs of PointState.add_rendering (point_state.py:49-50) for
 * all cameras in camera order (slots[c] = block index of camera c) and folds the screen-scale maximum (:37).
 * The two order-independent SUMS of the update ride along: gsr_dp_pack(visibility, visibility_sum, views_sum) adds this
 * camera's visibility and its "saw the point" count to two N-sized accumulators (the extra columns of the gradient
 * all-reduce); gsr_dp_replay(visibility_sum, views_sum, state_visibility, state_points_in_view) adds the all-reduced
 * sums to the state (:40,43).  Pass NULL for the group to leave it out. */
#define GSR_DP_BLOCK_FLOATS(N) (6 * (int64_t)(N) + 3)
int gsr_dp_pack(const int64_t* idx, const float* dL_dcolors, const float* split_score, const float* prune_cost,
                const float* screen_scale, int32_t scale_cols, const float* camera_pos, int64_t M, int64_t N,
                float* block_out, const float* visibility, float* visibility_sum, float* views_sum, void* stream);
int gsr_dp_replay(const float* blocks, int64_t stride, const int32_t* slots, int32_t num_cameras, int64_t N,
                  float split_alpha, float prune_alpha, float* state_split_score, float* state_prune_cost,
                  float* state_max_scale_px, const float* visibility_sum, const float* views_sum,
                  float* state_visibility, int16_t* state_points_in_view, void* stream);

/* Sharded form of the exchange (default since round 4).  L = ceil(N / num_ranks); rank r owns the points [r L, (r+1) L).
 * gsr_dp_pack_sharded fills, for ONE camera of this rank (slot of slots_per_rank): factors_out (3N + 3 floats: the
 * camera's all-gather block, colour-gradient rows + camera position -- the input of gsr_sh_backward_multi); its two
 * controller scores in the all-to-all SEND layout scores_out[dest rank][slot][field][L] (field 0 split_score, 1
 * prune_cost; NaN where unseen); the running maximum of the larger screen-space sigma over this rank's cameras in
 * scale_max[N] (finished by a MAX all-reduce); and the two sums as gsr_dp_pack does.  factors_out may be NULL (the block
 * was packed earlier by gsr_dp_pack_factors_rows).
 * gsr_dp_replay_slice applies the two exp_lerp EMAs (point_state.py:49-50) of ALL cameras of the batch in camera order
 * (camera c arrived from rank c % num_ranks in slot c / num_ranks: recv[src rank][slot][field][L]) to this rank's slice
 * of the state and leaves the slice's new values in slice_out[field][L], the all-gather send buffer.
 * gsr_dp_finish writes the gathered slices (gathered[rank][field][L]) back into the N-sized state and folds the reduced
 * maximum and sums (any of the two groups may be NULL). */
int gsr_dp_pack_sharded(const int64_t* idx, const float* dL_dcolors, const float* split_score, const float* prune_cost,
                        const float* screen_scale, int32_t scale_cols, const float* camera_pos, int64_t M, int64_t N,
                        int32_t num_ranks, int32_t slots_per_rank, int32_t slot, float* factors_out, float* scores_out,
                        float* scale_max, const float* visibility, float* visibility_sum, float* views_sum, void* stream);
/* factors_out (3N + 3) of one camera straight from its packed gradient rows [M,16] (columns 8..10 = d colour), i.e. before
 * the backward sweep has copied them out: what lets the factor all-gather start behind gsr_frame_backward_stages(.., 1, ..).
 * gsr_dp_pack_sharded(factors_out = NULL) then leaves the block alone. */
int gsr_dp_pack_factors_rows(const int64_t* idx, const float* grad_rows, const float* camera_pos, int64_t M, int64_t N,
                             float* factors_out, void* stream);
int gsr_dp_replay_slice(const float* recv, int32_t num_ranks, int32_t slots_per_rank, int64_t N, int32_t rank,
                        int32_t num_cameras, float split_alpha, float prune_alpha, const float* state_split_score,
                        const float* state_prune_cost, float* slice_out, void* stream);
int gsr_dp_finish(const float* gathered, int32_t num_ranks, int64_t N, float* state_split_score, float* state_prune_cost,
                  const float* scale_max, float* state_max_scale_px, const float* visibility_sum, const float* views_sum,
                  float* state_visibility, int16_t* state_points_in_view, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_HIP_H */
