// Arithmetic of the TSDF meshing (mesh.hip), shared with the CPU shim (hostmath_shim.cpp).  The functions read the
// sources' maps, the volume's state and cell_vertex and write nothing: who writes what is the caller's business.  This
// text is the statement of record of the contract; include/gsplat_hip.h gives the entry points and their argument checks.
//
// Everything is fp64, every product, sum and quotient rounded on its own in the order written here (no contraction).
//
// The volume.  nx x ny x nz nodes, nx ny nz <= 2^29; node (i, j, k) has the linear index (k ny + j) nx + i, x fastest,
// and the position o + idx voxel per axis (one product, one sum).  The state is int32 [6, nodes] in planes: 0 sum_d,
// 1 n, 2 colour count, 3..5 colour byte sums.  All accumulation is integer: the state after a set of views does not
// depend on their order or on how they are chunked into calls.  A volume takes at most 65535 views: |Q| <= 32768, so
// sum_d stays inside int32.
//
// Integration of one source into node P = (X, Y, Z), with rel = the rows of src_t_world (3 x 4):
//   p_k = ((r_k0 X + r_k1 Y) + r_k2 Z) + t_k;  !(p_2 > near): skip;  iz = 1 / p_2
//   us = fx (p_0 iz) + cx, vs likewise; outside [0, W) x [0, H) or NaN: skip;  ds = depth[floor vs, floor us]
//   (gsr_fuse_project of gsr_fusion.h: the same projection as the consistency check)
//   ds not valid (not above 0 or not finite): skip;  diff = ds - p_2;  !(diff >= -trunc): skip
//   s = max(min(diff inv_trunc, 1), -1) (inv_trunc = 1 / trunc formed by the host);  Q = (int) floor(s 32768 + 0.5)
//   sum_d += Q, n += 1;  if diff <= trunc: colour count += 1, colour sums += the pixel's bytes
//   bytes = floor(clamp(c, 0, 1) 255 + 0.5) of image[floor vs, floor us, :] (NaN -> 0; gsr_fuse_colour), 255 without
//   an image.
//
// Extraction: surface nets.  valid(node) = n >= min_weight (min_weight >= 1), neg(node) = sum_d < 0,
// m(node) = (double) sum_d / (double) n.  Cells are the (nx - 1)(ny - 1)(nz - 1) boxes between nodes; cell (i, j, k) has
// the index (k (ny - 1) + j)(nx - 1) + i and the corners (i + dx, j + dy, k + dz), corner number dx + 2 dy + 4 dz.  A
// cell is active when its eight corners are valid and their signs are mixed.
//   Vertex of an active cell.  The 12 edges in this order: for axis a = x, y, z, with u = (a + 1) % 3 and
//   v = (a + 2) % 3, for ov = 0, 1, for ou = 0, 1: the edge from the corner with offsets (a: 0, u: ou, v: ov) to the one
//   with (a: 1, u: ou, v: ov).  For each edge whose ends differ in sign, with A the lower end and B the upper:
//   t = m_A / (m_A - m_B); acc_a += t, acc_u += ou, acc_v += ov (each accumulator starts at 0 and takes its additions in
//   edge order), c += 1.  vertex_axis = (float)(o + ((double) idx + acc / c) voxel) with idx the cell's coordinate.
//   Colour of the vertex.  C_ch and n_c = the sums over the eight corners of the colour sums and counts, int64; the
//   byte is (2 C_ch + n_c) / (2 n_c) in integer division, 255 where n_c = 0.
//   Vertices come in ascending cell index; cell_vertex [cells] holds each cell's vertex index, or -1.
//   Faces.  Lattice edge e = 3 node + axis runs from the node to its neighbour one step up the axis.  It is kept when
//   that neighbour is in the grid, both ends are valid and differ in sign, and the four cells around it are in range and
//   active: the node's coordinates with (du, dv) = (-1, -1), (0, -1), (0, 0), (-1, 0) added on the axes u = (axis + 1) % 3
//   and v = (axis + 2) % 3.  The quad q0 q1 q2 q3 is those cells' vertex indexes in that order, which winds
//   counter-clockwise seen from up the axis; where the lower node is NOT negative it is reversed to q3 q2 q1 q0.  It
//   yields the triangles (q0, q1, q2), (q0, q2, q3): rows 2 r and 2 r + 1 of faces for the r-th kept edge in ascending e.
//   Normals point to the positive side, free space.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gsplat_hip.h"
#include "gsr_fusion.h"       // gsr_fuse_project, gsr_fuse_valid, gsr_fuse_colour, gsr_fuse_finite
#include "gsr_image.h"        // GSR_IMAGE_MAX_SIDE
#include "gsr_math.h"         // GSR_HD

#define GSR_TSDF_MAX_NODES (1ll << 29)
#define GSR_TSDF_SCALE 32768.0

struct GsrMeshGrid {          // the lattice alone: what the extraction's integer steps need
  int32_t n[3];               // nodes per axis
  GSR_HD int64_t nodes() const { return (int64_t)n[0] * n[1] * n[2]; }
  GSR_HD int64_t cells() const {
    return n[0] < 2 || n[1] < 2 || n[2] < 2 ? 0 : (int64_t)(n[0] - 1) * (n[1] - 1) * (n[2] - 1);
  }
  GSR_HD uint32_t node_index(const int32_t* c) const { return ((uint32_t)c[2] * (uint32_t)n[1] + (uint32_t)c[1]) * (uint32_t)n[0] + (uint32_t)c[0]; }
  GSR_HD uint32_t cell_index(const int32_t* c) const {
    return ((uint32_t)c[2] * (uint32_t)(n[1] - 1) + (uint32_t)c[1]) * (uint32_t)(n[0] - 1) + (uint32_t)c[0];
  }
  GSR_HD void node_coords(uint32_t node, int32_t* c) const {
    const uint32_t row = node / (uint32_t)n[0];
    c[0] = (int32_t)(node - row * (uint32_t)n[0]);
    c[2] = (int32_t)(row / (uint32_t)n[1]);
    c[1] = (int32_t)(row - (uint32_t)c[2] * (uint32_t)n[1]);
  }
  GSR_HD void cell_coords(uint32_t cell, int32_t* c) const {
    const uint32_t w = (uint32_t)(n[0] - 1), h = (uint32_t)(n[1] - 1);
    const uint32_t row = cell / w;
    c[0] = (int32_t)(cell - row * w);
    c[2] = (int32_t)(row / h);
    c[1] = (int32_t)(row - (uint32_t)c[2] * h);
  }
};

struct GsrTsdfParams {        // grid_host and tsdf_host as the kernels take them
  double voxel, origin[3];
  double near, trunc, inv_trunc;
};

struct GsrTsdfSourceSet {     // what the integrate kernel takes by value
  const float* depth[GSR_FUSE_MAX_SOURCES];
  const float* image[GSR_FUSE_MAX_SOURCES];
  int32_t H[GSR_FUSE_MAX_SOURCES], W[GSR_FUSE_MAX_SOURCES];
  GsrFuseView view[GSR_FUSE_MAX_SOURCES];
  int32_t S;
};

inline void gsr_tsdf_source_set_make(const GsrTsdfSource* sources, const double* source_params, int32_t S,
                                     GsrTsdfSourceSet* set) {      // host only
  set->S = S;
  for (int s = 0; s < S; ++s) {
    set->depth[s] = sources[s].depth;
    set->image[s] = sources[s].image;
    set->H[s] = sources[s].H;
    set->W[s] = sources[s].W;
    const double* p = source_params + 16 * s;
    for (int k = 0; k < 12; ++k) set->view[s].rel[k] = p[k];
    set->view[s].fx = p[12]; set->view[s].fy = p[13]; set->view[s].cx = p[14]; set->view[s].cy = p[15];
  }
}

inline GsrTsdfParams gsr_tsdf_params_make(const double* grid, const double* tsdf) {      // host only; tsdf may be NULL
  GsrTsdfParams p = {};
  p.voxel = grid[0];
  p.origin[0] = grid[1]; p.origin[1] = grid[2]; p.origin[2] = grid[3];
  if (tsdf) { p.near = tsdf[0]; p.trunc = tsdf[1]; p.inv_trunc = tsdf[2]; }
  return p;
}

// A node's or a cell's position on one axis: o + idx voxel.
GSR_HD double gsr_tsdf_position(double origin, double voxel, int32_t idx) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double step = (double)idx * voxel;
  return origin + step;
}

struct GsrTsdfDelta {         // what one call adds to a node's six integers
  int32_t sum_d, n, nc, c[3];
};

// A source depth ds against a node at depth p2 in that source: false for no sample, else Q and whether the sample
// carries colour.
GSR_HD bool gsr_tsdf_sample(double ds, double p2, double trunc, double inv_trunc, int32_t* Q, bool* coloured) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!gsr_fuse_valid(ds)) return false;
  const double diff = ds - p2;
  if (!(diff >= -trunc)) return false;
  double v = diff * inv_trunc;
  if (v > 1.0) v = 1.0;
  if (v < -1.0) v = -1.0;
  v = v * GSR_TSDF_SCALE;
  v = v + 0.5;
  *Q = (int32_t)floor(v);
  *coloured = diff <= trunc;
  return true;
}

// One source's share of node (X, Y, Z).
GSR_HD void gsr_tsdf_observe(const GsrTsdfSourceSet& set, int s, const GsrTsdfParams& p, double X, double Y, double Z,
                             GsrTsdfDelta* d) {
  int32_t is, js, Q;
  double p2;
  bool coloured;
  if (!gsr_fuse_project(set.view[s], set.H[s], set.W[s], p.near, X, Y, Z, &is, &js, &p2)) return;
  const int64_t px = (int64_t)is * set.W[s] + js;
  if (!gsr_tsdf_sample((double)set.depth[s][px], p2, p.trunc, p.inv_trunc, &Q, &coloured)) return;
  d->sum_d += Q;
  d->n += 1;
  if (coloured) {
    d->nc += 1;
    const float* im = set.image[s];
    if (im) {
      im += 3 * px;
      d->c[0] += gsr_fuse_colour(im[0]);
      d->c[1] += gsr_fuse_colour(im[1]);
      d->c[2] += gsr_fuse_colour(im[2]);
    } else {
      d->c[0] += 255; d->c[1] += 255; d->c[2] += 255;
    }
  }
}

// ---- extraction ----
struct GsrMeshCell {          // the eight corners of a cell: their sum_d and n, in corner order dx + 2 dy + 4 dz
  int32_t sum_d[8], n[8];
};

GSR_HD uint32_t gsr_mesh_corner_node(const GsrMeshGrid& g, const int32_t* c, int corner) {
  const int32_t q[3] = {c[0] + (corner & 1), c[1] + ((corner >> 1) & 1), c[2] + ((corner >> 2) & 1)};
  return g.node_index(q);
}

// The corners of the cell at coordinates c: planes 0 and 1 of the state.
GSR_HD void gsr_mesh_load_cell(const int32_t* __restrict__ state, const GsrMeshGrid& g, const int32_t* c, GsrMeshCell* cell) {
  const int64_t plane = g.nodes();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t node = gsr_mesh_corner_node(g, c, k);
    cell->sum_d[k] = state[node];
    cell->n[k] = state[plane + node];
  }
}

GSR_HD bool gsr_mesh_active(const GsrMeshCell& cell, int32_t min_weight) {
  bool valid = true;
  int negs = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    valid = valid && cell.n[k] >= min_weight;
    negs += cell.sum_d[k] < 0;
  }
  return valid && negs != 0 && negs != 8;
}

// The vertex of an active cell at coordinates c: out[3].
GSR_HD void gsr_mesh_vertex(const GsrMeshCell& cell, const int32_t* c, const GsrTsdfParams& p, float* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double m[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = (double)cell.sum_d[k] / (double)cell.n[k];
  double acc[3] = {0.0, 0.0, 0.0};
  int count = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int u = (a + 1) % 3, v = (a + 2) % 3;
#pragma unroll
    for (int ov = 0; ov < 2; ++ov) {
#pragma unroll
      for (int ou = 0; ou < 2; ++ou) {
        const int A = (ou << u) | (ov << v), B = A | (1 << a);
        if ((cell.sum_d[A] < 0) != (cell.sum_d[B] < 0)) {
          const double d = m[A] - m[B];
          const double t = m[A] / d;
          acc[a] = acc[a] + t;
          acc[u] = acc[u] + (double)ou;
          acc[v] = acc[v] + (double)ov;
          ++count;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double q = acc[k] / (double)count;
    q = (double)c[k] + q;
    q = q * p.voxel;
    q = p.origin[k] + q;
    out[k] = (float)q;
  }
}

GSR_HD uint8_t gsr_mesh_colour(int64_t C, int64_t nc) { return nc == 0 ? (uint8_t)255 : (uint8_t)((2 * C + nc) / (2 * nc)); }

// Lattice edge `axis` of the node at coordinates c: whether its upper node and its four cells are in range, and then the
// upper node and the cells in quad order.
GSR_HD bool gsr_mesh_edge_cells(const GsrMeshGrid& g, const int32_t* c, int axis, uint32_t* upper, uint32_t* cells) {
  const int u = (axis + 1) % 3, v = (axis + 2) % 3;
  if (c[axis] + 1 >= g.n[axis] || c[u] < 1 || c[u] + 1 >= g.n[u] || c[v] < 1 || c[v] + 1 >= g.n[v]) return false;
  int32_t q[3] = {c[0], c[1], c[2]};
  q[axis] += 1;
  *upper = g.node_index(q);
  q[axis] -= 1;
  q[u] -= 1; q[v] -= 1;
  cells[0] = g.cell_index(q);
  q[u] += 1;
  cells[1] = g.cell_index(q);
  q[v] += 1;
  cells[2] = g.cell_index(q);
  q[u] -= 1;
  cells[3] = g.cell_index(q);
  return true;
}

// Whether the ends of a lattice edge make it a crossing: both valid, signs differ.
GSR_HD bool gsr_mesh_crossing(int32_t sum_lo, int32_t n_lo, int32_t sum_hi, int32_t n_hi, int32_t min_weight) {
  return n_lo >= min_weight && n_hi >= min_weight && (sum_lo < 0) != (sum_hi < 0);
}

// Whether lattice edge e is kept; then its lower node's sign and its four cells' vertices in quad order.
GSR_HD bool gsr_mesh_edge_kept(const int32_t* __restrict__ state, const int32_t* __restrict__ cell_vertex, const GsrMeshGrid& g,
                               uint32_t e, int32_t min_weight, bool* lower_negative, int32_t* q) {
  const uint32_t node = e / 3u;
  const int axis = (int)(e - 3u * node);
  int32_t c[3];
  g.node_coords(node, c);
  uint32_t upper, cells[4];
  if (!gsr_mesh_edge_cells(g, c, axis, &upper, cells)) return false;
  const int64_t plane = g.nodes();
  const int32_t sum_lo = state[node], sum_hi = state[upper];
  if (!gsr_mesh_crossing(sum_lo, state[plane + node], sum_hi, state[plane + upper], min_weight)) return false;
  q[0] = cell_vertex[cells[0]];
  q[1] = cell_vertex[cells[1]];
  q[2] = cell_vertex[cells[2]];
  q[3] = cell_vertex[cells[3]];
  *lower_negative = sum_lo < 0;
  return q[0] >= 0 && q[1] >= 0 && q[2] >= 0 && q[3] >= 0;
}

// The two triangles of a kept edge: out[6].
GSR_HD void gsr_mesh_quad(const int32_t* q, bool lower_negative, int32_t* out) {
  const int32_t q0 = lower_negative ? q[0] : q[3], q1 = lower_negative ? q[1] : q[2];
  const int32_t q2 = lower_negative ? q[2] : q[1], q3 = lower_negative ? q[3] : q[0];
  out[0] = q0; out[1] = q1; out[2] = q2;
  out[3] = q0; out[4] = q2; out[5] = q3;
}

// ---- the argument checks, in the order the ABI states them.  *launch is 0 where GSR_OK means "nothing to do". ----
inline int gsr_mesh_dims_check(int32_t nx, int32_t ny, int32_t nz) {
  if (nx < 0 || ny < 0 || nz < 0) return GSR_ERR_INVALID_ARGUMENT;
  if (nx > GSR_TSDF_MAX_NODES || ny > GSR_TSDF_MAX_NODES || nz > GSR_TSDF_MAX_NODES) return GSR_ERR_UNSUPPORTED;
  const int64_t plane = (int64_t)nx * ny;
  if (nz > 0 && (plane > GSR_TSDF_MAX_NODES || plane * nz > GSR_TSDF_MAX_NODES)) return GSR_ERR_UNSUPPORTED;
  return GSR_OK;
}

inline bool gsr_mesh_grid_ok(const double* grid) {
  return grid && gsr_fuse_finite(grid, 4) && grid[0] > 0.0 && isfinite(1.0 / grid[0]);
}

inline int gsr_tsdf_integrate_args(const void* state, int32_t nx, int32_t ny, int32_t nz, const double* grid,
                                   const GsrTsdfSource* sources, const double* source_params, int32_t S,
                                   const double* tsdf, int* launch) {
  *launch = 0;
  const int rc = gsr_mesh_dims_check(nx, ny, nz);
  if (rc < 0) return rc;
  if (S < 1 || S > GSR_FUSE_MAX_SOURCES) return GSR_ERR_INVALID_ARGUMENT;
  if (!gsr_mesh_grid_ok(grid) || !sources || !source_params || !tsdf) return GSR_ERR_INVALID_ARGUMENT;
  if (!gsr_fuse_finite(source_params, 16 * S) || !gsr_fuse_finite(tsdf, 3) || !(tsdf[1] > 0.0) || !(tsdf[2] > 0.0))
    return GSR_ERR_INVALID_ARGUMENT;
  for (int s = 0; s < S; ++s) {
    if (sources[s].H < 0 || sources[s].W < 0) return GSR_ERR_INVALID_ARGUMENT;
    if (sources[s].H > GSR_IMAGE_MAX_SIDE || sources[s].W > GSR_IMAGE_MAX_SIDE) return GSR_ERR_UNSUPPORTED;
  }
  if ((int64_t)nx * ny * nz == 0) return GSR_OK;
  if (!state) return GSR_ERR_INVALID_ARGUMENT;
  for (int s = 0; s < S; ++s)
    if (!sources[s].depth && sources[s].H > 0 && sources[s].W > 0) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

// What the four extraction entry points share: the lattice, min_weight, and "no cell: nothing to do".
inline int gsr_mesh_common_args(int32_t nx, int32_t ny, int32_t nz, int32_t min_weight, int64_t capacity, const double* grid,
                                bool with_grid, bool* empty) {
  if (nx < 0 || ny < 0 || nz < 0 || capacity < 0) return GSR_ERR_INVALID_ARGUMENT;
  const int rc = gsr_mesh_dims_check(nx, ny, nz);
  if (rc < 0) return rc;
  if (min_weight < 1) return GSR_ERR_INVALID_ARGUMENT;
  if (with_grid && !gsr_mesh_grid_ok(grid)) return GSR_ERR_INVALID_ARGUMENT;
  const GsrMeshGrid g = {{nx, ny, nz}};
  *empty = g.cells() == 0;
  return GSR_OK;
}

inline int gsr_mesh_vertex_mask_args(const void* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                                     const void* active_out, int* launch) {
  *launch = 0;
  bool empty;
  const int rc = gsr_mesh_common_args(nx, ny, nz, min_weight, 0, nullptr, false, &empty);
  if (rc < 0 || empty) return rc;
  if (!state || !active_out) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

inline int gsr_mesh_vertex_emit_args(const void* state, int32_t nx, int32_t ny, int32_t nz, const double* grid,
                                     int32_t min_weight, const void* block_offsets, bool ranked, int64_t capacity,
                                     const void* cell_vertex_out, const void* vertices_out, const void* colors_out,
                                     int* launch) {
  *launch = 0;
  bool empty;
  const int rc = gsr_mesh_common_args(nx, ny, nz, min_weight, capacity, grid, true, &empty);
  if (rc < 0 || empty) return rc;
  if (!state || (ranked && !block_offsets) || !cell_vertex_out) return GSR_ERR_INVALID_ARGUMENT;
  if (capacity > 0 && (!vertices_out || !colors_out)) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

inline int gsr_mesh_face_mask_args(const void* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                                   const void* cell_vertex, const void* keep_out, int* launch) {
  *launch = 0;
  bool empty;
  const int rc = gsr_mesh_common_args(nx, ny, nz, min_weight, 0, nullptr, false, &empty);
  if (rc < 0 || empty) return rc;
  if (!state || !cell_vertex || !keep_out) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}

inline int gsr_mesh_face_emit_args(const void* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                                   const void* cell_vertex, const void* block_offsets, bool ranked, int64_t capacity,
                                   const void* faces_out, int* launch) {
  *launch = 0;
  bool empty;
  const int rc = gsr_mesh_common_args(nx, ny, nz, min_weight, capacity, nullptr, false, &empty);
  if (rc < 0 || empty || capacity == 0) return rc;
  if (!state || !cell_vertex || (ranked && !block_offsets) || !faces_out) return GSR_ERR_INVALID_ARGUMENT;
  *launch = 1;
  return GSR_OK;
}
