// TSDF meshing: integration of depth maps into a truncated signed distance volume and extraction of its zero surface
// as a surface-nets mesh.  The arithmetic and the contract are in gsr_mesh.h (fp64, no contraction), the entry points
// in include/gsplat_hip.h.
//
// tsdf_integrate_kernel.  One thread per node in blocks of 256 consecutive indexes, x fastest: the six plane accesses of
//   a wave are contiguous.  The sources travel in the kernel arguments; the thread walks them with its position in
//   registers and then reads and writes its six integers once, and not at all where no source reached it.  It is the only
//   writer of them: no atomics.
// mesh_vertex_mask_kernel / mesh_vertex_emit_kernel.  One thread per cell in blocks of GSR_COMPACT_BLOCK, the block
//   size of gsr_compact_offsets.  The mask kernel writes the active byte; the emit kernel evaluates the same predicate
//   again, ranks the active cells of its block by ballot and writes cell_vertex for every cell and the vertex row
//   block offset + rank for the active ones.
// mesh_face_mask_kernel / mesh_face_emit_kernel.  The same pair over the 3 nodes lattice edges; a cell is active where
//   cell_vertex says so.
// No LDS beyond the block hand-off of gsr_block_rank, no scratch, no atomics, plain vector stores.
#include "gsr_device.h"
#include "gsr_host.h"
#include "gsr_mesh.h"

namespace {

constexpr int MB = GSR_COMPACT_BLOCK;   // threads per block: the emit kernels rank inside gsr_compact_offsets' blocks

__global__ __launch_bounds__(MB) void tsdf_integrate_kernel(int32_t* __restrict__ state, GsrMeshGrid g, uint32_t nodes,
                                                            GsrTsdfParams p, GsrTsdfSourceSet set) {
  const uint32_t node = blockIdx.x * MB + threadIdx.x;      // nodes <= 2^29
  if (node >= nodes) return;
  int32_t c[3];
  g.node_coords(node, c);
  const double X = gsr_tsdf_position(p.origin[0], p.voxel, c[0]), Y = gsr_tsdf_position(p.origin[1], p.voxel, c[1]),
               Z = gsr_tsdf_position(p.origin[2], p.voxel, c[2]);
  GsrTsdfDelta d = {};
  for (int s = 0; s < set.S; ++s) gsr_tsdf_observe(set, s, p, X, Y, Z, &d);
  if (d.n == 0) return;
  int32_t* at = state + node;
  const int64_t plane = nodes;
  const bool coloured = d.nc != 0;
  const int32_t v0 = at[0], v1 = at[plane];
  int32_t v2 = 0, v3 = 0, v4 = 0, v5 = 0;
  if (coloured) { v2 = at[2 * plane]; v3 = at[3 * plane]; v4 = at[4 * plane]; v5 = at[5 * plane]; }
  at[0] = v0 + d.sum_d;
  at[plane] = v1 + d.n;
  if (!coloured) return;
  at[2 * plane] = v2 + d.nc;
  at[3 * plane] = v3 + d.c[0];
  at[4 * plane] = v4 + d.c[1];
  at[5 * plane] = v5 + d.c[2];
}

__global__ __launch_bounds__(MB) void mesh_vertex_mask_kernel(const int32_t* __restrict__ state, GsrMeshGrid g, uint32_t cells,
                                                              int32_t min_weight, uint8_t* __restrict__ active_out) {
  const uint32_t cell_id = blockIdx.x * MB + threadIdx.x;
  if (cell_id >= cells) return;
  int32_t c[3];
  g.cell_coords(cell_id, c);
  GsrMeshCell cell;
  gsr_mesh_load_cell(state, g, c, &cell);
  active_out[cell_id] = gsr_mesh_active(cell, min_weight) ? 1 : 0;
}

__global__ __launch_bounds__(MB) void mesh_vertex_emit_kernel(const int32_t* __restrict__ state, GsrMeshGrid g, uint32_t cells,
                                                              GsrTsdfParams p, int32_t min_weight,
                                                              const uint32_t* __restrict__ block_offsets, int64_t capacity,
                                                              int32_t* __restrict__ cell_vertex_out,
                                                              float* __restrict__ vertices_out,
                                                              uint8_t* __restrict__ colors_out) {
  const uint32_t cell_id = blockIdx.x * MB + threadIdx.x;
  const int64_t plane = g.nodes();
  int32_t c[3] = {0, 0, 0};
  GsrMeshCell cell;
  bool active = false;
  if (cell_id < cells) {
    g.cell_coords(cell_id, c);
    gsr_mesh_load_cell(state, g, c, &cell);
    active = gsr_mesh_active(cell, min_weight);
  }
  const uint32_t rank = gsr_block_rank(active).before;
  if (cell_id >= cells) return;
  const int64_t row = (int64_t)block_offsets[blockIdx.x] + rank;
  cell_vertex_out[cell_id] = active ? (int32_t)row : -1;
  if (!active || row >= capacity) return;
  float v[3];
  gsr_mesh_vertex(cell, c, p, v);
  float* out = vertices_out + 3 * row;
  out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
  int64_t nc = 0, C0 = 0, C1 = 0, C2 = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int32_t* at = state + gsr_mesh_corner_node(g, c, k);
    nc += at[2 * plane];
    C0 += at[3 * plane];
    C1 += at[4 * plane];
    C2 += at[5 * plane];
  }
  uint8_t* col = colors_out + 3 * row;
  col[0] = gsr_mesh_colour(C0, nc);
  col[1] = gsr_mesh_colour(C1, nc);
  col[2] = gsr_mesh_colour(C2, nc);
}

__global__ __launch_bounds__(MB) void mesh_face_mask_kernel(const int32_t* __restrict__ state,
                                                            const int32_t* __restrict__ cell_vertex, GsrMeshGrid g,
                                                            uint32_t edges, int32_t min_weight, uint8_t* __restrict__ keep_out) {
  const uint32_t e = blockIdx.x * MB + threadIdx.x;      // edges <= 3 * 2^29
  if (e >= edges) return;
  bool lower_negative;
  int32_t q[4];
  keep_out[e] = gsr_mesh_edge_kept(state, cell_vertex, g, e, min_weight, &lower_negative, q) ? 1 : 0;
}

__global__ __launch_bounds__(MB) void mesh_face_emit_kernel(const int32_t* __restrict__ state,
                                                            const int32_t* __restrict__ cell_vertex, GsrMeshGrid g,
                                                            uint32_t edges, int32_t min_weight,
                                                            const uint32_t* __restrict__ block_offsets, int64_t capacity,
                                                            int32_t* __restrict__ faces_out) {
  const uint32_t e = blockIdx.x * MB + threadIdx.x;
  bool lower_negative = false, kept = false;
  int32_t q[4] = {0, 0, 0, 0};
  if (e < edges) kept = gsr_mesh_edge_kept(state, cell_vertex, g, e, min_weight, &lower_negative, q);
  const uint32_t rank = gsr_block_rank(kept).before;
  if (!kept) return;
  const int64_t row = 2 * ((int64_t)block_offsets[blockIdx.x] + rank);
  int32_t t[6];
  gsr_mesh_quad(q, lower_negative, t);
  if (row < capacity) {
    int32_t* out = faces_out + 3 * row;
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
  }
  if (row + 1 < capacity) {
    int32_t* out = faces_out + 3 * (row + 1);
    out[0] = t[3]; out[1] = t[4]; out[2] = t[5];
  }
}

}  // namespace

extern "C" {

int gsr_tsdf_integrate(int32_t* state, int32_t nx, int32_t ny, int32_t nz, const double* grid_host,
                       const GsrTsdfSource* sources_host, const double* source_params_host, int32_t S,
                       const double* tsdf_host, void* stream_) {
  int launch = 0;
  const int rc = gsr_tsdf_integrate_args(state, nx, ny, nz, grid_host, sources_host, source_params_host, S, tsdf_host, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  GsrTsdfSourceSet set = {};
  gsr_tsdf_source_set_make(sources_host, source_params_host, S, &set);
  const int64_t nodes = g.nodes();
  tsdf_integrate_kernel<<<grid_for(nodes, MB), MB, 0, gsr_stream(stream_)>>>(state, g, (uint32_t)nodes,
                                                                            gsr_tsdf_params_make(grid_host, tsdf_host), set);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_mesh_vertex_mask(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight, uint8_t* active_out,
                         void* stream_) {
  int launch = 0;
  const int rc = gsr_mesh_vertex_mask_args(state, nx, ny, nz, min_weight, active_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  const int64_t cells = g.cells();
  mesh_vertex_mask_kernel<<<grid_for(cells, MB), MB, 0, gsr_stream(stream_)>>>(state, g, (uint32_t)cells, min_weight, active_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_mesh_vertex_emit(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, const double* grid_host,
                         int32_t min_weight, const uint32_t* block_offsets, int64_t capacity, int32_t* cell_vertex_out,
                         float* vertices_out, uint8_t* colors_out, void* stream_) {
  int launch = 0;
  const int rc = gsr_mesh_vertex_emit_args(state, nx, ny, nz, grid_host, min_weight, block_offsets, true, capacity,
                                           cell_vertex_out, vertices_out, colors_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  const int64_t cells = g.cells();
  mesh_vertex_emit_kernel<<<grid_for(cells, MB), MB, 0, gsr_stream(stream_)>>>(
      state, g, (uint32_t)cells, gsr_tsdf_params_make(grid_host, nullptr), min_weight, block_offsets, capacity,
      cell_vertex_out, vertices_out, colors_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_mesh_face_mask(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                       const int32_t* cell_vertex, uint8_t* keep_out, void* stream_) {
  int launch = 0;
  const int rc = gsr_mesh_face_mask_args(state, nx, ny, nz, min_weight, cell_vertex, keep_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  const int64_t edges = 3 * g.nodes();
  mesh_face_mask_kernel<<<grid_for(edges, MB), MB, 0, gsr_stream(stream_)>>>(state, cell_vertex, g, (uint32_t)edges,
                                                                            min_weight, keep_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

int gsr_mesh_face_emit(const int32_t* state, int32_t nx, int32_t ny, int32_t nz, int32_t min_weight,
                       const int32_t* cell_vertex, const uint32_t* block_offsets, int64_t capacity, int32_t* faces_out,
                       void* stream_) {
  int launch = 0;
  const int rc = gsr_mesh_face_emit_args(state, nx, ny, nz, min_weight, cell_vertex, block_offsets, true, capacity,
                                         faces_out, &launch);
  if (rc < 0 || !launch) return rc;
  const GsrMeshGrid g = {{nx, ny, nz}};
  const int64_t edges = 3 * g.nodes();
  mesh_face_emit_kernel<<<grid_for(edges, MB), MB, 0, gsr_stream(stream_)>>>(state, cell_vertex, g, (uint32_t)edges,
                                                                            min_weight, block_offsets, capacity, faces_out);
  GSR_CHECK_LAUNCH();
  return GSR_OK;
}

}  // extern "C"
