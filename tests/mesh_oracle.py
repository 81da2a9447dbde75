"""The TSDF meshing contract in numpy float64 and integers, stated on its own (not read off csrc/gsr_mesh.h): one
rounded operation per statement in the order the contract writes them.  No torch, nothing of the package: the native
layer and the host shim are both compared with this, bit for bit.

The volume: nx x ny x nz nodes, node (i, j, k) at index (k ny + j) nx + i and position o + idx voxel; state int (6, nodes)
in planes sum_d, n, colour count, three colour byte sums."""
import numpy as np

import fusion_oracle

F64 = np.float64
SCALE = F64(32768.0)


def node_coords(dims):
  """(I, J, K) int64 (nodes,) of every node in index order, x fastest."""
  nx, ny, nz = dims
  k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
  return i.reshape(-1), j.reshape(-1), k.reshape(-1)


def positions(dims, grid):
  """(X, Y, Z) float64 (nodes,): o + idx voxel, the product rounded, then the sum."""
  voxel, origin = F64(grid[0]), [F64(v) for v in grid[1:]]
  out = []
  for axis, idx in enumerate(node_coords(dims)):
    step = idx.astype(F64) * voxel
    out.append(origin[axis] + step)
  return out


def sample(ds, p2, trunc, inv_trunc):
  """(taken bool, Q int64, coloured bool) of source depths ds against node depths p2, float64 arrays."""
  with np.errstate(all="ignore"):
    ds, p2 = np.asarray(ds, F64), np.asarray(p2, F64)
    diff = ds - p2
    taken = fusion_oracle.valid(ds) & (diff >= -F64(trunc))
    s = diff * F64(inv_trunc)
    s = np.where(s > 1, 1.0, s)
    s = np.where(s < -1, -1.0, s)
    s = s * SCALE
    s = s + F64(0.5)
    Q = np.floor(np.where(taken, s, 0.0)).astype(np.int64)
    return taken, Q, taken & (diff <= F64(trunc))


def integrate(state, dims, grid, sources, near, trunc):
  """The state after the views `sources` = [(depth float32 (H, W), image float32 (H, W, 3) or None, params16)];
  `state` int (6, nodes) is not modified.  `near`: one value, or one per source."""
  out = np.array(state, np.int64)
  X, Y, Z = positions(dims, grid)
  inv_trunc = F64(1.0) / F64(trunc)
  nears = list(near) if np.ndim(near) else [near] * len(sources)
  with np.errstate(all="ignore"):
    for (depth, image, params), n in zip(sources, nears):
      H, W = depth.shape
      params = np.asarray(params, F64)
      rel, (fx, fy, cx, cy) = params[:12], params[12:]
      p0, p1, p2 = (fusion_oracle._row(rel[4 * k:4 * k + 4], X, Y, Z) for k in range(3))
      ok = p2 > F64(n)
      iz = F64(1.0) / p2
      us = p0 * iz
      vs = p1 * iz
      us = fx * us
      vs = fy * vs
      us = us + cx
      vs = vs + cy
      ok = ok & (us >= 0) & (us < F64(W)) & (vs >= 0) & (vs < F64(H))
      js = np.floor(np.where(ok, us, 0.0)).astype(np.int64)
      is_ = np.floor(np.where(ok, vs, 0.0)).astype(np.int64)
      ds = (depth[is_, js] if depth.size else np.zeros_like(p2)).astype(F64)
      taken, Q, coloured = sample(ds, p2, trunc, inv_trunc)
      taken, coloured = taken & ok, coloured & ok
      out[0] += np.where(taken, Q, 0)
      out[1] += taken
      out[2] += coloured
      if image is None:
        out[3:6] += 255 * coloured.astype(np.int64)[None]
      else:
        out[3:6] += np.where(coloured[:, None], fusion_oracle.colour_bytes(image)[is_, js].astype(np.int64), 0).T
  assert np.abs(out).max(initial=0) < 2 ** 31
  return out.astype(np.int32)


# corner number dx + 2 dy + 4 dz; the 12 edges: axis a, then ov, then ou, from (a: 0, u: ou, v: ov) to (a: 1, ...)
def _edges():
  out = []
  for a in range(3):
    u, v = (a + 1) % 3, (a + 2) % 3
    for ov in range(2):
      for ou in range(2):
        A = (ou << u) | (ov << v)
        out.append((a, u, v, ou, ov, A, A | (1 << a)))
  return out


EDGES = _edges()
QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))


def extract(state, dims, grid, min_weight=1):
  """(vertices float32 (V, 3), colours uint8 (V, 3), faces int32 (F, 3), cell_vertex int32 (cells,))."""
  nx, ny, nz = dims
  state = np.asarray(state).astype(np.int64).reshape(6, nz, ny, nx)
  cell_dims = (max(nx - 1, 0), max(ny - 1, 0), max(nz - 1, 0))
  cells = cell_dims[0] * cell_dims[1] * cell_dims[2]
  none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
  if cells == 0:
    return none + (np.zeros((0,), np.int32),)
  voxel, origin = F64(grid[0]), [F64(v) for v in grid[1:]]

  def corner(plane, k):
    dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
    return state[plane, dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].reshape(-1)
  sums, ns = [corner(0, k) for k in range(8)], [corner(1, k) for k in range(8)]
  valid = np.all([n >= min_weight for n in ns], 0)
  negs = np.sum([s < 0 for s in sums], 0)
  active = valid & (negs != 0) & (negs != 8)
  at = np.flatnonzero(active)                                         # ascending cell index
  cell_vertex = np.full(cells, -1, np.int32)
  cell_vertex[at] = np.arange(len(at), dtype=np.int32)
  with np.errstate(all="ignore"):
    m = [sums[k][at].astype(F64) / ns[k][at].astype(F64) for k in range(8)]
    neg = [sums[k][at] < 0 for k in range(8)]
    acc = [np.zeros(len(at), F64) for _ in range(3)]
    count = np.zeros(len(at), np.int64)
    for a, u, v, ou, ov, A, B in EDGES:
      cross = neg[A] != neg[B]
      d = m[A] - m[B]
      t = m[A] / d
      acc[a] = np.where(cross, acc[a] + t, acc[a])
      acc[u] = np.where(cross, acc[u] + F64(ou), acc[u])
      acc[v] = np.where(cross, acc[v] + F64(ov), acc[v])
      count += cross
    ci = at % cell_dims[0], (at // cell_dims[0]) % cell_dims[1], at // (cell_dims[0] * cell_dims[1])
    vertices = np.zeros((len(at), 3), np.float32)
    for k in range(3):
      q = acc[k] / count.astype(F64)
      q = ci[k].astype(F64) + q
      q = q * voxel
      q = origin[k] + q
      vertices[:, k] = q.astype(np.float32)
  n_c = np.sum([corner(2, k)[at] for k in range(8)], 0)
  colours = np.full((len(at), 3), 255, np.uint8)
  for ch in range(3):
    C = np.sum([corner(3 + ch, k)[at] for k in range(8)], 0)
    has = n_c > 0
    colours[has, ch] = (2 * C[has] + n_c[has]) // (2 * n_c[has])

  # faces: every lattice edge e = 3 node + axis, in ascending e
  c = node_coords(dims)
  n = (nx, ny, nz)
  flat_sum, flat_n = state[0].reshape(-1), state[1].reshape(-1)
  nodes = nx * ny * nz
  kept = np.zeros((nodes, 3), bool)
  tris = np.zeros((nodes, 3, 2, 3), np.int32)
  stride = (1, nx, nx * ny)
  cell_stride = (1, cell_dims[0], cell_dims[0] * cell_dims[1])
  for axis in range(3):
    u, v = (axis + 1) % 3, (axis + 2) % 3
    ok = (c[axis] + 1 < n[axis]) & (c[u] >= 1) & (c[u] + 1 < n[u]) & (c[v] >= 1) & (c[v] + 1 < n[v])
    lower = np.flatnonzero(ok)
    upper = lower + stride[axis]
    cross = ((flat_n[lower] >= min_weight) & (flat_n[upper] >= min_weight) & ((flat_sum[lower] < 0) != (flat_sum[upper] < 0)))
    q = []
    for du, dv in QUAD:
      cc = [c[0][lower], c[1][lower], c[2][lower]]
      cc[u] = cc[u] + du
      cc[v] = cc[v] + dv
      q.append(cell_vertex[cc[0] * cell_stride[0] + cc[1] * cell_stride[1] + cc[2] * cell_stride[2]])
    q = np.stack(q, 1)                                                # (edges, 4)
    keep = cross & (q >= 0).all(1)
    flip = ~(flat_sum[lower] < 0)                                     # the lower node is not negative: reversed
    q = np.where(flip[:, None], q[:, ::-1], q)
    kept[lower, axis] = keep
    tris[lower, axis, 0] = q[:, [0, 1, 2]]
    tris[lower, axis, 1] = q[:, [0, 2, 3]]
  faces = tris[kept].reshape(-1, 3).astype(np.int32)
  return vertices, colours, faces, cell_vertex


# ---- properties of a mesh ----
def signed_volume_normals(vertices, faces):
  """Per-face normals (not normalised) and centroids, float64."""
  p = vertices.astype(F64)[faces]
  return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p.mean(1)


def closed_manifold_report(faces):
  """(every undirected edge in exactly two triangles, every directed edge once, V - E + F over the used vertices)."""
  directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
  _, directed_counts = np.unique(directed, axis=0, return_counts=True)
  undirected, counts = np.unique(np.sort(directed, 1), axis=0, return_counts=True)
  V, E, F = len(np.unique(faces)), len(undirected), len(faces)
  return bool((counts == 2).all()), bool((directed_counts == 1).all()), V - E + F


def sphere_state(dims, grid, centre, radius, trunc):
  """The state of an analytic sphere: sum_d = floor(clamp(sdf / trunc) 32768 + 0.5), n = 1, no colour."""
  X, Y, Z = positions(dims, grid)
  sdf = np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius
  state = np.zeros((6, len(X)), np.int32)
  state[0] = np.floor(np.clip(sdf / trunc, -1.0, 1.0) * 32768.0 + 0.5).astype(np.int32)
  state[1] = 1
  return state
