"""The TSDF meshing cases that tests/test_mesh_host.py runs on the host shim and tests/test_gpu_mesh.py on the device:
each is a function of a backend (where the arrays live and which library is called) that compares with
tests/mesh_oracle.py exactly, bit for bit.  The raw entry points are used where the package's classes do not reach (one
call of S sources onto a given state, the capacities of the emission); the rest goes through the package."""

import numpy as np
import torch

import fusion_cases
import fusion_oracle
import mesh_oracle as oracle
import splat_trainer_amd as sta
from fusion_cases import camera, depth_map, intrinsics, pose, same
from splat_trainer_amd import _lib

F32, F64 = np.float32, np.float64
SOURCE_DTYPE = np.dtype([("depth", "<u8"), ("image", "<u8"), ("H", "<i4"), ("W", "<i4")])       # GsrTsdfSource: 24 bytes
DIMS = (13, 9, 7)                      # 819 nodes and 576 cells: each compaction spans three blocks and more, the last partial
GRID = np.array([0.5, -3.0, -2.0, 2.0], F64)                     # x in [-3, 3], y in [-2, 2], z in [2, 5]
NODES, CELLS = 13 * 9 * 7, 12 * 8 * 6


# ---- backends --------------------------------------------------------------------------------------------------------
class HostBackend:
  device = "cpu"

  def __init__(self, shim):
    self.shim = shim

  def integrate(self, state, dims, grid, sources, near, trunc):
    state = np.ascontiguousarray(state, np.int32).copy()
    table = np.zeros(len(sources), SOURCE_DTYPE)
    keep = []
    for s, (d, im, _) in enumerate(sources):
      d = np.ascontiguousarray(d, F32)
      im = None if im is None else np.ascontiguousarray(im, F32)
      keep += [d, im]
      table[s] = (d.ctypes.data if d.size else 0, im.ctypes.data if im is not None and im.size else 0, d.shape[0], d.shape[1])
    params = np.ascontiguousarray(np.stack([p for _, _, p in sources]), F64)
    rc = self.shim.hm_tsdf_integrate(state, *dims, np.asarray(grid, F64), table, params, len(sources),
                                     np.array([near, trunc, 1.0 / trunc], F64))
    assert rc == 0
    return state

  def extract(self, state, dims, grid, min_weight, vertices, colours, faces, capacity_v, capacity_f):
    """Fills the given buffers up to the capacities (the buffers have guard rows beyond them); -> (V, F, cell_vertex)."""
    state, grid = np.ascontiguousarray(state, np.int32), np.asarray(grid, F64)
    nodes, cells = state.shape[1], max(dims[0] - 1, 0) * max(dims[1] - 1, 0) * max(dims[2] - 1, 0)
    active, cell_vertex = np.full(cells, 9, np.uint8), np.full(cells, -7, np.int32)
    assert self.shim.hm_mesh_vertex_mask(state, *dims, min_weight, active) == 0
    assert self.shim.hm_mesh_vertex_emit(state, *dims, grid, min_weight, capacity_v, cell_vertex, vertices, colours) == 0
    keep = np.full(3 * nodes, 9, np.uint8)
    assert self.shim.hm_mesh_face_mask(state, *dims, min_weight, cell_vertex, keep) == 0
    assert self.shim.hm_mesh_face_emit(state, *dims, min_weight, cell_vertex, capacity_f, faces) == 0
    if cells == 0:
      return 0, 0, cell_vertex
    assert np.array_equal(active.astype(bool), cell_vertex >= 0)
    return int(active.sum()), 2 * int(keep.sum()), cell_vertex


class DeviceBackend:
  device = "cuda"

  def _up(self, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

  def integrate(self, state, dims, grid, sources, near, trunc):
    d_state = self._up(np.ascontiguousarray(state, np.int32))
    depths = [self._up(np.ascontiguousarray(d, F32)) for d, _, _ in sources]
    images = [self._up(None if im is None else np.ascontiguousarray(im, F32)) for _, im, _ in sources]
    table = (_lib.GsrTsdfSource * len(sources))(*[
        _lib.GsrTsdfSource(depth=_lib.ptr(d), image=_lib.ptr(im), H=d.shape[0], W=d.shape[1]) for d, im in zip(depths, images)])
    params = np.ascontiguousarray(np.stack([p for _, _, p in sources]), F64)
    grid, tsdf = np.asarray(grid, F64), np.array([near, trunc, 1.0 / trunc], F64)
    _lib.call("gsr_tsdf_integrate", _lib.ptr(d_state), *dims, grid.ctypes.data, table, params.ctypes.data, len(sources),
              tsdf.ctypes.data, _lib.current_stream_ptr())
    return d_state.cpu().numpy()

  def _offsets(self, mask):
    n, block = mask.numel(), _lib.CONSTANTS["GSR_COMPACT_BLOCK"]
    offsets = torch.empty((n + block - 1) // block, dtype=torch.int32, device="cuda")
    total = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = _lib.workspace(int(_lib.load().gsr_compact_workspace_bytes(n)), "cuda")
    _lib.call("gsr_compact_offsets", mask.data_ptr(), n, offsets.data_ptr(), total.data_ptr(), _lib.ptr(ws), ws.numel(),
              _lib.current_stream_ptr())
    return offsets, int(total.item())

  def extract(self, state, dims, grid, min_weight, vertices, colours, faces, capacity_v, capacity_f):
    d_state, grid = self._up(np.ascontiguousarray(state, np.int32)), np.asarray(grid, F64)
    nodes, cells = state.shape[1], max(dims[0] - 1, 0) * max(dims[1] - 1, 0) * max(dims[2] - 1, 0)
    stream = _lib.current_stream_ptr()
    if cells == 0:                                                          # every entry point returns before a launch
      head = (_lib.ptr(d_state), *dims)
      _lib.call("gsr_mesh_vertex_mask", *head, min_weight, None, stream)
      _lib.call("gsr_mesh_vertex_emit", *head, grid.ctypes.data, min_weight, None, 4, None, None, None, stream)
      _lib.call("gsr_mesh_face_mask", *head, min_weight, None, None, stream)
      _lib.call("gsr_mesh_face_emit", *head, min_weight, None, None, 4, None, stream)
      return 0, 0, np.zeros(0, np.int32)
    active = torch.full((cells,), 9, dtype=torch.uint8, device="cuda")
    cell_vertex = torch.full((cells,), -7, dtype=torch.int32, device="cuda")
    d_vertices, d_colours, d_faces = self._up(vertices), self._up(colours), self._up(faces)
    _lib.call("gsr_mesh_vertex_mask", d_state.data_ptr(), *dims, min_weight, active.data_ptr(), stream)
    offsets, V = self._offsets(active)
    assert offsets.numel() >= 3 or cells < 513
    _lib.call("gsr_mesh_vertex_emit", d_state.data_ptr(), *dims, grid.ctypes.data, min_weight, offsets.data_ptr(),
              capacity_v, cell_vertex.data_ptr(), _lib.ptr(d_vertices), _lib.ptr(d_colours), stream)
    keep = torch.full((3 * nodes,), 9, dtype=torch.uint8, device="cuda")
    _lib.call("gsr_mesh_face_mask", d_state.data_ptr(), *dims, min_weight, cell_vertex.data_ptr(), keep.data_ptr(), stream)
    offsets, kept = self._offsets(keep)
    _lib.call("gsr_mesh_face_emit", d_state.data_ptr(), *dims, min_weight, cell_vertex.data_ptr(), offsets.data_ptr(),
              capacity_f, _lib.ptr(d_faces), stream)
    vertices[...], colours[...], faces[...] = d_vertices.cpu().numpy(), d_colours.cpu().numpy(), d_faces.cpu().numpy()
    assert np.array_equal(active.cpu().numpy().astype(bool), cell_vertex.cpu().numpy() >= 0)
    return V, 2 * kept, cell_vertex.cpu().numpy()


# ---- inputs ----------------------------------------------------------------------------------------------------------
SOURCE_SHAPES = fusion_cases.SOURCE_SHAPES                       # (7, 11) and (5, 17)


def world_params(T, projection):
  """The 16 doubles of one view: the rows of src_t_world, then fx fy cx cy."""
  return np.concatenate([fusion_oracle.pose(T).reshape(12), np.asarray(projection, F32).astype(F64)])


def random_views(rng, S, images="some", special=True):
  """S views of the two shapes in turn looking down +z at the grid from near the origin, a few turned far enough to put
  part of the grid behind them: [(depth, image or None, params16)] and their (T, projection, H, W)."""
  out, cams = [], []
  for s in range(S):
    H, W = SOURCE_SHAPES[s % 2]
    T = pose(rng, angle=0.9 if s % 5 == 4 else 0.25, shift=0.5)
    if s % 7 == 3:
      T[2, 3] = F32(-3.5)                                         # the camera stands inside the grid: nodes behind it
    proj = intrinsics(H, W, 0.6)
    image = None
    if images == "all" or (images == "some" and s % 3 != 2):
      image = rng.uniform(-0.2, 1.2, (H, W, 3)).astype(F32)
      image[0, 0] = (np.nan, 0.5, 1.0)
      image[0, 1] = (np.inf, -np.inf, 1.0 / 510)
    out.append((depth_map(rng, H, W, 2.5, 5.0, special=special), image, world_params(T, proj)))
    cams.append((T, proj, H, W))
  return out, cams


def random_state(rng, nodes, empty_share=0.04, spread=30000):
  """A state with every combination: nodes without a sample (n = 0, sum_d = 0), zero sums, colourless nodes (the first
  fifth of them all, so that whole cells are without colour)."""
  state = np.zeros((6, nodes), np.int32)
  state[1] = rng.integers(1, 21, nodes)
  state[0] = rng.integers(-spread, spread + 1, nodes) * state[1]
  state[0][rng.random(nodes) < 0.03] = 0
  state[2] = np.minimum(rng.integers(0, 4, nodes), state[1])
  state[3:6] = rng.integers(0, 256, (3, nodes)) * state[2]
  state[2:6, :nodes // 5] = 0
  gone = rng.random(nodes) < empty_share
  state[:, gone] = 0
  return state


# ---- integration -----------------------------------------------------------------------------------------------------
NEAR, TRUNC = 0.1, 0.75


def _integrate_one_call(backend, S, images="some", strip_images=False):
  rng = np.random.default_rng(200 + S)
  sources, _ = random_views(rng, S, images)
  if strip_images:
    sources = [(d, None, p) for d, _, p in sources]
  start = random_state(rng, NODES)
  want = oracle.integrate(start, DIMS, GRID, sources, NEAR, TRUNC)
  delta = want.astype(np.int64) - start
  same(backend.integrate(start, DIMS, GRID, sources, NEAR, TRUNC), want)
  touched = delta[1] > 0
  assert touched.any() and (delta[2] <= delta[1]).all()
  if S == 1:
    assert (~touched).any()                                                 # a node that is not reached keeps its integers
  if S == 16:
    assert (delta[2] < delta[1]).any() and (delta[2] > 0).any()           # samples beyond +trunc carry no colour
    assert (delta[0] < 0).any() and (delta[0] > 0).any() and delta[1].max() > 4
  return delta


def integrate_1_source(backend):
  _integrate_one_call(backend, 1)


def integrate_16_sources(backend):
  _integrate_one_call(backend, 16)


def integrate_with_and_without_images(backend):
  with_images, without = _integrate_one_call(backend, 2, "all"), _integrate_one_call(backend, 2, "all", strip_images=True)
  assert np.array_equal(with_images[:3], without[:3])                      # the geometry does not look at the image
  assert np.array_equal(without[3], 255 * without[2]) and not np.array_equal(with_images[3:], without[3:])


def integrate_behind_and_outside(backend):
  """A camera inside the grid looking down +z: the nodes at or behind its near plane and those outside its image take
  nothing.  The depth map is near (1.0, the camera at z = 3.25), so the nodes that count lie around and behind the
  surface, with diff from +0.75 down to -0.75 = -trunc."""
  T = np.eye(4, dtype=F32)
  T[2, 3] = F32(-3.25)                                             # the camera centre at z = 3.25
  H, W = 7, 11
  proj = np.array([6.0, 6.0, 5.5, 3.5], F32)
  depth = np.full((H, W), 1.0, F32)
  sources = [(depth, None, world_params(T, proj))]
  start = np.zeros((6, NODES), np.int32)
  want = oracle.integrate(start, DIMS, GRID, sources, NEAR, TRUNC)
  X, Y, Z = oracle.positions(DIMS, GRID)
  behind = Z - 3.25 <= NEAR
  us = 6.0 * X / np.where(behind, 1.0, Z - 3.25) + 5.5
  outside = ~behind & ((us < 0) | (us >= W))
  assert behind.sum() > 100 and outside.sum() > 100 and want[1][behind].sum() == 0 and want[1][outside].sum() == 0
  assert want[1].sum() > 20
  same(backend.integrate(start, DIMS, GRID, sources, NEAR, TRUNC), want)


def integrate_trunc_boundaries(backend):
  """One node on the axis of a one-pixel view of depth 2, trunc 1/4: a node at depth 2.25 has diff = -trunc and counts
  with Q = -32768, one double further it is skipped; at 1.75 diff = +trunc and the sample carries colour, one double
  nearer it counts without colour."""
  depth = np.full((1, 1), 2.0, F32)
  params = np.concatenate([np.eye(3, 4).reshape(12), [1.0, 1.0, 0.5, 0.5]]).astype(F64)
  rows = [(2.25, [-32768, 1, 1, 255, 255, 255]), (np.nextafter(2.25, np.inf), [0, 0, 0, 0, 0, 0]),
          (np.nextafter(2.25, 0), [-32768, 1, 1, 255, 255, 255]), (1.75, [32768, 1, 1, 255, 255, 255]),
          (np.nextafter(1.75, 0), [32768, 1, 0, 0, 0, 0]), (np.nextafter(1.75, np.inf), [32768, 1, 1, 255, 255, 255]),
          (2.0, [0, 1, 1, 255, 255, 255]), (2.0 - 2.0 ** -18, [1, 1, 1, 255, 255, 255]), (2.0 + 2.0 ** -18, [0, 1, 1, 255, 255, 255])]
  for z, expected in rows:
    grid = np.array([1.0, 0.0, 0.0, z], F64)
    want = oracle.integrate(np.zeros((6, 1), np.int32), (1, 1, 1), grid, [(depth, None, params)], 0.1, 0.25)
    assert want[:, 0].tolist() == expected, (z, want[:, 0])
    same(backend.integrate(np.zeros((6, 1), np.int32), (1, 1, 1), grid, [(depth, None, params)], 0.1, 0.25), want)


def integrate_17_views_any_order_and_chunking(backend):
  """Through the package: 17 views are two launches; the reversed order, one view at a time and chunks of five give the
  same integers."""
  rng = np.random.default_rng(17)
  sources, cams = random_views(rng, 17)
  want = oracle.integrate(np.zeros((6, NODES), np.int32), DIMS, GRID, sources, NEAR, TRUNC)
  dev = backend.device
  views = [(torch.from_numpy(d).to(dev), None if im is None else torch.from_numpy(im).to(dev), camera(T, proj, H, W, NEAR, dev))
           for (d, im, _), (T, proj, H, W) in zip(sources, cams)]

  def volume(order, step):
    v = sta.TsdfVolume(GRID[1:], DIMS, GRID[0], dev, trunc=TRUNC)
    for b in range(0, len(order), step):
      part = [views[i] for i in order[b:b + step]]
      v.integrate([p[0] for p in part], [p[1] for p in part], [p[2] for p in part])
    assert v.views == 17
    return v.state.cpu().numpy()
  same(volume(list(range(17)), 17), want)
  same(volume(list(range(16, -1, -1)), 1), want)
  same(volume(list(rng.permutation(17)), 5), want)
  near_2 = oracle.integrate(np.zeros((6, NODES), np.int32), DIMS, GRID, sources, [NEAR] * 9 + [3.0] * 8, TRUNC)
  assert not np.array_equal(near_2, want)                                   # views with another near plane: their own launch
  v = sta.TsdfVolume(GRID[1:], DIMS, GRID[0], dev, trunc=TRUNC)
  cameras = [camera(T, proj, H, W, NEAR if i < 9 else 3.0, dev) for i, (T, proj, H, W) in enumerate(cams)]
  v.integrate([p[0] for p in views], [p[1] for p in views], cameras)
  same(v.state.cpu().numpy(), near_2)


# ---- extraction ------------------------------------------------------------------------------------------------------
GUARD = 5                              # sentinel rows beyond the counts; the buffers hold every row whatever the capacity,
#                                        so a write past the capacity shows and still lands inside the buffer


def _extract(backend, state, dims, grid, min_weight=1, short_vertices=0, short_faces=0):
  v, c, f, cell_vertex = oracle.extract(state, dims, grid, min_weight)
  V, F = len(v), len(f)
  cap_v, cap_f = max(V - short_vertices, 0), max(F - short_faces, 0)        # the capacities
  vertices, colours = np.full((V + GUARD, 3), -7.0, F32), np.full((V + GUARD, 3), 99, np.uint8)
  faces = np.full((F + GUARD, 3), -5, np.int32)
  want = [x.copy() for x in (vertices, colours, faces)]
  want[0][:cap_v], want[1][:cap_v], want[2][:cap_f] = v[:cap_v], c[:cap_v], f[:cap_f]      # rows at and beyond keep the sentinel
  got_V, got_F, got_cells = backend.extract(state, dims, grid, min_weight, vertices, colours, faces, cap_v, cap_f)
  assert (got_V, got_F) == (V, F)
  same(got_cells, cell_vertex)                                              # whatever the capacity
  for g, w in zip((vertices, colours, faces), want):
    same(g, w)
  return v, c, f


def extract_random(backend):
  """Random states: heavily ambiguous cells, nodes without samples, zero sums (not negative), colourless corners."""
  rng = np.random.default_rng(61)
  state = random_state(rng, NODES)
  v, c, f = _extract(backend, state, DIMS, GRID)
  assert len(v) > 256 and len(f) > 2 * 256 and (c == 255).all(1).any() and (c != 255).any()
  v2, _, f2 = _extract(backend, state, DIMS, GRID, min_weight=2)
  assert 0 < len(v2) < len(v) and 0 < len(f2) < len(f)
  dense = random_state(rng, NODES, empty_share=0.0)
  v3, _, f3 = _extract(backend, dense, DIMS, GRID)
  assert len(f3) > 2 * 256                                                  # kept edges in more than one block


def extract_nothing(backend):
  """No cell (a flat grid, no node at all), and cells without an active one: V = F = 0."""
  for dims in ((13, 9, 1), (1, 1, 1), (0, 0, 0), (5, 0, 3)):
    nodes = dims[0] * dims[1] * dims[2]
    v, _, f = _extract(backend, np.ones((6, nodes), np.int32), dims, GRID)
    assert len(v) == 0 and len(f) == 0
  rng = np.random.default_rng(62)
  outside = random_state(rng, NODES, empty_share=0.0)
  outside[0] = np.abs(outside[0])                                           # no negative node
  unseen = random_state(rng, NODES)
  for state, min_weight in ((outside, 1), (np.zeros((6, NODES), np.int32), 1), (unseen, 21)):
    v, _, f = _extract(backend, state, DIMS, GRID, min_weight)
    assert len(v) == 0 and len(f) == 0
  mesh = sta.TsdfVolume(GRID[1:], (13, 9, 1), GRID[0], backend.device).extract()
  assert (mesh.num_vertices, mesh.num_faces) == (0, 0) and mesh.faces.dtype is torch.int32
  mesh = sta.TsdfVolume(GRID[1:], DIMS, GRID[0], backend.device).extract()
  assert (mesh.num_vertices, mesh.num_faces) == (0, 0) and mesh.vertices.shape == (0, 3)


def extract_short_capacity(backend):
  """Capacities below the counts: the rows below them are the oracle's and nothing is written at or past them (the
  buffers go on, filled with sentinels, for all the rows there are and GUARD more).  An odd face capacity cuts a quad: its first triangle is written, row
  2 r + 1 == capacity is not; an even one ends between two quads."""
  state = random_state(np.random.default_rng(63), NODES)
  _, _, f = _extract(backend, state, DIMS, GRID, short_vertices=300, short_faces=301)
  assert len(f) % 2 == 0 and (len(f) - 301) % 2 == 1 and len(f) > 301       # the capacity is odd
  _extract(backend, state, DIMS, GRID, short_vertices=1, short_faces=2)
  _extract(backend, state, DIMS, GRID, short_vertices=10 ** 6, short_faces=10 ** 6)      # capacity 0


SPHERE_DIMS, SPHERE_VOXEL, SPHERE_TRUNC = (33, 33, 33), 0.08, 0.32
SPHERE_GRID = np.array([SPHERE_VOXEL, -1.28, -1.28, -1.28], F64)


def check_closed_sphere(v, f, centre):
  closed, oriented, euler = oracle.closed_manifold_report(f)
  normals, centroids = oracle.signed_volume_normals(v, f)
  deviation = np.abs(np.linalg.norm(v.astype(F64) - centre, axis=1) - 1.0).max() / SPHERE_VOXEL
  print(f"sphere at {centre}: V {len(v)} F {len(f)} euler {euler} max deviation {deviation:.4f} voxel")
  assert closed and oriented and euler == 2
  assert len(np.unique(f)) == len(v)                                        # every vertex is used
  assert (np.linalg.norm(normals, axis=1) > 0).all()                        # no zero-area triangle
  assert ((normals * (centroids - centre)).sum(1) > 0).all()                # outward
  assert deviation < 0.1


def _sphere(backend, centre):
  centre = np.asarray(centre, F64)
  state = oracle.sphere_state(SPHERE_DIMS, SPHERE_GRID, centre, 1.0, SPHERE_TRUNC)
  v, _, f = _extract(backend, state, SPHERE_DIMS, SPHERE_GRID)
  check_closed_sphere(v, f, centre)
  volume = sta.TsdfVolume(SPHERE_GRID[1:], SPHERE_DIMS, SPHERE_VOXEL, backend.device)      # ... and through the package
  volume.state.copy_(torch.from_numpy(state))
  mesh = volume.extract()
  same(mesh.vertices.cpu().numpy(), v)
  same(mesh.faces.cpu().numpy(), f)
  assert (mesh.colors == 255).all()


def sphere_centred(backend):
  _sphere(backend, (0.0, 0.0, 0.0))


def sphere_off_centre(backend):
  _sphere(backend, (0.013, -0.021, 0.034))


# ---- the whole meshing through the package ---------------------------------------------------------------------------
def look_at(eye):
  """A (4, 4) float32 world-to-camera pose at `eye` looking at the origin (+z forward)."""
  eye = np.asarray(eye, F64)
  z = -eye / np.linalg.norm(eye)
  up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
  x = np.cross(up, z)
  x /= np.linalg.norm(x)
  y = np.cross(z, x)
  T = np.eye(4)
  T[:3, :3] = np.stack([x, y, z])
  T[:3, 3] = -T[:3, :3] @ eye
  return T.astype(F32)


def sphere_views(size=64, focal=70.4, distance=3.0):
  """Analytic z-depth maps of the unit sphere from 14 cameras: the six axes and the eight cube diagonals."""
  eyes = [np.eye(3)[a] * s for a in range(3) for s in (1, -1)] + [np.array([a, b, c]) / np.sqrt(3.0) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
  proj = np.array([focal, focal, size / 2, size / 2], F32)
  j, i = np.meshgrid(np.arange(size) + 0.5, np.arange(size) + 0.5)
  rays = np.stack([(j - size / 2) / focal, (i - size / 2) / focal, np.ones_like(j)], -1)      # camera space, z = 1
  depths, images, cams = [], [], []
  for eye in eyes:
    T = look_at(distance * np.asarray(eye, F64))
    centre = T.astype(F64)[:3, 3]                                    # the sphere's centre in camera space
    a, b, c = (rays * rays).sum(-1), -2.0 * (rays @ centre), centre @ centre - 1.0
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
      z = (-b - np.sqrt(disc)) / (2 * a)                             # rays have z = 1: the parameter is the z-depth
    depths.append(np.where(disc > 0, z, 0.0).astype(F32))
    images.append(np.broadcast_to(0.5 + 0.5 * np.asarray(eye, F64), (size, size, 3)).astype(F32).copy())
    cams.append((T, proj, size, size))
  return depths, images, cams


def mesh_of_sphere_views(backend):
  """mesh_depth_maps on 14 analytic views into the 33^3 grid against the oracle.  The projective distance leaves
  silhouette artefacts, so the mesh is not asserted closed: every vertex lies within one voxel of the sphere and at
  least 99 % of the triangles face outward."""
  depths, images, cams = sphere_views()
  dev = backend.device
  cameras = [camera(T, proj, H, W, 0.1, dev) for T, proj, H, W in cams]
  config = sta.TsdfConfig(voxel_size=SPHERE_VOXEL, bounds=((-1.28, -1.28, -1.28), (1.28, 1.28, 1.28)), near=0.1)
  mesh = sta.mesh_depth_maps([torch.from_numpy(d).to(dev) for d in depths], [torch.from_numpy(i).to(dev) for i in images],
                             cameras, config)
  sources = [(d, im, world_params(T, proj)) for d, im, (T, proj, _, _) in zip(depths, images, cams)]
  state = oracle.integrate(np.zeros((6, 33 ** 3), np.int32), SPHERE_DIMS, SPHERE_GRID, sources, 0.1, SPHERE_TRUNC)
  v, c, f, _ = oracle.extract(state, SPHERE_DIMS, SPHERE_GRID, 1)
  deviation = np.abs(np.linalg.norm(v.astype(F64), axis=1) - 1.0).max() / SPHERE_VOXEL
  normals, centroids = oracle.signed_volume_normals(v, f)
  outward = ((normals * centroids).sum(1) > 0).mean()
  print(f"14 views: V {len(v)} F {len(f)} max deviation {deviation:.3f} voxel, outward {100 * outward:.2f} %")
  same(mesh.vertices.cpu().numpy(), v)
  same(mesh.colors.cpu().numpy(), c)
  same(mesh.faces.cpu().numpy(), f)
  assert len(f) > 4000 and deviation < 1.0 and outward >= 0.99
  assert len(np.unique(c, axis=0)) > 14                               # the views' colours blend


CASES = {f.__name__: f for f in (
    integrate_1_source, integrate_16_sources, integrate_with_and_without_images, integrate_behind_and_outside,
    integrate_trunc_boundaries, integrate_17_views_any_order_and_chunking, extract_random, extract_nothing,
    extract_short_capacity, sphere_centred, sphere_off_centre, mesh_of_sphere_views)}
