"""The depth-fusion cases that tests/test_fusion_host.py runs on the host shim and tests/test_gpu_fusion.py on the device:
each is a function of a backend (where the arrays live and which library is called) that compares with
tests/fusion_oracle.py exactly, bit for bit.  The raw entry points are used where the package's functions do not reach
(one call of S sources, `base` and `capacity` of the emission); the rest goes through the package."""

import numpy as np
import torch

import fusion_oracle as oracle
import splat_trainer_amd as sta
from splat_trainer_amd import _lib, fusion

F32, F64 = np.float32, np.float64
SOURCE_DTYPE = np.dtype([("depth", "<u8"), ("H", "<i4"), ("W", "<i4")])       # GsrFuseSource: 16 bytes
DENORMAL = F32(1e-41)


# ---- backends --------------------------------------------------------------------------------------------------------
class HostBackend:
  device = "cpu"

  def __init__(self, shim):
    self.shim = shim

  def check(self, ref, intr, sources, near, rel_tol, counts):
    table = np.zeros(len(sources), SOURCE_DTYPE)
    depths = [np.ascontiguousarray(d, F32) for d, _ in sources]
    for s, d in enumerate(depths):
      table[s] = (d.ctypes.data if d.size else 0, d.shape[0], d.shape[1])
    params = np.ascontiguousarray(np.stack([p for _, p in sources]), F64)
    rc = self.shim.hm_fuse_check(ref, ref.shape[0], ref.shape[1], np.asarray(intr, F64), table, params, len(sources),
                                 np.array([near, rel_tol], F64), counts)
    assert rc == 0
    return counts

  def emit(self, ref, counts, image, intr, world, min_agree, max_violate, base, capacity, points, colours, agree):
    rc = self.shim.hm_fuse_emit(ref, counts, image, ref.shape[0], ref.shape[1], np.asarray(intr, F64),
                                np.ascontiguousarray(world, F64).reshape(12), min_agree, max_violate, base, capacity,
                                points, colours, agree)
    assert rc == 0
    kept = int(oracle.keep_mask(ref, counts, min_agree, max_violate).sum())
    mask = np.zeros(ref.size, np.uint8)
    assert self.shim.hm_fuse_mask(ref, counts, ref.shape[0], ref.shape[1], min_agree, max_violate, mask) == 0
    assert int(mask.sum()) == kept
    return kept


class DeviceBackend:
  device = "cuda"

  def _up(self, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

  def check(self, ref, intr, sources, near, rel_tol, counts):
    d_ref, d_counts = self._up(ref), self._up(counts)
    depths = [self._up(np.ascontiguousarray(d, F32)) for d, _ in sources]
    table = (_lib.GsrFuseSource * len(sources))(*[_lib.GsrFuseSource(depth=_lib.ptr(d), H=d.shape[0], W=d.shape[1])
                                                  for d in depths])
    params = np.ascontiguousarray(np.stack([p for _, p in sources]), F64)
    intr, tol = np.asarray(intr, F64), np.array([near, rel_tol], F64)
    _lib.call("gsr_fuse_check", d_ref.data_ptr(), ref.shape[0], ref.shape[1], intr.ctypes.data, table, params.ctypes.data,
              len(sources), tol.ctypes.data, d_counts.data_ptr(), _lib.current_stream_ptr())
    counts[...] = d_counts.cpu().numpy()
    return counts

  def emit(self, ref, counts, image, intr, world, min_agree, max_violate, base, capacity, points, colours, agree):
    H, W = ref.shape
    n_px = H * W
    d_ref, d_counts, d_image = self._up(ref), self._up(counts), self._up(image)
    d_points, d_colours, d_agree = self._up(points), self._up(colours), self._up(agree)
    keep = torch.empty(n_px, dtype=torch.uint8, device="cuda")
    stream = _lib.current_stream_ptr()
    _lib.call("gsr_fuse_mask", d_ref.data_ptr(), d_counts.data_ptr(), H, W, min_agree, max_violate, keep.data_ptr(), stream)
    block = _lib.CONSTANTS["GSR_COMPACT_BLOCK"]                            # the header's number, which the package takes
    assert fusion.COMPACT_BLOCK == block
    offsets = torch.empty((n_px + block - 1) // block, dtype=torch.int32, device="cuda")
    total = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = _lib.workspace(int(_lib.load().gsr_compact_workspace_bytes(n_px)), "cuda")
    _lib.call("gsr_compact_offsets", keep.data_ptr(), n_px, offsets.data_ptr(), total.data_ptr(), _lib.ptr(ws), ws.numel(),
              stream)
    kept_in_block = np.add.reduceat(oracle.keep_mask(ref, counts, min_agree, max_violate).reshape(-1).astype(np.int64),
                                    np.arange(0, n_px, block))
    assert len(kept_in_block) >= 3                                         # gsr_compact_offsets counts by blocks of that size
    assert offsets.cpu().tolist() == (np.cumsum(kept_in_block) - kept_in_block).tolist()
    intr, world = np.asarray(intr, F64), np.ascontiguousarray(world, F64).reshape(12)
    _lib.call("gsr_fuse_emit", d_ref.data_ptr(), d_counts.data_ptr(), _lib.ptr(d_image), H, W, intr.ctypes.data,
              world.ctypes.data, min_agree, max_violate, offsets.data_ptr(), base, capacity, _lib.ptr(d_points),
              _lib.ptr(d_colours), _lib.ptr(d_agree), stream)
    points[...], colours[...], agree[...] = d_points.cpu().numpy(), d_colours.cpu().numpy(), d_agree.cpu().numpy()
    assert np.array_equal(keep.cpu().numpy().astype(bool), oracle.keep_mask(ref, counts, min_agree, max_violate).reshape(-1))
    return int(total.item())


def same(a, b):
  """Equal shapes, dtypes and bytes (NaN payloads included)."""
  a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
  assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
  assert a.tobytes() == b.tobytes(), f"{int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


# ---- inputs ----------------------------------------------------------------------------------------------------------
def depth_map(rng, H, W, lo=3.0, hi=5.0, special=True):
  d = rng.uniform(lo, hi, (H, W)).astype(F32)
  if special and d.size >= 12:                           # invalid and odd values at fixed places
    flat = d.reshape(-1)
    flat[[1, 5, 7, 9, 11]] = [0.0, -2.0, np.nan, np.inf, DENORMAL]
    flat[3] = -np.inf
  return d


def intrinsics(H, W, scale=1.0):
  return np.array([scale * W, scale * W + 1.5, W / 2 + 0.25, H / 2 - 0.125], F32)


def pose(rng, angle=0.05, shift=0.3):
  """A (4, 4) float32 world-to-camera pose near the identity (a rotation matrix to float32 accuracy: the contract
  applies whatever 3 x 4 it is given)."""
  a, b, c = rng.uniform(-angle, angle, 3)
  Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
  Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
  Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
  T = np.eye(4)
  T[:3, :3] = Rx @ Ry @ Rz
  T[:3, 3] = rng.uniform(-shift, shift, 3)
  return T.astype(F32)


def camera(T, projection, H, W, near=0.1, device="cpu"):
  return sta.CameraParams(T_camera_world=torch.from_numpy(np.asarray(T, F32)).to(device),
                          projection=torch.from_numpy(np.asarray(projection, F32)).to(device), image_size=(W, H),
                          near_plane=near)


REF_H, REF_W = 9, 13
SOURCE_SHAPES = ((7, 11), (5, 17))


def random_sources(rng, S, ref_T, special=True):
  """S sources (depth, params16) of the two shapes in turn, and their (T, projection, H, W)."""
  out, cams = [], []
  for s in range(S):
    H, W = SOURCE_SHAPES[s % 2]
    T, proj = pose(rng), intrinsics(H, W, 0.9)
    out.append((depth_map(rng, H, W, special=special), oracle.source_params(T, ref_T, proj)))
    cams.append((T, proj, H, W))
  return out, cams


# ---- consistency -----------------------------------------------------------------------------------------------------
def _consistency_shapes(backend, S):
  rng = np.random.default_rng(100 + S)
  ref, ref_T, ref_proj = depth_map(rng, REF_H, REF_W), pose(rng), intrinsics(REF_H, REF_W)
  sources, _ = random_sources(rng, S, ref_T)
  intr = oracle.ref_intrinsics(ref_proj)
  start = rng.integers(0, 3, (REF_H, REF_W, 2)).astype(np.uint8)          # the counters accumulate
  want = oracle.consistency(ref, intr, sources, 0.1, 0.08, start)
  got = backend.check(ref, intr, sources, 0.1, 0.08, start.copy())
  same(got, want)
  delta = want.astype(int) - start
  invalid = ~oracle.valid(ref.astype(F64))
  assert invalid.sum() == 5 and (delta[invalid] == 0).all()                # 0, negative, NaN, +-inf: no part
  assert oracle.valid(np.array([DENORMAL], F64))[0]                        # the denormal depth is a valid one
  if S == 16:                                                              # every outcome occurs
    assert delta[:, :, 0].sum() > 0 and delta[:, :, 1].sum() > 0 and (delta.sum(-1) < S)[~invalid].any()


def consistency_1_source(backend):
  _consistency_shapes(backend, 1)


def consistency_2_sources(backend):
  _consistency_shapes(backend, 2)


def consistency_16_sources(backend):
  _consistency_shapes(backend, 16)


def consistency_17_sources_chunked(backend):
  """Through the package: 17 sources are two calls, and sources with another near plane a call of their own."""
  rng = np.random.default_rng(7)
  ref, ref_T, ref_proj = depth_map(rng, REF_H, REF_W), pose(rng), intrinsics(REF_H, REF_W)
  sources, cams = random_sources(rng, 17, ref_T)
  nears = [0.1] * 17
  nears[4], nears[5] = 3.9, 3.9
  want = oracle.consistency(ref, oracle.ref_intrinsics(ref_proj), sources, nears, 0.08)
  dev = backend.device
  pairs = [(torch.from_numpy(d).to(dev), camera(T, proj, H, W, near, dev))
           for (d, _), (T, proj, H, W), near in zip(sources, cams, nears)]
  got = sta.depth_consistency(torch.from_numpy(ref).to(dev), camera(ref_T, ref_proj, REF_H, REF_W, device=dev), pairs, 0.08)
  same(got.cpu().numpy(), want)
  one_near = oracle.consistency(ref, oracle.ref_intrinsics(ref_proj), sources, 3.9, 0.08)
  assert not np.array_equal(one_near, oracle.consistency(ref, oracle.ref_intrinsics(ref_proj), sources, 0.1, 0.08))
  got = sta.depth_consistency(torch.from_numpy(ref).to(dev), camera(ref_T, ref_proj, REF_H, REF_W, device=dev), pairs, 0.08,
                              near=3.9)
  same(got.cpu().numpy(), one_near)


def consistency_behind_the_source(backend):
  """A source 4 units ahead of the reference: points nearer than 4 + near lie behind it or before its near plane."""
  rng = np.random.default_rng(8)
  ref = depth_map(rng, REF_H, REF_W, 3.0, 5.0)
  proj = np.array([8.0, 8.0, 6.5, 4.5], F32)
  src_T = np.eye(4, dtype=F32)
  src_T[2, 3] = -4.0
  src = np.full((40, 60), 0.5, F32)                            # wide: a point close to the source projects far out
  params = oracle.source_params(src_T, np.eye(4, dtype=F32), np.array([2.0, 2.0, 30.0, 20.0], F32))
  intr = oracle.ref_intrinsics(proj)
  want = oracle.consistency(ref, intr, [(src, params)], 0.1, 0.5)
  behind = oracle.valid(ref.astype(F64)) & (ref.astype(F64) - 4.0 <= 0.1)
  assert behind.sum() > 10 and (~behind).sum() > 10 and (want[behind] == 0).all() and want[~behind].sum() > 0
  same(backend.check(ref, intr, [(src, params)], 0.1, 0.5, np.zeros((REF_H, REF_W, 2), np.uint8)), want)


def consistency_borders(backend):
  """us = j - 1 exactly: column 0 falls on us = -1, column 1 on the border us = 0 (inside), column Ws + 1 on us = Ws
  (outside).  Likewise the rows."""
  Hs, Ws = 4, 6
  ref = np.full((Hs + 3, Ws + 3), 2.0, F32)                     # a power of two: x d (1 / d) = x exactly
  intr = np.array([1.0, 1.0, 0.5, 0.5], F64)                    # x = j, y = i
  params = np.concatenate([np.eye(3, 4).reshape(12), [1.0, 1.0, -1.0, -1.0]]).astype(F64)
  src = np.full((Hs, Ws), 2.0, F32)
  want = oracle.consistency(ref, intr, [(src, params)], 0.1, 0.0)
  inside = np.zeros(ref.shape, bool)
  inside[1:Hs + 1, 1:Ws + 1] = True
  assert np.array_equal(want[:, :, 0], inside.astype(np.uint8)) and not want[:, :, 1].any()
  same(backend.check(ref, intr, [(src, params)], 0.1, 0.0, np.zeros(ref.shape + (2,), np.uint8)), want)


def consistency_exact_boundary(backend):
  """rel = identity, equal intrinsics, rel_tol = 2^-7, depths zs powers of two: a source depth zs (1 +- 2^-7) agrees,
  the next float32 above violates and the next below is occluded (the maps are float32; the vote on doubles one ulp
  beyond is in test_fusion_host.py)."""
  zs = np.array([0.5, 1.0, 2.0, 8.0, 64.0], F32)
  tol = F32(2.0 ** -7)
  hi, lo = zs * (1 + tol), zs * (1 - tol)
  rows = [hi, lo, np.nextafter(hi, F32(np.inf)), np.nextafter(lo, F32(0)), np.nextafter(hi, F32(0)),
          np.nextafter(lo, F32(np.inf))]
  src = np.stack(rows).astype(F32)                                        # (6, 5)
  ref = np.broadcast_to(zs, src.shape).astype(F32).copy()
  intr = np.array([1.0, 1.0, 2.5, 3.0], F64)
  params = np.concatenate([np.eye(3, 4).reshape(12), [1.0, 1.0, 2.5, 3.0]]).astype(F64)
  want = oracle.consistency(ref, intr, [(src, params)], 0.01, float(tol))
  expect = np.zeros(src.shape + (2,), np.uint8)
  expect[[0, 1, 4, 5], :, 0] = 1                                          # on the bound and just inside: agree
  expect[2, :, 1] = 1                                                     # just above: violate; row 3, just below: none
  assert np.array_equal(want, expect)
  same(backend.check(ref, intr, [(src, params)], 0.01, float(tol), np.zeros(src.shape + (2,), np.uint8)), want)


def consistency_saturates(backend):
  ref = np.full((3, 5), 2.0, F32)
  intr = np.array([1.0, 1.0, 2.5, 1.5], F64)
  params = np.concatenate([np.eye(3, 4).reshape(12), [1.0, 1.0, 2.5, 1.5]]).astype(F64)
  agreeing, past = (np.full((3, 5), 2.0, F32), params), (np.full((3, 5), 4.0, F32), params)
  counts = np.zeros((3, 5, 2), np.uint8)
  for _ in range(16):
    counts = backend.check(ref, intr, [agreeing] * 15 + [past], 0.1, 0.01, counts)
  assert (counts[:, :, 0] == 240).all() and (counts[:, :, 1] == 16).all()
  counts = backend.check(ref, intr, [agreeing] * 16, 0.1, 0.01, counts)     # 256 would wrap to 0
  assert (counts[:, :, 0] == 255).all()
  counts[:, :, 1] = 250
  counts = backend.check(ref, intr, [past] * 16, 0.1, 0.01, counts)
  assert (counts[:, :, 0] == 255).all() and (counts[:, :, 1] == 255).all()


# ---- emission --------------------------------------------------------------------------------------------------------
EMIT_H, EMIT_W = 29, 37              # 1073 pixels: five blocks of the 256 gsr_compact_offsets counts by


def _emit(backend, pattern, base=0, short_by=0, with_image=True):
  rng = np.random.default_rng(31)
  ref = depth_map(rng, EMIT_H, EMIT_W)
  counts = np.stack([rng.integers(0, 6, ref.shape), rng.integers(0, 3, ref.shape)], -1).astype(np.uint8)
  flat = counts.reshape(-1, 2)
  if pattern == "none":
    flat[:, 0] = 0
  elif pattern == "all":
    flat[:] = (7, 0)
    ref = depth_map(rng, EMIT_H, EMIT_W, special=False)
  elif pattern == "empty block":
    flat[256:512, 1] = 9                                                  # the second block keeps nothing
  image = rng.uniform(-0.2, 1.2, ref.shape + (3,)).astype(F32) if with_image else None
  if with_image:
    image[0, 0], image[0, 1], image[0, 2] = (np.nan, 0.5, 1.0), (1.0 / 510, 3.0 / 510, 0.0), (np.inf, -np.inf, 0.25)
  proj, T = intrinsics(EMIT_H, EMIT_W), pose(np.random.default_rng(32))
  intr, world = oracle.ref_intrinsics(proj), oracle.rigid_inverse(oracle.pose(T))
  p, c, a = oracle.emit(ref, counts, image, intr, world, 2, 1)
  kept = p.shape[0]
  assert {"none": kept == 0, "all": kept == ref.size}.get(pattern, 0 < kept < ref.size)
  if pattern == "empty block":
    assert not oracle.keep_mask(ref, counts, 2, 1).reshape(-1)[256:512].any()
  rows = base + kept + 5 - short_by                                        # rows of the buffers, `capacity`
  capacity = base + kept - short_by
  points, colours, agree = (np.full((rows, 3), -7.0, F32), np.full((rows, 3), 99, np.uint8), np.full((rows,), 77, np.uint8))
  want = [x.copy() for x in (points, colours, agree)]
  n = max(0, min(kept, capacity - base))
  for w, o in zip(want, (p, c, a)):
    w[base:base + n] = o[:n]                                               # rows outside [base, capacity) keep the sentinel
  got_kept = backend.emit(ref, counts, image, intr, world, 2, 1, base, capacity, points, colours, agree)
  assert got_kept == kept
  for g, w in zip((points, colours, agree), want):
    same(g, w)


def emit_random(backend):
  _emit(backend, "random")


def emit_none(backend):
  _emit(backend, "none")


def emit_all(backend):
  _emit(backend, "all")


def emit_empty_block(backend):
  _emit(backend, "empty block")


def emit_base(backend):
  _emit(backend, "random", base=11)


def emit_short_capacity(backend):
  _emit(backend, "random", base=3, short_by=300)


def emit_without_image(backend):
  _emit(backend, "random", with_image=False)


# ---- voxels ----------------------------------------------------------------------------------------------------------
def _voxel(backend, points, colours, voxel, origin=None):
  points, colours = np.asarray(points, F32).reshape(-1, 3), np.asarray(colours, np.uint8).reshape(-1, 3)
  want = oracle.voxel_downsample(points, colours, voxel, origin or (0.0, 0.0, 0.0))
  got = sta.voxel_downsample(torch.from_numpy(points).to(backend.device), torch.from_numpy(colours).to(backend.device),
                             voxel, origin)
  for g, w in zip(got, want[:3]):
    same(g.cpu().numpy(), w)
  assert want[3] == sorted(set(want[3]))                                   # ascending keys
  return want


def _colours(rng, n):
  return rng.integers(0, 256, (n, 3)).astype(np.uint8)


def voxel_tiny(backend):
  rng = np.random.default_rng(41)
  assert _voxel(backend, np.zeros((0, 3)), np.zeros((0, 3)), 0.5)[0].shape == (0, 3)
  assert _voxel(backend, [[0.3, -0.2, 9.0]], [[1, 2, 3]], 0.5)[2].tolist() == [1]
  p, c, n, _ = _voxel(backend, [[0.30, 0.30, 0.30], [0.40, 0.45, 0.26]], [[0, 255, 1], [1, 254, 2]], 0.5)
  assert n.tolist() == [2] and c.tolist() == [[1, 255, 2]]                 # .5 rounds up
  del rng


def voxel_floor_and_multiples(backend):
  """Exact multiples of the voxel size open a cell; negative coordinates floor, they do not truncate."""
  pts = [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [-0.5, 0.0, 0.0], [-0.25, 0.0, 0.0], [-1e-30, 0.0, 0.0], [0.25, 0.0, 0.0],
         [1.0, -1.0, 0.0], [0.999, -0.001, -0.0]]
  p, c, n, keys = _voxel(backend, pts, _colours(np.random.default_rng(42), len(pts)), 0.5)
  qx = [(k & 0x1fffff) - (1 << 20) for k in keys]
  assert sorted(set(qx)) == [-1, 0, 1, 2] and n.sum() == len(pts)


def voxel_clamps(backend):
  pts = [[3e6, 0.0, 0.0], [2e6, 0.0, 0.0], [-3e6, 1.0, 0.0], [-2e6, 1.0, 0.0], [np.nan, 2.0, 0.0], [0.0, np.nan, np.nan],
         [np.inf, -np.inf, 0.0], [1048575.5, 0.0, 0.0], [-1048576.0, 0.0, 0.0]]
  p, c, n, keys = _voxel(backend, pts, _colours(np.random.default_rng(43), len(pts)), 1.0)
  assert sorted(n.tolist()) == [1, 1, 1, 1, 2, 3]                          # the far points of a side share its last cell


def voxel_word_boundary(backend):
  """Cells that differ only in z, and only in qy by multiples of 2^11: qy's bits straddle the key's two words."""
  pts = [[0.5, 0.5, z + 0.5] for z in (0, 1, -1, 700)] + [[0.5, y * 2048 + 0.5, 0.5] for y in (1, 2, -1, 3, 511, -512)]
  pts += [[0.25, 2048.75, 0.5], [0.5, 0.5, 1.25]]
  p, c, n, keys = _voxel(backend, pts, _colours(np.random.default_rng(44), len(pts)), 1.0)
  assert len(keys) == len(pts) - 2 and len({k & 0xffffffff for k in keys}) < len(keys)      # equal low words, other high


def voxel_long_run(backend):
  """One cell of 5000 points (summed by a whole wave on the device) between short runs."""
  rng = np.random.default_rng(45)
  pts = np.concatenate([rng.uniform(0, 1, (5000, 3)), rng.uniform(-4, 0, (300, 3)), rng.uniform(1, 5, (300, 3)),
                        rng.uniform(2, 3, (40, 3)) * [1, 0, 0] + [0, 7.5, 7.5]]).astype(F32)
  perm = rng.permutation(len(pts))
  p, c, n, _ = _voxel(backend, pts[perm], _colours(rng, len(pts))[perm], 1.0)
  assert 5000 in n.tolist() and 40 in n.tolist()                           # runs above and below the wave threshold


def voxel_random_origin(backend):
  rng = np.random.default_rng(46)
  pts = rng.normal(0, 2.0, (3000, 3)).astype(F32)
  _voxel(backend, pts, _colours(rng, 3000), 0.37, (0.11, -3.3, 1e-3))


# ---- the whole fusion through the package ----------------------------------------------------------------------------
def oracle_fusion(depths, images, cams, sources, rel_tol, min_agree, max_violate, voxel=None):
  """cams: (T, projection, near).  -> (points, colour bytes, agree, kept per view)."""
  parts, kept = [], []
  for v, (T, proj, _) in enumerate(cams):
    intr = oracle.ref_intrinsics(proj)
    src = [(depths[s], oracle.source_params(cams[s][0], T, cams[s][1])) for s in sources[v]]
    counts = oracle.consistency(depths[v], intr, src, [cams[s][2] for s in sources[v]], rel_tol)
    parts.append(oracle.emit(depths[v], counts, images[v], intr, oracle.rigid_inverse(oracle.pose(T)), min_agree, max_violate))
    kept.append(parts[-1][0].shape[0])
  p, c, a = (np.concatenate([x[k] for x in parts]) for k in range(3))
  if voxel is not None:
    p, c, n = oracle.voxel_downsample(p, c, voxel)[:3]
    a = np.minimum(n, 255).astype(np.uint8)                                # a voxel's point count, saturated
  return p, c, a, kept


def check_fusion(got, want):
  cloud, agree = got
  same(cloud.points.cpu().numpy(), want[0])
  same((cloud.colors.cpu() * 255.0).round().to(torch.uint8).numpy(), want[1])
  same(agree.cpu().numpy(), want[2])


def plane_views():
  """Four views of the plane z = 4 seen from cameras shifted along x, of two sizes; view 3 has no valid depth."""
  rng = np.random.default_rng(51)
  sizes = [(12, 16), (12, 16), (10, 20), (12, 16)]
  depths, images, cams = [], [], []
  for v, (H, W) in enumerate(sizes):
    T = np.eye(4, dtype=F32)
    T[0, 3] = -0.25 * v
    d = np.full((H, W), 4.0, F32)
    d[rng.integers(0, H, 6), rng.integers(0, W, 6)] = [2.0, 7.0, np.nan, 0.0, 3.99, 4.02]
    if v == 3:
      d[:] = np.nan
    depths.append(d)
    images.append(rng.uniform(0, 1, (H, W, 3)).astype(F32))
    cams.append((T, np.array([W, W, W / 2, H / 2], F32), 0.1 + 0.1 * v))
  return depths, images, cams


def fusion_of_plane_views(backend):
  depths, images, cams = plane_views()
  dev = backend.device
  cameras = [camera(T, proj, d.shape[0], d.shape[1], near, dev) for (T, proj, near), d in zip(cams, depths)]
  chosen = sta.select_sources(cameras, 2)
  assert chosen == [[1, 2], [0, 2], [1, 3], [2, 1]]                        # nearest first, ties to the lower index
  t_depths, t_images = [torch.from_numpy(d).to(dev) for d in depths], [torch.from_numpy(i).to(dev) for i in images]
  for voxel in (None, 0.3):
    config = sta.FusionConfig(rel_tol=0.01, min_agree=1, max_violate=0, num_sources=2, voxel_size=voxel)
    want = oracle_fusion(depths, images, cams, chosen, 0.01, 1, 0, voxel)
    assert all(k > 0 for k in want[3][:3]) and want[3][3] == 0             # the empty view contributes nothing
    check_fusion(sta.fuse_depth_maps(t_depths, t_images, cameras, config), want)
  lists = [[2], [0, 2, 3], [], [0]]
  want = oracle_fusion(depths, [None] * 4, cams, lists, 0.01, 1, 1)
  config = sta.FusionConfig(rel_tol=0.01, min_agree=1, max_violate=1)
  check_fusion(sta.fuse_depth_maps(t_depths, None, cameras, config, sources=lists), want)
  assert want[3][2] == 0                                                   # no sources: nothing agrees


CASES = {f.__name__: f for f in (
    consistency_1_source, consistency_2_sources, consistency_16_sources, consistency_17_sources_chunked,
    consistency_behind_the_source, consistency_borders, consistency_exact_boundary, consistency_saturates, emit_random,
    emit_none, emit_all, emit_empty_block, emit_base, emit_short_capacity, emit_without_image, voxel_tiny,
    voxel_floor_and_multiples, voxel_clamps, voxel_word_boundary, voxel_long_run, voxel_random_origin,
    fusion_of_plane_views)}
