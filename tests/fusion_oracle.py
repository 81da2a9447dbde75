"""The depth-fusion contract (include/gsplat_hip.h: gsr_fuse_check, gsr_fuse_emit, gsr_voxel_downsample) in numpy
float64, one rounded operation per statement in the order the contract writes them, Python integers for the voxel sums.
No torch, nothing of the package: the native layer and the host shim are both compared with this, bit for bit."""
import numpy as np

F64 = np.float64
HALF = 1 << 20


def valid(d):
  """Above 0 and finite (d: float64 array)."""
  return (d > 0) & np.isfinite(d)


def rigid_inverse(m):
  """[R | t] (3, 4) float64 -> [R^T | -R^T t], t'_k = -((R_0k t_0 + R_1k t_1) + R_2k t_2)."""
  m = np.asarray(m, F64)
  out = np.zeros((3, 4), F64)
  for k in range(3):
    for c in range(3):
      out[k, c] = m[c, k]
    a = m[0, k] * m[0, 3]
    b = m[1, k] * m[1, 3]
    s = a + b
    c2 = m[2, k] * m[2, 3]
    s = s + c2
    out[k, 3] = -s
  return out


def compose(a, b):
  """a after b (3, 4): (a_k0 b_0c + a_k1 b_1c) + a_k2 b_2c, plus a_k3 in the last column."""
  a, b = np.asarray(a, F64), np.asarray(b, F64)
  out = np.zeros((3, 4), F64)
  for k in range(3):
    for c in range(4):
      x = a[k, 0] * b[0, c]
      y = a[k, 1] * b[1, c]
      s = x + y
      z = a[k, 2] * b[2, c]
      s = s + z
      if c == 3:
        s = s + a[k, 3]
      out[k, c] = s
  return out


def pose(T):
  """A (4, 4) float32 pose -> its (3, 4) rows in float64."""
  return np.asarray(T, np.float32).astype(F64)[:3, :4]


def ref_intrinsics(projection):
  fx, fy, cx, cy = np.asarray(projection, np.float32).astype(F64)
  return np.array([F64(1.0) / fx, F64(1.0) / fy, cx, cy], F64)


def source_params(src_T, ref_T, projection):
  """The 16 doubles of one source: src_t_ref = src_t_world after the inverse of ref_t_world, then fx fy cx cy."""
  rel = compose(pose(src_T), rigid_inverse(pose(ref_T)))
  return np.concatenate([rel.reshape(12), np.asarray(projection, np.float32).astype(F64)])


def _unproject(ref_depth, intr):
  H, W = ref_depth.shape
  ifx, ify, cx, cy = (F64(v) for v in intr)
  d = ref_depth.astype(F64)
  j = np.broadcast_to(np.arange(W, dtype=F64)[None, :], (H, W))
  i = np.broadcast_to(np.arange(H, dtype=F64)[:, None], (H, W))
  x = j + F64(0.5)
  y = i + F64(0.5)
  x = x - cx
  y = y - cy
  x = x * ifx
  y = y * ify
  X = x * d
  Y = y * d
  return d, X, Y


def _row(m, X, Y, Z):
  a = F64(m[0]) * X
  b = F64(m[1]) * Y
  c = F64(m[2]) * Z
  s = a + b
  s = s + c
  return s + F64(m[3])


def votes(ref_depth, intr, src_depth, params, near, rel_tol):
  """(agree, violate) bool (H, W) of a float32 reference map against one source (float32 map, 16 doubles)."""
  with np.errstate(all="ignore"):
    Hs, Ws = src_depth.shape
    params = np.asarray(params, F64)
    rel, (fx, fy, cx, cy) = params[:12], params[12:]
    d, X, Y = _unproject(ref_depth, intr)
    ok = valid(d)
    p0, p1, p2 = _row(rel[0:4], X, Y, d), _row(rel[4:8], X, Y, d), _row(rel[8:12], X, Y, d)
    ok = ok & (p2 > F64(near))
    iz = F64(1.0) / p2
    us = p0 * iz
    vs = p1 * iz
    us = fx * us
    vs = fy * vs
    us = us + cx
    vs = vs + cy
    ok = ok & (us >= 0) & (us < F64(Ws)) & (vs >= 0) & (vs < F64(Hs))
    js = np.where(ok, np.floor(np.where(ok, us, 0.0)), 0).astype(np.int64)
    is_ = np.where(ok, np.floor(np.where(ok, vs, 0.0)), 0).astype(np.int64)
    ds = (src_depth[is_, js] if src_depth.size else np.zeros_like(d)).astype(F64)
    ok = ok & valid(ds)
    tol = F64(rel_tol) * p2
    diff = ds - p2
    agree = ok & (np.abs(diff) <= tol)
    violate = ok & ~agree & (diff > tol)
    return agree, violate


def consistency(ref_depth, intr, sources, near, rel_tol, counts=None):
  """uint8 (H, W, 2): agree and violate counts over `sources` = [(depth, params16)], saturating at 255, added to
  `counts` (not modified).  `near`: one value, or one per source."""
  H, W = ref_depth.shape
  total = np.zeros((H, W, 2), np.int64) if counts is None else counts.astype(np.int64)
  nears = list(near) if np.ndim(near) else [near] * len(sources)
  for (depth, params), n in zip(sources, nears):
    a, v = votes(ref_depth, intr, depth, params, n, rel_tol)
    total[:, :, 0] += a
    total[:, :, 1] += v
  # saturation per call of up to 16 sources equals saturation at the end: the counters only grow
  return np.minimum(total, 255).astype(np.uint8)


def keep_mask(ref_depth, counts, min_agree, max_violate):
  return valid(ref_depth.astype(F64)) & (counts[:, :, 0] >= min_agree) & (counts[:, :, 1] <= max_violate)


def colour_bytes(c):
  with np.errstate(all="ignore"):
    v = np.asarray(c, np.float32).astype(F64)
    v = np.where(v >= 0, v, 0.0)                 # NaN -> 0
    v = np.where(v > 1, 1.0, v)
    v = v * F64(255.0)
    v = v + F64(0.5)
    return np.floor(v).astype(np.uint8)


def emit(ref_depth, counts, image, intr, world, min_agree, max_violate):
  """(points float32 (n, 3), colours uint8 (n, 3), agree uint8 (n,)) of the kept pixels in row-major order."""
  with np.errstate(all="ignore"):
    keep = keep_mask(ref_depth, counts, min_agree, max_violate)
    d, X, Y = _unproject(ref_depth, intr)
    world = np.asarray(world, F64).reshape(12)
    p = np.stack([_row(world[4 * k:4 * k + 4], X, Y, d) for k in range(3)], -1)
    points = p[keep].astype(np.float32)
    colours = np.full((int(keep.sum()), 3), 255, np.uint8) if image is None else colour_bytes(image)[keep]
    return points, colours, counts[:, :, 0][keep].astype(np.uint8)


def voxel_axis(p, origin, inv):
  """(q int64, F int64) of float32 coordinates p on one axis."""
  with np.errstate(all="ignore"):
    s = np.asarray(p, np.float32).astype(F64) - F64(origin)
    s = s * F64(inv)
    q = np.floor(s)
    q = np.where(q >= -HALF, q, float(-HALF))      # NaN -> the lower clamp
    q = np.where(q > HALF - 1, float(HALF - 1), q)
    f = s - q
    f = np.where(f >= 0, f, 0.0)                   # NaN -> 0
    f = np.where(f > 1, 1.0, f)
    f = f * F64(1048576.0)
    f = f + F64(0.5)
    return q.astype(np.int64), np.floor(f).astype(np.int64)


def voxel_keys(points, voxel, origin=(0.0, 0.0, 0.0)):
  inv = F64(1.0) / F64(voxel)
  q = [voxel_axis(points[:, a], origin[a], inv)[0] for a in range(3)]
  return [((int(z) + HALF) << 42) | ((int(y) + HALF) << 21) | (int(x) + HALF) for x, y, z in zip(*q)]


def voxel_downsample(points, colours, voxel, origin=(0.0, 0.0, 0.0)):
  """(points float32 (K, 3), colours uint8 (K, 3), counts int32 (K,), keys list) in ascending key order."""
  points = np.asarray(points, np.float32).reshape(-1, 3)
  inv = F64(1.0) / F64(voxel)
  axes = [voxel_axis(points[:, a], origin[a], inv) for a in range(3)]
  keys = voxel_keys(points, voxel, origin)
  cells = {}
  for i, key in enumerate(keys):
    cell = cells.setdefault(key, [0, [0, 0, 0], [0, 0, 0], [int(axes[a][0][i]) for a in range(3)]])
    cell[0] += 1
    for a in range(3):
      cell[1][a] += int(axes[a][1][i])
      cell[2][a] += int(colours[i, a])
  order = sorted(cells)
  out_p = np.zeros((len(order), 3), np.float32)
  out_c = np.zeros((len(order), 3), np.uint8)
  out_n = np.zeros((len(order),), np.int32)
  for r, key in enumerate(order):
    n, S, C, q = cells[key]
    for a in range(3):
      m = F64(S[a]) / F64(n)
      m = m * F64(2.0 ** -20)
      m = F64(q[a]) + m
      m = m * F64(voxel)
      m = F64(origin[a]) + m
      out_p[r, a] = np.float32(m)
      out_c[r, a] = (2 * C[a] + n) // (2 * n)
    out_n[r] = n
  return out_p, out_c, out_n, order
