"""Oracle of the lens undistortion (include/gsplat_hip.h: gsr_undistort_map, gsr_image_remap_u8) in numpy: the map in
fp64 with every product and sum on its own line of the stated order (numpy never fuses), the clamp and the quantisation;
the remap in integers from the definition, tap by tap.  It shares no code with csrc/gsr_undistort.h.  Also the cameras,
the map shapes and the hand-made maps that the host and the GPU tests both run."""
import functools

import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

# name -> (H, W, (fx, fy, cx, cy), (k1, k2, k3, p1, p2)), centres at integers
CAMERAS = {"barrel": (48, 64, (60.0, 61.0, 31.3, 23.6), (-0.25, 0.08, -0.01, 0.002, -0.003)),
           "pincushion": (48, 64, (60.0, 61.0, 31.3, 23.6), (0.2, 0.05, 0.0, -0.004, 0.003)),
           "big": (3024, 4032, (3000.0, 3010.0, 2010.3, 1500.7), (-0.12, 0.03, 0.0, 0.0005, -0.0007))}      # border only
SMALL = ("barrel", "pincushion")


def source_array(name):
  """The nine doubles of the native layer, fx fy cx cy k1 k2 p1 p2 k3."""
  _, _, K, (k1, k2, k3, p1, p2) = CAMERAS[name]
  return np.array(K + (k1, k2, p1, p2, k3), np.float64)


def map_points(source, target, Hs, Ws, u, v):
  """The quantised map at destination pixels (u, v) (float64 arrays of one shape): int32 (..., 2)."""
  fx, fy, cx, cy, k1, k2, p1, p2, k3 = (np.float64(s) for s in source)
  fxt, fyt, cxt, cyt = (np.float64(t) for t in target)
  ifx, ify = np.float64(1.0) / fxt, np.float64(1.0) / fyt
  x = (u - cxt) * ifx
  y = (v - cyt) * ify
  xx = x * x
  yy = y * y
  xy = x * y
  r2 = xx + yy
  t = r2 * k3
  t = k2 + t
  t = r2 * t
  t = k1 + t
  t = r2 * t
  rad = 1.0 + t
  a = (2.0 * p1) * xy
  b = 2.0 * xx
  b = r2 + b
  b = p2 * b
  dx = a + b
  a = 2.0 * yy
  a = r2 + a
  a = p1 * a
  b = (2.0 * p2) * xy
  dy = a + b
  xd = x * rad
  xd = xd + dx
  yd = y * rad
  yd = yd + dy
  xs = fx * xd
  xs = xs + cx
  ys = fy * yd
  ys = ys + cy
  return np.stack([quantise(xs, Ws), quantise(ys, Hs)], axis=-1)


def unquantised(source, target, u, v):
  """Source coordinates in plain float64 (any order of operations): for bounds on where a view samples."""
  fx, fy, cx, cy, k1, k2, p1, p2, k3 = source
  x, y = (u - target[2]) / target[0], (v - target[3]) / target[1]
  r2 = x * x + y * y
  rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
  return (fx * (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx,
          fy * (y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy)


def quantise(xs, S):
  xs = np.where(np.isnan(xs), -1.0, xs)
  xs = np.minimum(np.maximum(xs, -1.0), float(S))
  return np.floor(xs * 32.0 + 0.5).astype(np.int32)


def undistort_map(source, target, Hs, Ws, Hd, Wd):
  """int32 (Hd, Wd, 2)."""
  u = np.broadcast_to(np.arange(Wd, dtype=np.float64)[None, :], (Hd, Wd))
  v = np.broadcast_to(np.arange(Hd, dtype=np.float64)[:, None], (Hd, Wd))
  return map_points(source, target, Hs, Ws, u, v)


def border(W, H):
  """(n, 2) float64: the border pixels (u, v) of a W x H image, side by side: top, bottom, left, right."""
  u, v = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
  return np.concatenate([np.stack([u, 0 * u], 1), np.stack([u, 0 * u + H - 1], 1), np.stack([0 * v, v], 1),
                         np.stack([0 * v + W - 1, v], 1)])


def remap(src, map_):
  """src (B, Hs, Ws, C) uint8 through map (Hd, Wd, 2) int32 -> (B, Hd, Wd, C) uint8: the entry clamped to
  [-32, 32 Ws] x [-32, 32 Hs], four taps with weights (32 - ay, ay) x (32 - ax, ax), a tap outside the source 0,
  (sum + 512) >> 10."""
  assert src.dtype == np.uint8 and src.ndim == 4 and map_.dtype == np.int32 and map_.shape[2:] == (2,)
  B, Hs, Ws, C = src.shape
  X = np.clip(map_[..., 0].astype(np.int64), -32, 32 * Ws)
  Y = np.clip(map_[..., 1].astype(np.int64), -32, 32 * Hs)
  x0, y0, ax, ay = X // 32, Y // 32, X % 32, Y % 32                     # floor division, remainder in 0 .. 31
  padded = np.zeros((B, Hs + 3, Ws + 3, C), np.int64)                 # pixel (y, x) at [y + 1, x + 1]; zeros all round
  padded[:, 1:Hs + 1, 1:Ws + 1] = src
  total = np.zeros((B,) + map_.shape[:2] + (C,), np.int64)
  for dy, wy in ((0, 32 - ay), (1, ay)):
    for dx, wx in ((0, 32 - ax), (1, ax)):
      total += (wy * wx)[None, :, :, None] * padded[:, y0 + dy + 1, x0 + dx + 1]
  out = (total + 512) >> 10
  assert out.min() >= 0 and out.max() <= 255
  return out.astype(np.uint8)


def make_input(B, Hs, Ws, C, seed=0):
  rng = np.random.default_rng([seed, B, Hs, Ws, C])
  return rng.integers(0, 256, size=(B, Hs, Ws, C), dtype=np.uint8)


# ---- map cases: name -> (camera, target or None for the optimal pinhole, (Hd, Wd)) -------------------------------------
# The map tests need only SOME target (the optimal pinhole has its own test, against the two properties that define it),
# so these are plain numbers that owe nothing to the package: a view of the source's size a little inside it, one of
# another size, the source's own K (pincushion: the border samples outside the source and the zero border shows), and
# a larger destination of odd width.
def _inner_target(name, Hd, Wd, shrink):
  H, W, K, _ = CAMERAS[name]
  fx, fy = K[0] * shrink * Wd / W, K[1] * shrink * Hd / H
  return (fx, fy, (Wd - 1) / 2.0 + 0.3, (Hd - 1) / 2.0 - 0.4)


MAP_CASES = {}
for _name in SMALL:
  _H, _W, _K, _ = CAMERAS[_name]
  MAP_CASES[f"{_name}-same"] = (_name, _inner_target(_name, _H, _W, 1.12 if _name == "barrel" else 0.9), (_H, _W))
  MAP_CASES[f"{_name}-37x53"] = (_name, _inner_target(_name, 37, 53, 1.1), (37, 53))
  MAP_CASES[f"{_name}-own-K"] = (_name, _K, (_H, _W))
  MAP_CASES[f"{_name}-70x119"] = (_name, _inner_target(_name, 70, 119, 1.0), (70, 119))


@functools.lru_cache(maxsize=None)
def case_map(case):
  name, target, (Hd, Wd) = MAP_CASES[case]
  H, W, _, _ = CAMERAS[name]
  return undistort_map(source_array(name), target, H, W, Hd, Wd)


# ---- hand-made maps for the remap: name -> ((Hs, Ws), map) -------------------------------------------------------------
def _grid(Hd, Wd):
  return np.stack(np.meshgrid(np.arange(Wd), np.arange(Hd)), axis=-1).astype(np.int64)      # (Hd, Wd, 2): (x, y)


@functools.lru_cache(maxsize=None)
def remap_cases():
  cases = {}
  cases["identity"] = ((48, 64), 32 * _grid(48, 64))
  cases["half-pixel"] = ((48, 64), 32 * _grid(47, 63) + 16)
  edge = 32 * _grid(6, 64)                                             # rows of entries at and past every clamp
  edge[0, :, 0], edge[1, :, 0], edge[2, :, 0] = -32, -1, 32 * 64
  edge[3, :8] = (INT32_MIN, INT32_MIN)
  edge[3, 8:16] = (INT32_MAX, INT32_MAX)
  edge[3, 16:24, 0], edge[3, 24:32, 1] = INT32_MIN, INT32_MAX
  edge[4, :, 1], edge[5, :, 1] = -17, 32 * 48 - 15
  edge[3, 32:, 0] = 32 * 63 + 31                                       # the last column with a tap one past it
  cases["clamps"] = ((48, 64), edge)
  cases["flip-5x3000"] = ((5, 3000), 32 * _grid(5, 3000)[:, ::-1] + np.array([7, 3]))
  rng = np.random.default_rng(11)
  cases["random-96x120"] = ((96, 120), np.stack([rng.integers(-40, 32 * 120 + 40, size=(96, 120)),
                                                 rng.integers(-40, 32 * 96 + 40, size=(96, 120))], axis=-1))
  H, W = 517, 1031                                                     # a smooth barrel map, Ws C odd
  source = np.array([900.0, 905.0, 515.2, 258.4, -0.2, 0.05, 0.001, -0.0008, 0.0])
  cases["barrel-517x1031"] = ((H, W), undistort_map(source, (1010.0, 1015.0, 514.0, 259.0), H, W, H, W))
  return {k: (size, np.ascontiguousarray(m.astype(np.int32))) for k, (size, m) in cases.items()}


REMAP_IDS = ["identity", "half-pixel", "clamps", "flip-5x3000", "random-96x120", "barrel-517x1031"]


@functools.lru_cache(maxsize=None)
def remap_reference(case, C, B):
  """(src, expected) of a hand-made map: computed once and shared, not to be modified."""
  (Hs, Ws), m = remap_cases()[case]
  src = make_input(B, Hs, Ws, C)
  out = remap(src, m)
  src.flags.writeable = out.flags.writeable = False
  return src, out
