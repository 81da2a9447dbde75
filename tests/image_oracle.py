"""Oracle of the area resize (include/gsplat_hip.h: gsr_image_resize_area_u8), in numpy integers: the overlap-weight
matrices are built from the definition, the weighted sum is an int64 einsum and the division is ``//``.  It shares no
code with csrc/gsr_image.h.  Also the list of shapes the host and the GPU tests both run, and their inputs."""
import numpy as np

# (Hs, Ws) -> (Hd, Wd)
SHAPES = [((48, 64), (48, 64)),          # copy
          ((48, 64), (24, 32)),          # ratio 2
          ((48, 63), (16, 21)),          # ratio 3
          ((64, 64), (16, 16)),          # ratio 4
          ((96, 120), (61, 77)),         # fractional, both axes
          ((97, 97), (96, 96)),          # every output spans two source pixels with a thin weight
          ((40, 257), (1, 1)),           # one output spanning more than a wave of columns
          ((5, 300), (5, 63)), ((5, 300), (5, 64)), ((5, 300), (5, 65)),      # either side of a 64-column band
          ((70, 119), (33, 50)),         # Ws C odd: misaligned row starts
          ((517, 1031), (32, 64)),       # spans of sixteen and more
          ((300, 7), (100, 3))]          # tall and narrow
SHAPE_IDS = [f"{hs}x{ws}-{hd}x{wd}" for (hs, ws), (hd, wd) in SHAPES]


def weights(S: int, T: int) -> np.ndarray:
  """(T, S) int64: on an axis of S T units, the overlap of destination pixel j = [j S, (j + 1) S) with source pixel
  i = [i T, (i + 1) T)."""
  j, i = np.arange(T, dtype=np.int64)[:, None], np.arange(S, dtype=np.int64)[None, :]
  w = np.clip(np.minimum((i + 1) * T, (j + 1) * S) - np.maximum(i * T, j * S), 0, None)
  assert w.max() <= T and (w.sum(axis=1) == S).all()
  return w


def resize_area(src: np.ndarray, Hd: int, Wd: int) -> np.ndarray:
  """src (B, Hs, Ws, C) uint8 -> (B, Hd, Wd, C) uint8: floor((2 S + D) / (2 D)) with D = Ws Hs."""
  assert src.dtype == np.uint8 and src.ndim == 4
  _, Hs, Ws, _ = src.shape
  wy, wx = weights(Hs, Hd), weights(Ws, Wd)
  S = np.einsum("dy,jx,byxc->bdjc", wy, wx, src.astype(np.int64), optimize=True)
  D = Ws * Hs
  out = (2 * S + D) // (2 * D)
  assert out.min() >= 0 and out.max() <= 255
  return out.astype(np.uint8)


def make_input(B: int, Hs: int, Ws: int, C: int, seed: int = 0) -> np.ndarray:
  """Random uint8 with a row of all 0 and a row of all 255 planted in every image."""
  rng = np.random.default_rng([seed, B, Hs, Ws, C])
  src = rng.integers(0, 256, size=(B, Hs, Ws, C), dtype=np.uint8)
  src[:, Hs // 3] = 0
  src[:, (2 * Hs) // 3] = 255
  return src
