"""Lens undistortion of uint8 images: what the reference's scan loader asks cv2 for (``Undistortion.undistort`` with
``optimal_undistorted(camera, alpha=0)``), without cv2 and without the host.  The contract is in include/gsplat_hip.h
under ``gsr_undistort_map`` and ``gsr_image_remap_u8``, the arithmetic in csrc/gsr_undistort.h.

``LensCamera`` is a camera with OpenCV's five coefficients and pixel centres at integers.  ``optimal_pinhole(camera)``
is the largest pinhole view of the same size whose pixels all come from inside the source.  ``undistort_map`` builds the
map of a camera onto a pinhole target, in units of 1/32 source pixel, and ``remap`` takes images through a map.  A
device tensor goes through the native kernels (csrc/undistort.hip) and waits for nothing; a CPU tensor goes through the
same arithmetic compiled for the host (libgsr_hostmath.so), so the two give the same map and the same bytes.
``Undistortion`` holds a camera's map, one copy per device.  A missing library is an error on either path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .image import MAX_SIDE, _host

PULL_LIMIT = 64             # steps of 1/32 pixel a side of the optimal view may be pulled inwards
NEWTON_STEPS = 30


@dataclass(frozen=True)
class LensCamera:
  """A camera of ``width`` x ``height`` pixels whose centres sit at integer coordinates, with OpenCV's distortion
  coefficients in OpenCV's order of meaning: radial k1 k2 k3, tangential p1 p2."""
  width: int
  height: int
  fx: float
  fy: float
  cx: float
  cy: float
  k1: float = 0.0
  k2: float = 0.0
  p1: float = 0.0
  p2: float = 0.0
  k3: float = 0.0

  @property
  def intrinsics(self) -> Tuple[float, float, float, float]:
    return (self.fx, self.fy, self.cx, self.cy)

  @property
  def coefficients(self) -> Tuple[float, float, float, float, float]:
    return (self.k1, self.k2, self.p1, self.p2, self.k3)

  @property
  def distorted(self) -> bool:
    return any(v != 0.0 for v in self.coefficients)

  def source_array(self) -> np.ndarray:
    """The nine doubles the native layer takes: fx fy cx cy k1 k2 p1 p2 k3."""
    return np.array(self.intrinsics + self.coefficients, np.float64)

  @staticmethod
  def from_colmap(camera) -> "LensCamera":
    """A ``colmap_io.Camera`` of model SIMPLE_RADIAL, RADIAL, OPENCV, PINHOLE or SIMPLE_PINHOLE.  COLMAP puts the centre
    of the first pixel at (0.5, 0.5), so 0.5 is taken off cx and cy (``to_colmap_intrinsics`` is the way back)."""
    p = [float(v) for v in camera.params]
    sizes = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4, "SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8}
    if camera.model not in sizes:
      raise ValueError(f"camera model {camera.model} cannot be undistorted: only {', '.join(sizes)} can")
    if len(p) != sizes[camera.model]:
      raise ValueError(f"camera model {camera.model} takes {sizes[camera.model]} parameters, got {len(p)}")
    k1 = k2 = p1 = p2 = 0.0
    if camera.model == "PINHOLE":
      fx, fy, cx, cy = p
    elif camera.model == "OPENCV":
      fx, fy, cx, cy, k1, k2, p1, p2 = p
    else:
      fx = fy = p[0]
      cx, cy = p[1], p[2]
      k1 = p[3] if len(p) > 3 else 0.0
      k2 = p[4] if len(p) > 4 else 0.0
    return LensCamera(int(camera.width), int(camera.height), fx, fy, cx - 0.5, cy - 0.5, k1, k2, p1, p2, 0.0)


def to_colmap_intrinsics(target: Sequence[float]) -> Tuple[float, float, float, float]:
  """(fx, fy, cx, cy) with centres at integers -> the same in COLMAP's convention (the first centre at (0.5, 0.5))."""
  fx, fy, cx, cy = (float(v) for v in target)
  return fx, fy, cx + 0.5, cy + 0.5


def _distort(camera: LensCamera, x: np.ndarray, y: np.ndarray):
  """The model on the normalised plane and its Jacobian: (xd, yd, dxd/dx, dxd/dy, dyd/dx, dyd/dy)."""
  k1, k2, p1, p2, k3 = camera.coefficients
  r2 = x * x + y * y
  rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
  drad = 2 * (k1 + r2 * (2 * k2 + 3 * r2 * k3))                  # d rad / d r2 times 2: d rad / dx = drad x
  xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
  yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
  j00 = rad + x * x * drad + 2 * p1 * y + 6 * p2 * x
  j01 = x * y * drad + 2 * p1 * x + 2 * p2 * y
  j10 = j01
  j11 = rad + y * y * drad + 6 * p1 * y + 2 * p2 * x
  return xd, yd, j00, j01, j10, j11


def _undistort_points(camera: LensCamera, px: np.ndarray, py: np.ndarray):
  """Normalised undistorted coordinates of source pixels (px, py), by Newton iteration in float64.  A sample at which
  the Jacobian's determinant is not positive, or that does not converge, raises: the distortion folds there."""
  xd, yd = (px - camera.cx) / camera.fx, (py - camera.cy) / camera.fy
  x, y = xd.copy(), yd.copy()
  fold = ValueError(f"the distortion {camera.coefficients} folds inside the {camera.width} x {camera.height} image: "
                    "a border pixel has no undistorted position")
  for _ in range(NEWTON_STEPS):
    ex, ey, j00, j01, j10, j11 = _distort(camera, x, y)
    det = j00 * j11 - j01 * j10
    if not (det > 0).all():
      raise fold
    rx, ry = ex - xd, ey - yd
    x, y = x - (j11 * rx - j01 * ry) / det, y - (j00 * ry - j10 * rx) / det
  ex, ey, j00, j01, j10, j11 = _distort(camera, x, y)
  if not ((j00 * j11 - j01 * j10) > 0).all() or not (np.hypot(ex - xd, ey - yd) < 1e-9).all():
    raise fold
  return x, y


def _border(width: int, height: int) -> np.ndarray:
  """(n, 2) float64: the pixels (u, v) of the border of a width x height image."""
  u, v = np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64)
  sides = [np.stack([u, np.zeros_like(u)], 1), np.stack([u, np.full_like(u, height - 1)], 1),
           np.stack([np.zeros_like(v), v], 1), np.stack([np.full_like(v, width - 1), v], 1)]
  return np.ascontiguousarray(np.concatenate(sides))


def _map_points(camera: LensCamera, target: Sequence[float], uv: np.ndarray) -> np.ndarray:
  """The quantised map at destination pixels uv (n, 2), from the host library: (n, 2) int32."""
  source, tgt = camera.source_array(), np.array(target, np.float64)
  out = np.empty((uv.shape[0], 2), np.int32)
  _host().hm_undistort_points(source.ctypes.data, tgt.ctypes.data, camera.height, camera.width, uv.shape[0],
                              uv.ctypes.data, out.ctypes.data)
  return out


def optimal_pinhole(camera: LensCamera) -> Tuple[float, float, float, float]:
  """(fx', fy', cx', cy') of the largest pinhole view of the camera's own size whose pixels all come from inside the
  source (the reference's ``optimal_undistorted(camera, alpha=0)``), centres at integers.  Every border pixel of the
  source is undistorted; the inner rectangle of those positions (the largest left and top, the smallest right and
  bottom) is laid on [0, W - 1] x [0, H - 1]; then, while an entry of the quantised map's border still falls outside
  [0, 32 (S - 1)], that side is pulled inwards by 1/32 pixel.  Without distortion the view is the camera's own."""
  W, H = camera.width, camera.height
  if W < 2 or H < 2 or not (camera.fx > 0 and camera.fy > 0):
    raise ValueError(f"a camera of at least 2 x 2 pixels with positive focal lengths is needed, got {camera}")
  if not all(np.isfinite(camera.source_array())):
    raise ValueError(f"camera parameters must be finite, got {camera}")
  if not camera.distorted:
    return camera.intrinsics
  u, v = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
  left = _undistort_points(camera, np.zeros(H), v)[0].max()
  right = _undistort_points(camera, np.full(H, W - 1.0), v)[0].min()
  top = _undistort_points(camera, u, np.zeros(W))[1].max()
  bottom = _undistort_points(camera, u, np.full(W, H - 1.0))[1].min()
  border = _border(W, H)
  step_x, step_y = 1.0 / (32.0 * camera.fx), 1.0 / (32.0 * camera.fy)
  for _ in range(PULL_LIMIT + 1):
    if not (right > left and bottom > top):
      break
    fx, fy = (W - 1) / (right - left), (H - 1) / (bottom - top)
    target = (float(fx), float(fy), float(-left * fx), float(-top * fy))
    m = _map_points(camera, target, border)
    low_x, high_x = bool((m[:, 0] < 0).any()), bool((m[:, 0] > 32 * (W - 1)).any())      # past the left, the right side
    low_y, high_y = bool((m[:, 1] < 0).any()), bool((m[:, 1] > 32 * (H - 1)).any())
    if not (low_x or high_x or low_y or high_y):
      return target
    left, right = left + step_x * low_x, right - step_x * high_x
    top, bottom = top + step_y * low_y, bottom - step_y * high_y
  raise ValueError(f"no pinhole view inside the source was found for {camera} within {PULL_LIMIT} steps of 1/32 pixel")


def undistort_map(camera: LensCamera, target: Sequence[float], size: Optional[Tuple[int, int]] = None, device=None
                  ) -> torch.Tensor:
  """The map of ``camera`` onto the pinhole ``target`` = (fx', fy', cx', cy'): int32 (Hd, Wd, 2), for destination pixel
  (u, v) the source position (X, Y) in units of 1/32 pixel.  ``size = (Hd, Wd)`` defaults to the camera's own."""
  Hd, Wd = (camera.height, camera.width) if size is None else (int(size[0]), int(size[1]))
  device = torch.device("cpu" if device is None else device)
  source, tgt = camera.source_array(), np.array([float(v) for v in target], np.float64)
  if tgt.shape != (4,):
    raise ValueError(f"target must be (fx, fy, cx, cy), got {target}")
  if not (np.isfinite(source).all() and np.isfinite(tgt).all() and min(source[0], source[1], tgt[0], tgt[1]) > 0):
    raise ValueError(f"camera and target parameters must be finite with positive focal lengths, got {camera}, {target}")
  if min(Hd, Wd, camera.height, camera.width) < 0 or max(Hd, Wd, camera.height, camera.width) > MAX_SIDE:
    raise ValueError(f"sides must be in 0 .. {MAX_SIDE}, got a {camera.width} x {camera.height} camera and size {(Hd, Wd)}")
  out = torch.empty((Hd, Wd, 2), dtype=torch.int32, device=device)
  if out.numel() > 0:
    args = (source.ctypes.data, tgt.ctypes.data, camera.height, camera.width, Hd, Wd, out.data_ptr())
    if out.is_cuda:
      with _lib.on_device(out.device) as stream:
        _lib.call("gsr_undistort_map", *args, stream)      # the parameters are read before the call returns
    else:
      _lib.call("hm_undistort_map", *args, lib=_host())
  return out


def remap(images: torch.Tensor, map: torch.Tensor) -> torch.Tensor:
  """``images`` (B, Hs, Ws, C) or (Hs, Ws, C) uint8 through ``map`` (Hd, Wd, 2) int32 on the same device -> the same
  with Hd x Wd pixels: bilinear at 1/32 pixel, zero outside the source."""
  if not isinstance(images, torch.Tensor) or images.dtype is not torch.uint8 or images.dim() not in (3, 4):
    raise ValueError("images must be a uint8 tensor of shape (B, H, W, C) or (H, W, C)")
  if not isinstance(map, torch.Tensor) or map.dtype is not torch.int32 or map.dim() != 3 or map.shape[2] != 2:
    raise ValueError("map must be an int32 tensor of shape (H, W, 2)")
  if map.device != images.device:
    raise ValueError(f"images are on {images.device}, the map is on {map.device}")
  src = (images if images.dim() == 4 else images.unsqueeze(0)).contiguous()
  map = map.contiguous()
  B, Hs, Ws, channels = src.shape
  Hd, Wd = int(map.shape[0]), int(map.shape[1])
  if channels not in (1, 3):
    raise ValueError(f"images must have 1 or 3 channels, got {channels}")
  if max(Hs, Ws, Hd, Wd) > MAX_SIDE:
    raise ValueError(f"more than {MAX_SIDE} pixels a side are not supported, got images {Ws} x {Hs} and a map {Wd} x {Hd}")
  dst = torch.empty((B, Hd, Wd, channels), dtype=torch.uint8, device=src.device)
  if dst.numel() > 0:
    args = (_lib.ptr(src), B, Hs, Ws, channels, map.data_ptr(), dst.data_ptr(), Hd, Wd)
    if src.is_cuda:
      with _lib.on_device(src.device) as stream:
        _lib.call("gsr_image_remap_u8", *args, stream)
    else:
      _lib.call("hm_image_remap_u8", *args, lib=_host())
  return dst if images.dim() == 4 else dst[0]


class Undistortion:
  """The undistortion of one camera: ``target`` (the optimal pinhole unless given), the map built once per device, and
  ``__call__(images)`` that remaps images of the camera's size on whichever device they are."""

  def __init__(self, camera: LensCamera, target: Optional[Sequence[float]] = None):
    self.camera = camera
    self.target = tuple(float(v) for v in (optimal_pinhole(camera) if target is None else target))
    self._maps: Dict[torch.device, torch.Tensor] = {}

  def map_on(self, device) -> torch.Tensor:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
      device = torch.device("cuda", torch.cuda.current_device())
    if device not in self._maps:
      self._maps[device] = undistort_map(self.camera, self.target, device=device)
    return self._maps[device]

  @property
  def map(self) -> torch.Tensor:
    """The map in host memory."""
    return self.map_on("cpu")

  def __call__(self, images: torch.Tensor) -> torch.Tensor:
    if not isinstance(images, torch.Tensor) or images.dim() not in (3, 4):
      raise ValueError("images must be a uint8 tensor of shape (B, H, W, C) or (H, W, C)")
    if tuple(images.shape[-3:-1]) != (self.camera.height, self.camera.width):
      raise ValueError(f"images are {images.shape[-2]} x {images.shape[-3]}, the camera is "
                       f"{self.camera.width} x {self.camera.height}")
    return remap(images, self.map_on(images.device))
