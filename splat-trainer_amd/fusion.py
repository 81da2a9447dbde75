"""Depth-map fusion: V median-depth maps of a trained scene -> one dense coloured point cloud.  The contract is in
include/gsplat_hip.h under ``gsr_fuse_check``, ``gsr_fuse_emit`` and ``gsr_voxel_downsample``, the arithmetic in
csrc/gsr_fusion.h.

``depth_consistency`` counts, per pixel of a reference depth map, the source views that agree with it and those that
see past it.  ``fuse_depth_maps`` keeps the pixels with enough agreement and no more than the allowed violations and
emits them as world points with colours; ``voxel_downsample`` reduces a cloud to one mean point per occupied voxel;
``fuse_scene`` renders the depth maps first.  ``select_sources`` picks each view's neighbours on the host.

A device tensor goes through the native kernels (csrc/fusion.hip), a CPU tensor through the same arithmetic compiled for
the host (libgsr_hostmath.so): the two give the same bytes.  A missing library is an error on either path.

Host reads.  The pose arithmetic is float64 on the host, so cameras that live on the device are read back: all the
cameras a call is given in ONE copy (``read_cameras``), never one by one.  ``depth_consistency`` and ``select_sources``:
that one read (none for CPU cameras).  ``fuse_depth_maps`` / ``fuse_scene``: that one read for all V cameras, then one
per view, the view's kept count, which sizes its rows; with ``voxel_size`` one more, K.  ``voxel_downsample``: one, the
number of occupied voxels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .data_types import CameraParams
from .dataset import PointCloud
from .image import MAX_SIDE, _host

MAX_SOURCES = _lib.CONSTANTS["GSR_FUSE_MAX_SOURCES"]
COMPACT_BLOCK = _lib.CONSTANTS["GSR_COMPACT_BLOCK"]         # source rows per block offset of gsr_compact_offsets


@dataclass(frozen=True)
class FusionConfig:
  rel_tol: float = 0.01                  # a source agrees within rel_tol of the point's depth in that source
  min_agree: int = 2
  max_violate: int = 0
  num_sources: int = 8
  voxel_size: Optional[float] = None     # None: the cloud is not reduced
  near: Optional[float] = None           # None: each source camera's near_plane


# ---- poses, on the host in float64 with every product written out ----------------------------------------------------
@dataclass(frozen=True)
class HostCamera:
  """A camera's numbers on the host in float64, widened from float32."""
  pose: np.ndarray               # camera_t_world (3, 4)
  intrinsics: np.ndarray         # fx fy cx cy
  near: float
  image_size: Tuple[int, int]    # (W, H)

  @property
  def ref_intrinsics(self) -> np.ndarray:
    """ifx ify cx cy: the reciprocals are formed here, once."""
    fx, fy, cx, cy = self.intrinsics
    return np.array([1.0 / fx, 1.0 / fy, cx, cy], np.float64)


def read_cameras(cameras: Sequence[CameraParams]) -> List[HostCamera]:
  """The poses and intrinsics of ``cameras`` on the host.  Cameras on one device come back in one copy of a (V, 20)
  table; a ``HostCamera`` passes through."""
  todo = [i for i, c in enumerate(cameras) if not isinstance(c, HostCamera)]
  out = list(cameras)
  if todo:
    rows = []
    for i in todo:
      T, proj = cameras[i].T_camera_world.detach(), cameras[i].projection.detach()
      if tuple(T.shape) != (4, 4) or tuple(proj.shape) != (4,):
        raise ValueError(f"a camera needs a (4, 4) pose and a (4,) projection, got {tuple(T.shape)} and {tuple(proj.shape)}")
      rows.append(torch.cat([T.to(torch.float32).reshape(16), proj.to(torch.float32).reshape(4)]))
    if len({r.device for r in rows}) > 1:
      rows = [r.cpu() for r in rows]
    table = torch.stack(rows).cpu().numpy().astype(np.float64)             # the host read
    for i, row in zip(todo, table):
      p = row[16:].copy()
      if not np.isfinite(row).all() or not (p[0] > 0 and p[1] > 0):
        raise ValueError(f"a camera needs a finite pose and finite fx, fy, cx, cy with positive focal lengths, got {row}")
      out[i] = HostCamera(row[:12].reshape(3, 4).copy(), p, float(cameras[i].near_plane),
                          (int(cameras[i].image_size[0]), int(cameras[i].image_size[1])))
  return out


def rigid_inverse(m: np.ndarray) -> np.ndarray:
  """[R | t] (3, 4) -> [R^T | -R^T t]: t' = -((R_0k t_0 + R_1k t_1) + R_2k t_2)."""
  out = np.empty((3, 4), np.float64)
  for k in range(3):
    for c in range(3):
      out[k, c] = m[c, k]
    out[k, 3] = -((m[0, k] * m[0, 3] + m[1, k] * m[1, 3]) + m[2, k] * m[2, 3])
  return out


def compose(a: np.ndarray, b: np.ndarray) -> np.ndarray:
  """a after b, both (3, 4) rigid: entry (k, c) = (a_k0 b_0c + a_k1 b_1c) + a_k2 b_2c, plus a_k3 in the last column."""
  out = np.empty((3, 4), np.float64)
  for k in range(3):
    for c in range(4):
      v = (a[k, 0] * b[0, c] + a[k, 1] * b[1, c]) + a[k, 2] * b[2, c]
      out[k, c] = v + a[k, 3] if c == 3 else v
  return out


def _depth_map(depth, size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
  if not isinstance(depth, torch.Tensor) or depth.dtype is not torch.float32:
    raise ValueError("a depth map must be a float32 tensor of shape (H, W)")
  if depth.dim() == 3 and depth.shape[2] == 1:
    depth = depth[:, :, 0]
  if depth.dim() != 2 or max(depth.shape) > MAX_SIDE:
    raise ValueError(f"a depth map must be (H, W) with sides up to {MAX_SIDE}, got {tuple(depth.shape)}")
  if size is not None and (int(depth.shape[1]), int(depth.shape[0])) != tuple(int(v) for v in size):
    raise ValueError(f"the depth map is {depth.shape[1]} x {depth.shape[0]}, its camera {size[0]} x {size[1]}")
  return depth.detach().contiguous()


def _call(t: torch.Tensor, name: str, *args):
  """The device entry point gsr_<name> on t's device and stream, or the host's hm_<name> for a CPU tensor."""
  if t.is_cuda:
    with _lib.on_device(t.device) as stream:
      return _lib.call("gsr_" + name, *args, stream)
  return _lib.call("hm_" + name, *args, lib=_host())


# ---- consistency -----------------------------------------------------------------------------------------------------
def depth_consistency(ref_depth: torch.Tensor, ref_camera: CameraParams,
                      sources: Sequence[Tuple[torch.Tensor, CameraParams]], rel_tol: float, near: Optional[float] = None,
                      counts: Optional[torch.Tensor] = None) -> torch.Tensor:
  """uint8 (H, W, 2): per pixel of ``ref_depth`` the number of ``sources`` = [(depth, camera)] that agree with it and
  the number that see past it, each saturating at 255.  ``counts`` (the same shape) is added to in place.  ``near``
  defaults to each source camera's ``near_plane``.  Sources go to the device GSR_FUSE_MAX_SOURCES at a time.  Cameras
  on the device are read back, all in one copy (``read_cameras``; a ``HostCamera`` costs nothing)."""
  views = read_cameras([ref_camera] + [camera for _, camera in sources])
  ref_camera, sources = views[0], [(depth, view) for (depth, _), view in zip(sources, views[1:])]
  ref = _depth_map(ref_depth, ref_camera.image_size)
  H, W = int(ref.shape[0]), int(ref.shape[1])
  if not (np.isfinite(rel_tol) and rel_tol >= 0):
    raise ValueError(f"rel_tol must be finite and >= 0, got {rel_tol}")
  if counts is None:
    counts = torch.zeros((H, W, 2), dtype=torch.uint8, device=ref.device)
  elif (not isinstance(counts, torch.Tensor) or counts.dtype is not torch.uint8 or tuple(counts.shape) != (H, W, 2) or
        counts.device != ref.device or not counts.is_contiguous()):
    raise ValueError(f"counts must be a contiguous uint8 tensor of shape {(H, W, 2)} on {ref.device}")
  if H == 0 or W == 0 or len(sources) == 0:
    return counts
  ref_intrinsics, world_t_ref = ref_camera.ref_intrinsics, rigid_inverse(ref_camera.pose)
  entries = []                                  # (depth map, its near plane, 16 doubles)
  for depth, camera in sources:
    d = _depth_map(depth, camera.image_size)
    if d.device != ref.device:
      raise ValueError(f"the reference depth is on {ref.device}, a source on {d.device}")
    params = np.concatenate([compose(camera.pose, world_t_ref).reshape(12), camera.intrinsics])
    entries.append((d, float(camera.near if near is None else near), params))
  begin = 0
  while begin < len(entries):                   # a call takes up to 16 sources that share a near plane
    end = begin + 1
    while end < len(entries) and end - begin < MAX_SOURCES and entries[end][1] == entries[begin][1]:
      end += 1
    chunk = entries[begin:end]
    table = (_lib.GsrFuseSource * len(chunk))(*[
        _lib.GsrFuseSource(depth=_lib.ptr(d), H=int(d.shape[0]), W=int(d.shape[1])) for d, _, _ in chunk])
    params = np.ascontiguousarray(np.stack([p for _, _, p in chunk]))
    tolerances = np.array([chunk[0][1], float(rel_tol)], np.float64)
    args = (ref.data_ptr(), H, W, ref_intrinsics.ctypes.data, table if ref.is_cuda else C.addressof(table),
            params.ctypes.data, len(chunk), tolerances.ctypes.data, counts.data_ptr())
    _call(ref, "fuse_check", *args)             # the host arrays are read before the call returns
    begin = end
  return counts


def select_sources(cameras: Sequence[CameraParams], k: int) -> List[List[int]]:
  """Per view the ``k`` other views with the nearest camera centres among those whose forward axes have a dot product
  above 0.5 with its own, nearest first, ties to the lower index.  Host, float64, deterministic; cameras on the device
  are read back in one copy."""
  k = int(k)
  if k < 0:
    raise ValueError(f"k must be >= 0, got {k}")
  world = [rigid_inverse(c.pose) for c in read_cameras(cameras)]
  centres = [w[:, 3] for w in world]
  forward = [w[:, 2] for w in world]                                   # the world direction of +z
  out = []
  for a in range(len(world)):
    found = []
    for b in range(len(world)):
      if b == a:
        continue
      dot = (forward[a][0] * forward[b][0] + forward[a][1] * forward[b][1]) + forward[a][2] * forward[b][2]
      if dot > 0.5:
        d = centres[a] - centres[b]
        found.append(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], b))
    out.append([b for _, b in sorted(found)[:k]])
  return out


# ---- emission --------------------------------------------------------------------------------------------------------
def _emit_view(depth: torch.Tensor, counts: torch.Tensor, image: Optional[torch.Tensor], camera: HostCamera,
               min_agree: int, max_violate: int):
  """(points (n, 3) float32, colours (n, 3) uint8, agree (n,) uint8) of one view: mask, offsets, ONE host read, emit."""
  H, W = int(depth.shape[0]), int(depth.shape[1])
  device, n_px = depth.device, H * W
  if image is not None:
    if (not isinstance(image, torch.Tensor) or image.dtype is not torch.float32 or tuple(image.shape) != (H, W, 3) or
        image.device != device):
      raise ValueError(f"an image must be a float32 tensor of shape {(H, W, 3)} on {device}")
    image = image.detach().contiguous()
  keep = torch.empty(n_px, dtype=torch.uint8, device=device)
  if n_px > 0:
    _call(depth, "fuse_mask", depth.data_ptr(), counts.data_ptr(), H, W, min_agree, max_violate, keep.data_ptr())
  offsets = None
  if depth.is_cuda and n_px > 0:
    offsets = torch.empty((n_px + COMPACT_BLOCK - 1) // COMPACT_BLOCK, dtype=torch.int32, device=device)
    total = torch.empty(1, dtype=torch.int32, device=device)
    ws = _lib.workspace(int(_lib.load().gsr_compact_workspace_bytes(n_px)), device)
    with _lib.on_device(device) as stream:
      _lib.call("gsr_compact_offsets", keep.data_ptr(), n_px, offsets.data_ptr(), total.data_ptr(), _lib.ptr(ws),
                ws.numel(), stream)
    kept = int(total.item())                                            # the host read
  else:
    kept = int(keep.sum(dtype=torch.int64).item())
  points = torch.empty((kept, 3), dtype=torch.float32, device=device)
  colors = torch.empty((kept, 3), dtype=torch.uint8, device=device)
  agree = torch.empty((kept,), dtype=torch.uint8, device=device)
  if kept > 0:
    ref_intrinsics, world_t_ref = camera.ref_intrinsics, np.ascontiguousarray(rigid_inverse(camera.pose))
    head = (depth.data_ptr(), counts.data_ptr(), _lib.ptr(image), H, W, ref_intrinsics.ctypes.data,
            world_t_ref.ctypes.data, min_agree, max_violate)
    tail = (0, kept, points.data_ptr(), colors.data_ptr(), agree.data_ptr())
    _call(depth, "fuse_emit", *head, *((offsets.data_ptr(),) if depth.is_cuda else ()), *tail)
  return points, colors, agree


def fuse_depth_maps(depths: Sequence[torch.Tensor], images: Optional[Sequence[Optional[torch.Tensor]]],
                    cameras: Sequence[CameraParams], config: FusionConfig = FusionConfig(),
                    sources: Optional[Sequence[Sequence[int]]] = None) -> Tuple[PointCloud, torch.Tensor]:
  """The fused cloud of V views and each point's agree count, uint8 (N,).  ``depths[v]`` (H_v, W_v) float32 and
  ``images[v]`` (H_v, W_v, 3) float32 in [0, 1] (or None: white) belong to ``cameras[v]``; the views may differ in size.
  ``sources[v]`` lists the views that view v is checked against (default ``select_sources(cameras, num_sources)``).
  With ``config.voxel_size`` the cloud goes through ``voxel_downsample``, and the second value is then each voxel's
  point count, saturated at 255.  The cloud's colours are the emitted bytes / 255.  The cameras are read to the host
  once, all together; then each view costs one host read, its kept count."""
  V = len(cameras)
  if V == 0:
    raise ValueError("no views to fuse")
  cameras = read_cameras(cameras)
  if len(depths) != V or (images is not None and len(images) != V):
    raise ValueError(f"{V} cameras need {V} depth maps and images, got {len(depths)} and "
                     f"{None if images is None else len(images)}")
  min_agree, max_violate = int(config.min_agree), int(config.max_violate)
  if not (0 <= min_agree <= 255 and 0 <= max_violate <= 255):
    raise ValueError(f"min_agree and max_violate must be in 0 .. 255, got {min_agree} and {max_violate}")
  if sources is None:
    sources = select_sources(cameras, config.num_sources)
  if len(sources) != V or any(not 0 <= int(s) < V for row in sources for s in row):
    raise ValueError(f"sources must list, for each of the {V} views, indexes of other views")
  maps = [_depth_map(d, c.image_size) for d, c in zip(depths, cameras)]
  parts = []
  for v in range(V):
    counts = depth_consistency(maps[v], cameras[v], [(maps[int(s)], cameras[int(s)]) for s in sources[v]], config.rel_tol,
                               config.near)
    parts.append(_emit_view(maps[v], counts, None if images is None else images[v], cameras[v], min_agree, max_violate))
  points = torch.cat([p[0] for p in parts])
  colors = torch.cat([p[1] for p in parts])
  agree = torch.cat([p[2] for p in parts])
  if config.voxel_size is not None:
    points, colors, n = voxel_downsample(points, colors, config.voxel_size)
    agree = n.clamp(max=255).to(torch.uint8)
  return PointCloud(points, colors.to(torch.float32) / 255.0), agree


def voxel_downsample(points: torch.Tensor, colors_u8: torch.Tensor, voxel_size: float,
                     origin: Optional[Sequence[float]] = None):
  """One point per occupied voxel of side ``voxel_size`` on the grid through ``origin`` (default 0): the mean position
  (K, 3) float32, the mean colour (K, 3) uint8 rounded half up, and the voxel's point count (K,) int32, in ascending
  order of the voxel key (z, then y, then x).  Deterministic: the sums are integers.  One host read, K."""
  if (not isinstance(points, torch.Tensor) or points.dtype is not torch.float32 or points.dim() != 2 or
      points.shape[1] != 3):
    raise ValueError("points must be a float32 tensor of shape (N, 3)")
  if (not isinstance(colors_u8, torch.Tensor) or colors_u8.dtype is not torch.uint8 or
      tuple(colors_u8.shape) != tuple(points.shape) or colors_u8.device != points.device):
    raise ValueError(f"colors must be a uint8 tensor of shape {tuple(points.shape)} on {points.device}")
  grid = np.array([float(voxel_size)] + [float(v) for v in (origin if origin is not None else (0.0, 0.0, 0.0))], np.float64)
  if grid.shape != (4,) or not np.isfinite(grid).all() or not grid[0] > 0 or not np.isfinite(1.0 / grid[0]):
    raise ValueError(f"voxel_size must be finite and above 0 and origin three finite numbers, got {voxel_size}, {origin}")
  N, device = int(points.shape[0]), points.device
  if N > 2 ** 31 - 1:
    raise ValueError(f"at most 2^31 - 1 points, got {N}")
  points, colors_u8 = points.detach().contiguous(), colors_u8.contiguous()
  out_p = torch.empty((N, 3), dtype=torch.float32, device=device)
  out_c = torch.empty((N, 3), dtype=torch.uint8, device=device)
  out_n = torch.empty((N,), dtype=torch.int32, device=device)
  if N == 0:
    return out_p, out_c, out_n
  args = (points.data_ptr(), colors_u8.data_ptr(), N, grid.ctypes.data, out_p.data_ptr(), out_c.data_ptr(),
          out_n.data_ptr())
  if points.is_cuda:
    K_dev = torch.empty(1, dtype=torch.int32, device=device)
    ws = _lib.workspace(int(_lib.load().gsr_voxel_workspace_bytes(N)), device)
    with _lib.on_device(device) as stream:
      _lib.call("gsr_voxel_downsample", *args, K_dev.data_ptr(), _lib.ptr(ws), ws.numel(), stream)
    K = int(K_dev.item())                                               # the host read
  else:
    K_host = np.zeros(1, np.int64)
    _lib.call("hm_voxel_downsample", *args, K_host.ctypes.data, lib=_host())
    K = int(K_host[0])
  return out_p[:K].clone(), out_c[:K].clone(), out_n[:K].clone()


def fuse_scene(render: Callable, cameras: Sequence[CameraParams], config: FusionConfig = FusionConfig(),
               image_indexes: Optional[Sequence[int]] = None) -> Tuple[PointCloud, torch.Tensor]:
  """Renders every camera and fuses the median depth maps: what ``fuse_depth_maps`` returns.  ``render(camera_params,
  image_idx)`` returns a ``Rendering`` with ``median_depth_image``; an object with a ``render`` method (an ``MLPScene``)
  is called as ``render(camera_params, image_idx, render_median_depth=True)``.  All depth maps and images stay on the
  device until the cloud is made."""
  if image_indexes is None:
    image_indexes = list(range(len(cameras)))
  if len(image_indexes) != len(cameras):
    raise ValueError(f"{len(cameras)} cameras need {len(cameras)} image indexes, got {len(image_indexes)}")
  if hasattr(render, "render"):
    scene = render
    render = lambda camera, idx: scene.render(camera, idx, render_median_depth=True)      # noqa: E731
  depths, images = [], []
  with torch.no_grad():
    for camera, idx in zip(cameras, image_indexes):
      rendering = render(camera, None if idx is None else int(idx))
      if rendering.median_depth_image is None:
        raise ValueError("the rendering has no median_depth_image: render with render_median_depth=True")
      depths.append(rendering.median_depth_image.detach().to(torch.float32))
      image = rendering.image.detach().to(torch.float32)
      images.append(image[:, :, :3].contiguous() if image.dim() == 3 and image.shape[2] >= 3 else None)
  return fuse_depth_maps(depths, images, cameras, config)
