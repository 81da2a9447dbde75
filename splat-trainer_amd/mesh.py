"""TSDF meshing: V median-depth maps of a trained scene -> a truncated signed distance volume -> one coloured triangle
mesh.  The contract is stated in csrc/gsr_mesh.h, the entry points in include/gsplat_hip.h under ``gsr_tsdf_integrate``.

``TsdfVolume`` holds the volume's six integer planes; ``integrate`` adds views to it (any order and any chunking give the
same integers) and ``extract`` makes the surface-nets mesh of its zero surface: one vertex per cell that the surface
crosses, one quad per crossed lattice edge, an indexed mesh that needs no welding.  ``mesh_depth_maps`` sizes the volume
and does both; ``mesh_scene`` renders the depth maps first.

A device tensor goes through the native kernels (csrc/mesh.hip), a CPU tensor through the same arithmetic compiled for
the host (libgsr_hostmath.so): the two give the same bytes.  A missing library is an error on either path.

Host reads.  ``integrate``: all the cameras of the call in ONE copy (``read_cameras``; none for ``HostCamera`` records).
``extract``: two, the vertex count V and the face count F, each sizing the rows that the next launch writes.
``mesh_depth_maps``: the cameras once; with ``bounds=None`` what ``fuse_depth_maps`` reads and one more for the cloud's
box; then the two of ``extract``.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, ply_io
from .data_types import CameraParams
from .fusion import (COMPACT_BLOCK, MAX_SOURCES, FusionConfig, _call, _depth_map, depth_consistency, fuse_depth_maps,
                     read_cameras, select_sources)
from .normalization import Normalization

MAX_NODES = 2 ** 29
MAX_VIEWS = 65535                      # integrations a volume takes: sum_d stays inside int32


@dataclass(frozen=True)
class TsdfConfig:
  voxel_size: float = 0.02
  trunc: Optional[float] = None                  # None: 4 voxels
  min_weight: int = 1                            # a node counts with at least this many samples
  bounds: Optional[Tuple[Sequence[float], Sequence[float]]] = None      # (lo, hi); None: the box of the fused cloud
  max_voxels: int = 256 ** 3                     # cap on the node count
  near: Optional[float] = None                   # None: each camera's near_plane
  fusion: Optional[FusionConfig] = None          # set: depths that fail the consistency check are dropped first


class TriangleMesh:
  """vertices (V, 3) float32, colors (V, 3) uint8, faces (F, 3) int32 on one device.  Normals by the right-hand rule
  point to free space."""

  def __init__(self, vertices: torch.Tensor, colors: torch.Tensor, faces: torch.Tensor):
    if (vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype is not torch.float32 or
        tuple(colors.shape) != tuple(vertices.shape) or colors.dtype is not torch.uint8 or faces.dim() != 2 or
        faces.shape[1] != 3 or faces.dtype is not torch.int32):
      raise ValueError("a mesh needs float32 vertices (V, 3), uint8 colors (V, 3) and int32 faces (F, 3), got "
                       f"{tuple(vertices.shape)} {vertices.dtype}, {tuple(colors.shape)} {colors.dtype}, "
                       f"{tuple(faces.shape)} {faces.dtype}")
    self.vertices, self.colors, self.faces = vertices, colors, faces

  @property
  def num_vertices(self) -> int:
    return int(self.vertices.shape[0])

  @property
  def num_faces(self) -> int:
    return int(self.faces.shape[0])

  @property
  def device(self) -> torch.device:
    return self.vertices.device

  def __repr__(self):
    return f"TriangleMesh({self.num_vertices} vertices, {self.num_faces} faces, {self.device})"

  def to(self, device) -> "TriangleMesh":
    return TriangleMesh(self.vertices.to(device), self.colors.to(device), self.faces.to(device))

  def transformed(self, normalization: Normalization) -> "TriangleMesh":
    """The mesh with its vertices taken through ``normalization``; colours and faces as they are."""
    return TriangleMesh(normalization.transform_points(self.vertices), self.colors, self.faces)

  def save_ply(self, path: Union[str, Path]) -> None:
    ply_io.write_mesh(path, self.vertices.detach().cpu().numpy(), self.colors.cpu().numpy(), self.faces.cpu().numpy())


def _grid(voxel_size, origin) -> np.ndarray:
  try:
    grid = np.array([float(voxel_size)] + [float(v) for v in origin], np.float64)
  except (TypeError, ValueError):
    grid = np.zeros(0)
  if grid.shape != (4,) or not np.isfinite(grid).all() or not grid[0] > 0 or not np.isfinite(1.0 / grid[0]):
    raise ValueError(f"voxel_size must be finite and above 0 and origin three finite numbers, got {voxel_size}, {origin}")
  return grid


def _compact(mask: torch.Tensor) -> Tuple[Optional[torch.Tensor], int]:
  """(block offsets, kept) of a byte mask: gsr_compact_offsets and ONE host read on the device, a sum on the host."""
  n = int(mask.numel())
  if not mask.is_cuda:
    return None, int(mask.sum(dtype=torch.int64).item())
  offsets = torch.empty((n + COMPACT_BLOCK - 1) // COMPACT_BLOCK, dtype=torch.int32, device=mask.device)
  total = torch.empty(1, dtype=torch.int32, device=mask.device)
  ws = _lib.workspace(int(_lib.load().gsr_compact_workspace_bytes(n)), mask.device)
  with _lib.on_device(mask.device) as stream:
    _lib.call("gsr_compact_offsets", mask.data_ptr(), n, offsets.data_ptr(), total.data_ptr(), _lib.ptr(ws), ws.numel(),
              stream)
  return offsets, int(total.item())                                      # the host read


class TsdfVolume:
  """``dims`` = (nx, ny, nz) nodes on the lattice ``origin + idx * voxel_size``; ``state`` int32 (6, nodes) in planes
  sum_d, n, colour count and three colour byte sums, node (i, j, k) at (k ny + j) nx + i."""

  def __init__(self, origin: Sequence[float], dims: Sequence[int], voxel_size: float, device="cpu",
               trunc: Optional[float] = None, near: Optional[float] = None):
    self.grid = _grid(voxel_size, origin)
    try:
      dims = tuple(int(d) for d in dims)
    except (TypeError, ValueError):
      dims = ()
    if len(dims) != 3 or min(dims) < 0:
      raise ValueError(f"dims must be three node counts >= 0, got {dims}")
    if dims[0] * dims[1] * dims[2] > MAX_NODES:
      raise ValueError(f"a volume holds at most 2^29 nodes, got {dims[0]} x {dims[1]} x {dims[2]}")
    trunc = 4.0 * self.grid[0] if trunc is None else float(trunc)
    if not (np.isfinite(trunc) and trunc > 0 and np.isfinite(1.0 / trunc)):
      raise ValueError(f"trunc must be finite and above 0, got {trunc}")
    if near is not None and not np.isfinite(float(near)):
      raise ValueError(f"near must be finite, got {near}")
    self.dims, self.trunc, self.near = dims, trunc, None if near is None else float(near)
    self.state = torch.zeros((6, self.num_nodes), dtype=torch.int32, device=device)
    self.device = self.state.device                                       # "cuda" has become "cuda:0"
    self.views = 0                                                        # integrations so far

  @property
  def num_nodes(self) -> int:
    return self.dims[0] * self.dims[1] * self.dims[2]

  @property
  def num_cells(self) -> int:
    return max(self.dims[0] - 1, 0) * max(self.dims[1] - 1, 0) * max(self.dims[2] - 1, 0)

  @property
  def voxel_size(self) -> float:
    return float(self.grid[0])

  @property
  def origin(self) -> Tuple[float, float, float]:
    return tuple(float(v) for v in self.grid[1:])

  def integrate(self, depths: Sequence[torch.Tensor], images: Optional[Sequence[Optional[torch.Tensor]]],
                cameras: Sequence[CameraParams]) -> "TsdfVolume":
    """Adds the views ``(depths[v] (H, W) float32, images[v] (H, W, 3) float32 or None: white, cameras[v])``, up to
    GSR_FUSE_MAX_SOURCES to a launch; views of one launch share a near plane.  The cameras are read back in one copy."""
    V = len(cameras)
    if len(depths) != V or (images is not None and len(images) != V):
      raise ValueError(f"{V} cameras need {V} depth maps and images, got {len(depths)} and "
                       f"{None if images is None else len(images)}")
    if self.views + V > MAX_VIEWS:
      raise ValueError(f"a volume takes at most {MAX_VIEWS} views, it holds {self.views} and was given {V} more")
    cameras = read_cameras(cameras)
    entries = []                                  # (depth, image, near, 16 doubles)
    for v, camera in enumerate(cameras):
      d = _depth_map(depths[v], camera.image_size)
      image = None if images is None else images[v]
      if d.device != self.device:
        raise ValueError(f"the volume is on {self.device}, a depth map on {d.device}")
      if image is not None:
        if (not isinstance(image, torch.Tensor) or image.dtype is not torch.float32 or
            tuple(image.shape) != tuple(d.shape) + (3,) or image.device != self.device):
          raise ValueError(f"an image must be a float32 tensor of shape {tuple(d.shape) + (3,)} on {self.device}")
        image = image.detach().contiguous()
      params = np.concatenate([camera.pose.reshape(12), camera.intrinsics])
      entries.append((d, image, float(camera.near if self.near is None else self.near), params))
    begin = 0
    while begin < V and self.num_nodes > 0:
      end = begin + 1
      while end < V and end - begin < MAX_SOURCES and entries[end][2] == entries[begin][2]:
        end += 1
      chunk = entries[begin:end]
      table = (_lib.GsrTsdfSource * len(chunk))(*[
          _lib.GsrTsdfSource(depth=_lib.ptr(d), image=_lib.ptr(im), H=int(d.shape[0]), W=int(d.shape[1]))
          for d, im, _, _ in chunk])
      params = np.ascontiguousarray(np.stack([p for _, _, _, p in chunk]))
      tsdf = np.array([chunk[0][2], self.trunc, 1.0 / self.trunc], np.float64)
      _call(self.state, "tsdf_integrate", self.state.data_ptr(), *self.dims, self.grid.ctypes.data,
            table if self.state.is_cuda else C.addressof(table), params.ctypes.data, len(chunk), tsdf.ctypes.data)
      begin = end
    self.views += V
    return self

  def extract(self, min_weight: int = 1) -> TriangleMesh:
    """The surface-nets mesh of the zero surface among the nodes with at least ``min_weight`` samples.  Two host reads,
    V and F."""
    mesh, _ = self._extract(min_weight)
    return mesh

  def _extract(self, min_weight: int) -> Tuple[TriangleMesh, torch.Tensor]:
    """(mesh, cell_vertex (cells,) int32)."""
    if isinstance(min_weight, bool) or int(min_weight) != min_weight or int(min_weight) < 1:
      raise ValueError(f"min_weight must be an int >= 1, got {min_weight!r}")
    min_weight, device, cells = int(min_weight), self.device, self.num_cells
    empty = lambda n, dtype: torch.empty((n, 3), dtype=dtype, device=device)      # noqa: E731
    if cells == 0:
      return (TriangleMesh(empty(0, torch.float32), empty(0, torch.uint8), empty(0, torch.int32)),
              torch.empty((0,), dtype=torch.int32, device=device))
    state, head = self.state, (self.state.data_ptr(), *self.dims)
    offsets = lambda o: (o.data_ptr(),) if state.is_cuda else ()                  # noqa: E731
    active = torch.empty(cells, dtype=torch.uint8, device=device)
    _call(state, "mesh_vertex_mask", *head, min_weight, active.data_ptr())
    block_offsets, V = _compact(active)
    cell_vertex = torch.empty(cells, dtype=torch.int32, device=device)
    vertices, colors = empty(V, torch.float32), empty(V, torch.uint8)
    _call(state, "mesh_vertex_emit", *head, self.grid.ctypes.data, min_weight, *offsets(block_offsets), V,
          cell_vertex.data_ptr(), _lib.ptr(vertices), _lib.ptr(colors))
    keep = torch.empty(3 * self.num_nodes, dtype=torch.uint8, device=device)
    _call(state, "mesh_face_mask", *head, min_weight, cell_vertex.data_ptr(), keep.data_ptr())
    block_offsets, kept = _compact(keep)
    faces = empty(2 * kept, torch.int32)
    if kept > 0:
      _call(state, "mesh_face_emit", *head, min_weight, cell_vertex.data_ptr(), *offsets(block_offsets), 2 * kept,
            faces.data_ptr())
    return TriangleMesh(vertices, colors, faces), cell_vertex


def _box_dims(lo: np.ndarray, hi: np.ndarray, voxel: float) -> Tuple[int, int, int]:
  """Nodes per axis of the lattice from ``lo`` that reaches ``hi``: cells = ceil((hi - lo) / voxel), to one part in a
  million, and one node more."""
  return tuple(int(max(1, math.ceil((h - l) / voxel - 1e-6))) + 1 for l, h in zip(lo, hi))


def mesh_depth_maps(depths: Sequence[torch.Tensor], images: Optional[Sequence[Optional[torch.Tensor]]],
                    cameras: Sequence[CameraParams], config: TsdfConfig = TsdfConfig()) -> TriangleMesh:
  """The mesh of V views.  ``depths[v]`` (H_v, W_v) float32 and ``images[v]`` (H_v, W_v, 3) float32 in [0, 1] (or None:
  white) belong to ``cameras[v]``.  With ``config.bounds = (lo, hi)`` the volume's lattice starts at ``lo`` and reaches
  ``hi``; with None the box is that of the ``fuse_depth_maps`` cloud (filtered by ``config.fusion``; every valid pixel
  without one), grown by ``trunc``.  A volume of more than ``config.max_voxels`` nodes raises, naming the voxel size that
  fits.  With ``config.fusion`` each view's depths that ``gsr_fuse_mask`` rejects are zeroed before integration, which
  removes floaters."""
  V = len(cameras)
  if V == 0:
    raise ValueError("no views to mesh")
  if len(depths) != V or (images is not None and len(images) != V):
    raise ValueError(f"{V} cameras need {V} depth maps and images, got {len(depths)} and "
                     f"{None if images is None else len(images)}")
  voxel = float(_grid(config.voxel_size, (0.0, 0.0, 0.0))[0])
  trunc = 4.0 * voxel if config.trunc is None else float(config.trunc)
  if not (np.isfinite(trunc) and trunc > 0):
    raise ValueError(f"trunc must be finite and above 0, got {config.trunc}")
  if isinstance(config.min_weight, bool) or int(config.min_weight) != config.min_weight or config.min_weight < 1:
    raise ValueError(f"min_weight must be an int >= 1, got {config.min_weight!r}")
  cameras = read_cameras(cameras)
  maps = [_depth_map(d, c.image_size) for d, c in zip(depths, cameras)]
  device = maps[0].device
  fusion = config.fusion
  if fusion is not None:                          # floater removal: what gsr_fuse_mask rejects is no depth
    min_agree, max_violate = int(fusion.min_agree), int(fusion.max_violate)
    if not (0 <= min_agree <= 255 and 0 <= max_violate <= 255):
      raise ValueError(f"min_agree and max_violate must be in 0 .. 255, got {min_agree} and {max_violate}")
    sources = select_sources(cameras, fusion.num_sources)
    kept_maps = []
    for v in range(V):
      counts = depth_consistency(maps[v], cameras[v], [(maps[s], cameras[s]) for s in sources[v]], fusion.rel_tol,
                                 fusion.near)
      H, W = int(maps[v].shape[0]), int(maps[v].shape[1])
      keep = torch.zeros((H, W), dtype=torch.uint8, device=maps[v].device)
      if H * W > 0:
        _call(maps[v], "fuse_mask", maps[v].data_ptr(), counts.data_ptr(), H, W, min_agree, max_violate, keep.data_ptr())
      kept_maps.append(torch.where(keep.bool(), maps[v], torch.zeros_like(maps[v])))
    maps = kept_maps
  if config.bounds is None:
    every = FusionConfig(min_agree=0, max_violate=255, num_sources=0)      # the maps are filtered already
    cloud, _ = fuse_depth_maps(maps, None, cameras, every)
    if cloud.num_points == 0:
      raise ValueError("no view has a valid depth: there is nothing to mesh")
    box = torch.stack([cloud.points.min(0).values, cloud.points.max(0).values]).cpu().numpy().astype(np.float64)
    lo, hi = box[0] - trunc, box[1] + trunc
  else:
    try:
      lo, hi = (np.array([float(v) for v in side], np.float64) for side in config.bounds)
    except (TypeError, ValueError):
      lo = hi = np.zeros(0)
    if lo.shape != (3,) or hi.shape != (3,) or not np.isfinite(lo).all() or not np.isfinite(hi).all() or not (hi > lo).all():
      raise ValueError(f"bounds must be (lo, hi), three finite numbers each with hi above lo, got {config.bounds}")
  dims = _box_dims(lo, hi, voxel)
  nodes = dims[0] * dims[1] * dims[2]
  limit = min(int(config.max_voxels), MAX_NODES)
  if nodes > limit:
    fits = voxel
    while True:                                   # the cube-root estimate, stepped up until the count fits
      fits *= max((nodes / limit) ** (1.0 / 3.0), 1.0) * 1.001
      d = _box_dims(lo, hi, fits)
      nodes = d[0] * d[1] * d[2]
      if nodes <= limit:
        break
    fits = float(f"{fits * 1.0001:.6g}")           # as printed; a larger voxel never needs more nodes
    raise ValueError(f"a voxel size of {voxel} needs {dims[0]} x {dims[1]} x {dims[2]} nodes, above max_voxels = "
                     f"{limit}: a voxel size of {fits:.6g} fits")
  volume = TsdfVolume(lo, dims, voxel, device, trunc=trunc, near=config.near)
  volume.integrate(maps, images, cameras)
  return volume.extract(int(config.min_weight))


def mesh_scene(render: Callable, cameras: Sequence[CameraParams], config: TsdfConfig = TsdfConfig(),
               image_indexes: Optional[Sequence[int]] = None) -> TriangleMesh:
  """Renders every camera and meshes the median depth maps: what ``mesh_depth_maps`` returns.  ``render`` is as in
  ``fuse_scene``: a function ``render(camera_params, image_idx)`` that returns a ``Rendering`` with
  ``median_depth_image``, or an object with such a ``render`` method (an ``MLPScene``)."""
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
  return mesh_depth_maps(depths, images, cameras, config)
