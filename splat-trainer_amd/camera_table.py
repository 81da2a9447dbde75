"""Camera tables with trainable poses: drop-ins for the reference's ``splat_trainer.camera_table`` (``PoseTable``,
``RigPoseTable``, ``CameraTable``, ``CameraRigTable``, ``MultiCameraTable``, ``Cameras``, ``Camera``, ``Projections``,
``Label`` and the functions beside them) on plain torch containers -- no ``tensordict``, ``roma`` or ``beartype`` -- with
the pose maths on two native launches (csrc/camera_table.hip, maths and the order of every operation in
csrc/gsr_camera_table.h).

A pose row is a quaternion ``q`` (XYZW, roma's order; normalised on use, ``F.normalize``) and a translation ``t``;
``table(idx)`` is ``[R(q^) t; 0 0 0 1]`` of the selected rows and, for a rig, ``camera_t_rig[camera_idx] @
rig_t_world[frame_idx]``.  Forward and backward are one launch each; the gradient of a row is the sum over the images that
selected it in increasing batch position, with no float atomics, so it is bit-identical between runs.

Indices.  An index tensor on the CPU (and an int) is checked on the host before the launch and raises ``GsplatHipError``
at once.  A device tensor is not read by the host: the kernel clamps an index outside the table to row 0 and sets a
status word on the device, and ``check_indices()`` -- one host wait, whenever the caller chooses -- raises for it.
Negative indices do not count from the end.

``forward`` needs the HIP device and raises ``GsplatHipError`` on CPU parameters; there is no second path.  Building a
table from ``(..., 4, 4)`` matrices, the containers and the functions are plain torch and run wherever their tensors live.
"""
from __future__ import annotations

import abc
import dataclasses
from dataclasses import dataclass
from enum import Flag
from typing import Any, List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._args import f32, on_one_device, require
from ._lib import ptr as _ptr
from .data_types import CameraParams


class Label(Flag):
  """Labels for camera tables.  Bitwise encoded."""
  Validation = 1 << 0
  Training = 1 << 1


# ---- rigid transforms (util/transforms.py) ---------------------------------------------------------------------------

def split_rt(transform: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
  return transform[..., :3, :3].contiguous(), transform[..., :3, 3].contiguous()


def join_rt(r: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
  if r.shape[-2:] != (3, 3) or t.shape[-1] != 3 or r.shape[:-2] != t.shape[:-1]:
    raise ValueError(f"expected (..., 3, 3) and (..., 3) with one prefix, got {tuple(r.shape)} and {tuple(t.shape)}")
  T = torch.eye(4, device=r.device, dtype=r.dtype).expand(t.shape[:-1] + (4, 4)).contiguous()
  T[..., 0:3, 0:3] = r
  T[..., 0:3, 3] = t
  return T


def to_matrix(intrinsics: torch.Tensor) -> torch.Tensor:
  fx, fy, cx, cy = intrinsics.unbind(-1)
  m = torch.eye(3, dtype=intrinsics.dtype, device=intrinsics.device)
  m = m.unsqueeze(0).expand(intrinsics.shape[:-1] + (3, 3)).clone()
  m[..., 0, 0] = fx
  m[..., 1, 1] = fy
  m[..., 0, 2] = cx
  m[..., 1, 2] = cy
  return m


def rotmat_to_unitquat(R: torch.Tensor) -> torch.Tensor:
  """(..., 3, 3) rotation matrices to (..., 4) unit quaternions XYZW, the four-branch form roma.rotmat_to_unitquat uses
  (the branch with the largest of m00, m11, m22 and the trace), in float64.  The sign is the branch's, as in roma."""
  m = R.reshape(-1, 3, 3).to(torch.float64)
  m00, m01, m02, m10, m11, m12, m20, m21, m22 = (m[:, i, j] for i in range(3) for j in range(3))
  trace = m00 + m11 + m22
  choice = torch.stack([m00, m11, m22, trace], dim=1).argmax(dim=1)
  branches = torch.stack([
      torch.stack([1 + m00 - m11 - m22, m10 + m01, m20 + m02, m21 - m12], dim=1),
      torch.stack([m01 + m10, 1 - m00 + m11 - m22, m21 + m12, m02 - m20], dim=1),
      torch.stack([m02 + m20, m12 + m21, 1 - m00 - m11 + m22, m10 - m01], dim=1),
      torch.stack([m21 - m12, m02 - m20, m10 - m01, 1 + trace], dim=1)], dim=1)          # (n, 4 branches, 4)
  q = branches[torch.arange(m.shape[0], device=m.device), choice]
  return F.normalize(q, dim=-1).reshape(R.shape[:-2] + (4,))


# ---- the native pose calls -------------------------------------------------------------------------------------------

_status = {}              # device index -> the (1,) int32 status word the kernels OR into


def _status_word(device: torch.device) -> torch.Tensor:
  key = device.index if device.index is not None else torch.cuda.current_device()
  if key not in _status:
    _status[key] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", key))
  return _status[key]


def check_indices(device: Optional[torch.device] = None) -> None:
  """Waits for the device (every device a table ran on when ``device`` is None) and raises ``GsplatHipError`` when a
  pose-table launch since the last check met an index outside its table; the flag is cleared."""
  keys = list(_status) if device is None else [torch.device(device).index or 0]
  for key in keys:
    word = _status.get(key)
    if word is not None and int(word.item()):
      word.zero_()
      raise _lib.GsplatHipError(f"a pose table on cuda:{key} was indexed outside its rows (the launch read row 0 instead)")


def _pose_table(q: torch.Tensor, t: torch.Tensor, name: str):
  """The two tensors of a pose table: both shapes, then both dtypes, then the device, then the table's own row limit."""
  tensors = {f"{name}'s q": q, f"{name}'s t": t}
  require(f"{name}'s q", q, shape=("A", 4))
  require(f"{name}'s t", t, shape=(q.shape[0], 3))
  for label, x in tensors.items():
    require(label, x, dtype=torch.float32)
  on_one_device(tensors, what="a pose table")
  if not 1 <= q.shape[0] <= _lib.CONSTANTS["GSR_POSE_MAX_ROWS"]:
    raise ValueError(f"{name} must hold 1..{_lib.CONSTANTS['GSR_POSE_MAX_ROWS']} rows, got {q.shape[0]}")


def _index(indices: Any, rows: int, device: torch.device, name: str) -> torch.Tensor:
  """``indices`` as a contiguous (B,) int64 tensor on ``device``; host-resident ones are checked here."""
  if isinstance(indices, int):
    indices = torch.tensor([indices], dtype=torch.int64)
  if not isinstance(indices, torch.Tensor) or indices.dtype.is_floating_point or indices.dtype is torch.bool:
    raise ValueError(f"{name} must be an integer tensor, got {indices!r}")
  if indices.dim() > 1:
    raise ValueError(f"{name}: expected a 0-D or 1-D tensor, got {tuple(indices.shape)}")
  indices = indices.reshape(-1)
  if not indices.is_cuda and indices.numel():
    lo, hi = int(indices.min()), int(indices.max())
    if lo < 0 or hi >= rows:
      raise _lib.GsplatHipError(f"{name} out of range: {lo if lo < 0 else hi} is not in [0, {rows})")
  return indices.to(device=device, dtype=torch.int64).contiguous()


class _PoseFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, q_l, t_l, idx_l, q_r, t_r, idx_r):
    q_l, t_l = q_l.detach().contiguous(), t_l.detach().contiguous()
    rig = q_r is not None
    if rig:
      q_r, t_r = q_r.detach().contiguous(), t_r.detach().contiguous()
    B = idx_l.shape[0]
    with _lib.on_device(q_l.device) as stream:
      T = torch.empty((B, 4, 4), dtype=torch.float32, device=q_l.device)
      _lib.call("gsr_pose_forward", _ptr(q_l), _ptr(t_l), q_l.shape[0], _ptr(idx_l), _ptr(q_r), _ptr(t_r),
                q_r.shape[0] if rig else 0, _ptr(idx_r), B, _ptr(T), _status_word(q_l.device).data_ptr(), stream)
    ctx.save_for_backward(*((q_l, t_l, idx_l, q_r, t_r, idx_r) if rig else (q_l, t_l, idx_l)))
    ctx.rig = rig
    return T

  @staticmethod
  def backward(ctx, G):
    saved = ctx.saved_tensors
    q_l, t_l, idx_l = saved[:3]
    q_r, t_r, idx_r = saved[3:] if ctx.rig else (None, None, None)
    want_l = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
    want_r = ctx.rig and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
    with _lib.on_device(q_l.device) as stream:
      G = f32(G)
      d_q_l, d_t_l = (torch.empty_like(q_l), torch.empty_like(t_l)) if want_l else (None, None)
      d_q_r, d_t_r = (torch.empty_like(q_r), torch.empty_like(t_r)) if want_r else (None, None)
      _lib.call("gsr_pose_backward", _ptr(q_l), _ptr(t_l), q_l.shape[0], _ptr(idx_l), _ptr(q_r), _ptr(t_r),
                q_r.shape[0] if ctx.rig else 0, _ptr(idx_r), idx_l.shape[0], _ptr(G), _ptr(d_q_l), _ptr(d_t_l), _ptr(d_q_r),
                _ptr(d_t_r), _status_word(q_l.device).data_ptr(), stream)
    return d_q_l, d_t_l, None, d_q_r, d_t_r, None


def pose_matrices(q: torch.Tensor, t: torch.Tensor, indices: torch.Tensor, q_right: Optional[torch.Tensor] = None,
                  t_right: Optional[torch.Tensor] = None, indices_right: Optional[torch.Tensor] = None) -> torch.Tensor:
  """(B, 4, 4) transforms of rows ``indices`` of the table ``(q (A, 4), t (A, 3))`` and, with a right table, the
  products ``left[indices] @ right[indices_right]``: one autograd node over the two native launches."""
  _pose_table(q, t, "the pose table")
  idx = _index(indices, q.shape[0], q.device, "indices")
  if q_right is None:
    return _PoseFn.apply(q, t, idx, None, None, None)
  _pose_table(q_right, t_right, "the right pose table")
  if q_right.device != q.device:
    raise ValueError(f"pose tables on different devices: {q.device} and {q_right.device}")
  idx_r = _index(indices_right, q_right.shape[0], q.device, "indices_right")
  if idx_r.shape != idx.shape:
    raise ValueError(f"one index per image into each table: got {tuple(idx.shape)} and {tuple(idx_r.shape)}")
  return _PoseFn.apply(q, t, idx, q_right, t_right, idx_r)


# ---- pose tables (camera_table/pose_table.py) ------------------------------------------------------------------------

class PoseTable(nn.Module):
  def __init__(self, m: torch.Tensor):
    super().__init__()
    if m.shape[-2:] != (4, 4):
      raise ValueError(f"Expected (..., 4, 4) tensor, got: {tuple(m.shape)}")
    R, t = split_rt(m)
    q = rotmat_to_unitquat(R)
    self.t = nn.Parameter(t.to(torch.float32), requires_grad=False)
    self.q = nn.Parameter(q.to(torch.float32), requires_grad=False)

  def forward(self, indices: Optional[torch.Tensor] = None) -> torch.Tensor:
    if indices is None:
      indices = torch.arange(self.q.shape[0], device=self.q.device)
    return pose_matrices(self.q, self.t, indices)

  @property
  def matrix(self) -> torch.Tensor:
    return self.forward()

  def __getitem__(self, idx: int) -> torch.Tensor:
    return self.forward(torch.tensor([idx])).squeeze(0)

  def normalize(self):
    self.q.data = F.normalize(self.q.data, dim=-1)
    return self

  def __len__(self):
    return self.t.shape[0]


class RigPoseTable(nn.Module):
  def __init__(self, rig_t_world: torch.Tensor, camera_t_rig: torch.Tensor):
    super().__init__()
    self.camera_t_rig = PoseTable(camera_t_rig)
    self.rig_t_world = PoseTable(rig_t_world)

  @property
  def num_cameras(self):
    return self.camera_t_rig.t.shape[0]

  @property
  def num_frames(self):
    return self.rig_t_world.t.shape[0]

  @property
  def rig_t_camera(self):
    return torch.linalg.inv(self.camera_t_rig.matrix)

  @property
  def world_t_rig(self):
    return torch.linalg.inv(self.rig_t_world.matrix)

  def normalize(self):
    self.camera_t_rig.normalize()
    self.rig_t_world.normalize()

  def __len__(self):
    return self.num_frames * self.num_cameras

  def forward(self, frame_idx: torch.Tensor, camera_idx: torch.Tensor) -> torch.Tensor:
    return pose_matrices(self.camera_t_rig.q, self.camera_t_rig.t, camera_idx,
                         self.rig_t_world.q, self.rig_t_world.t, frame_idx)


# ---- containers ------------------------------------------------------------------------------------------------------

def _select(key: Any, device: torch.device) -> Any:
  return key.to(device) if isinstance(key, torch.Tensor) else key


class Projections:
  """Projection parameters for a camera or a batch of cameras: the reference's tensorclass as a plain container with
  at most one batch dimension."""

  def __init__(self, intrinsics: torch.Tensor, image_size: torch.Tensor, depth_range: torch.Tensor, batch_size=None):
    self.intrinsics = intrinsics        # (..., 4) fx, fy, cx, cy
    self.image_size = image_size        # (..., 2) int
    self.depth_range = depth_range      # (..., 2) float
    shape = torch.Size(intrinsics.shape[:-1])
    if len(shape) > 1 or image_size.shape[:-1] != shape or depth_range.shape[:-1] != shape:
      raise ValueError(f"Projections takes at most one batch dimension, shared by its fields; got "
                       f"{tuple(intrinsics.shape)}, {tuple(image_size.shape)}, {tuple(depth_range.shape)}")
    if batch_size is not None and torch.Size(batch_size) != shape:
      raise ValueError(f"batch_size {tuple(batch_size)} does not match the fields' {tuple(shape)}")
    self.batch_size = shape

  @property
  def shape(self) -> torch.Size:
    return self.batch_size

  def __len__(self) -> int:
    if not self.batch_size:
      raise TypeError("a Projections without a batch dimension has no len()")
    return self.batch_size[0]

  def __getitem__(self, key) -> "Projections":
    if not self.batch_size:
      raise IndexError("a Projections without a batch dimension cannot be indexed")
    key = _select(key, self.device)
    return Projections(self.intrinsics[key], self.image_size[key], self.depth_range[key])

  def replace(self, **fields) -> "Projections":
    values = dict(intrinsics=self.intrinsics, image_size=self.image_size, depth_range=self.depth_range)
    unknown = set(fields) - set(values)
    if unknown:
      raise TypeError(f"Projections has no field {sorted(unknown)}")
    values.update(fields)
    return Projections(**values)

  def to(self, device) -> "Projections":
    return Projections(self.intrinsics.to(device), self.image_size.to(device), self.depth_range.to(device))

  @property
  def matrix(self) -> torch.Tensor:
    return to_matrix(self.intrinsics)

  @property
  def focal_length(self) -> torch.Tensor:
    return self.intrinsics[..., :2]

  @property
  def principal_point(self) -> torch.Tensor:
    return self.intrinsics[..., 2:]

  @property
  def aspect_ratio(self) -> torch.Tensor:
    return self.image_size[..., 0] / self.image_size[..., 1]

  @property
  def fov(self) -> torch.Tensor:
    return 2.0 * torch.atan(0.5 * self.image_size / self.focal_length)

  @property
  def device(self) -> torch.device:
    return self.intrinsics.device

  def __repr__(self):
    return f"Projections(batch_size={tuple(self.batch_size)}, device={self.device})"


@dataclass(kw_only=True)
class Camera:
  """Convenience class for a single camera."""
  intrinsics: torch.Tensor        # (4,) float
  camera_t_world: torch.Tensor    # (4, 4) float

  image_size: Tuple[int, int]
  depth_range: Tuple[float, float]

  camera_idx: int
  frame_idx: int
  label: Label

  image_name: str

  @property
  def device(self):
    return self.camera_t_world.device

  @property
  def matrix(self) -> torch.Tensor:
    return to_matrix(self.intrinsics)

  @property
  def position(self) -> torch.Tensor:
    return -(self.rotation @ self.world_t_camera[..., :3, 3:4]).squeeze(-1)

  @property
  def rotation(self) -> torch.Tensor:
    return self.world_t_camera[..., :3, :3].transpose(-1, -2)

  @property
  def world_t_camera(self) -> torch.Tensor:
    return torch.inverse(self.camera_t_world)

  def move_to(self, r: Optional[torch.Tensor] = None, t: Optional[torch.Tensor] = None) -> "Camera":
    r = r.transpose(-1, -2) if r is not None else self.camera_t_world[..., :3, :3]
    t = -(r @ t.unsqueeze(-1)).squeeze(-1) if t is not None else self.camera_t_world[..., :3, 3]
    return dataclasses.replace(self, camera_t_world=join_rt(r, t))

  def translated(self, vector: torch.Tensor) -> "Camera":
    return self.move_to(t=self.position + vector)

  def scaled(self, scale: float) -> "Camera":
    return self.move_to(t=self.position * scale)

  @property
  def near(self) -> float:
    return self.depth_range[0]

  @property
  def far(self) -> float:
    return self.depth_range[1]

  @property
  def focal_length(self) -> torch.Tensor:
    return self.intrinsics[..., :2]

  @property
  def principal_point(self) -> torch.Tensor:
    return self.intrinsics[..., 2:]

  @property
  def aspect_ratio(self) -> float:
    return self.image_size[0] / self.image_size[1]

  @property
  def fov(self) -> torch.Tensor:
    f = self.focal_length
    return 2.0 * torch.atan(0.5 * torch.tensor(self.image_size, device=self.device) / f)

  def has_label(self, label: Label) -> bool:
    return bool(self.label & label)

  def resized(self, image_scale: float) -> "Camera":
    return dataclasses.replace(
        self, intrinsics=self.intrinsics * image_scale,
        image_size=(int(self.image_size[0] * image_scale), int(self.image_size[1] * image_scale)))

  def to_camera_params(self) -> CameraParams:
    return CameraParams(projection=self.intrinsics, T_camera_world=self.camera_t_world,
                        near_plane=self.depth_range[0], far_plane=self.depth_range[1], image_size=self.image_size)


_CAMERAS_FIELDS = ("camera_t_world", "projection", "camera_idx", "frame_idx", "labels", "image_names")


class Cameras:
  """Either a single camera or a batch of cameras: the reference's tensorclass as a plain container with at most one
  batch dimension.  Indexing with an int drops the dimension; a slice, an index tensor or a mask keeps it."""

  def __init__(self, camera_t_world: torch.Tensor, projection: Projections, camera_idx: torch.Tensor,
               frame_idx: torch.Tensor, labels: torch.Tensor, image_names: List[str], batch_size=None):
    self.camera_t_world = camera_t_world        # (..., 4, 4) float
    self.projection = projection
    self.camera_idx = camera_idx                # (...) int
    self.frame_idx = frame_idx                  # (...) int
    self.labels = labels                        # (...) int
    self.image_names = list(image_names)
    shape = torch.Size(camera_t_world.shape[:-2])
    if len(shape) > 1 or any(torch.Size(s) != shape for s in (projection.batch_size, camera_idx.shape, frame_idx.shape,
                                                              labels.shape)):
      raise ValueError(f"Cameras takes at most one batch dimension, shared by its fields; got camera_t_world "
                       f"{tuple(camera_t_world.shape)}, projection {tuple(projection.batch_size)}, camera_idx "
                       f"{tuple(camera_idx.shape)}, frame_idx {tuple(frame_idx.shape)}, labels {tuple(labels.shape)}")
    if batch_size is not None and torch.Size(batch_size) != shape:
      raise ValueError(f"batch_size {tuple(batch_size)} does not match the fields' {tuple(shape)}")
    if len(self.image_names) != (shape[0] if shape else 1):
      raise ValueError(f"expected {shape[0] if shape else 1} image names, got {len(self.image_names)}")
    self.batch_size = shape
    self._world_t_camera = None

  @property
  def shape(self) -> torch.Size:
    return self.batch_size

  def __len__(self) -> int:
    if not self.batch_size:
      raise TypeError("a Cameras without a batch dimension has no len()")
    return self.batch_size[0]

  def __getitem__(self, key) -> "Cameras":
    if not self.batch_size:
      raise IndexError("a Cameras without a batch dimension cannot be indexed")
    key = _select(key, self.device)
    if isinstance(key, int):
      names = [self.image_names[key]]
    elif isinstance(key, slice):
      names = self.image_names[key]
    elif isinstance(key, torch.Tensor):
      rows = torch.nonzero(key, as_tuple=True)[0] if key.dtype is torch.bool else key.reshape(-1)
      names = [self.image_names[i] for i in rows.tolist()]
    else:
      raise IndexError(f"Cameras is indexed by an int, a slice, an index tensor or a mask, got {type(key).__name__}")
    return Cameras(self.camera_t_world[key], self.projection[key], self.camera_idx[key], self.frame_idx[key],
                   self.labels[key], names)

  def replace(self, **fields) -> "Cameras":
    values = {name: getattr(self, name) for name in _CAMERAS_FIELDS}
    unknown = set(fields) - set(values)
    if unknown:
      raise TypeError(f"Cameras has no field {sorted(unknown)}")
    values.update(fields)
    return Cameras(**values)

  def to(self, device) -> "Cameras":
    return Cameras(self.camera_t_world.to(device), self.projection.to(device), self.camera_idx.to(device),
                   self.frame_idx.to(device), self.labels.to(device), self.image_names)

  @property
  def device(self):
    return self.camera_t_world.device

  @property
  def positions(self) -> torch.Tensor:
    return -(self.rotations @ self.world_t_camera[..., :3, 3:4]).squeeze(-1)

  @property
  def rotations(self) -> torch.Tensor:
    return self.camera_t_world[..., :3, :3].transpose(-1, -2)

  @property
  def world_t_camera(self) -> torch.Tensor:
    if self._world_t_camera is None:              # (the reference's cached_property)
      self._world_t_camera = torch.inverse(self.camera_t_world)
    return self._world_t_camera

  @property
  def right(self) -> torch.Tensor:
    return self.world_t_camera[..., :3, 0]

  @property
  def up(self) -> torch.Tensor:
    return self.world_t_camera[..., :3, 1]

  @property
  def forward(self) -> torch.Tensor:
    return -self.rotations[..., :3, 2]

  @property
  def intrinsics(self) -> torch.Tensor:
    return self.projection.intrinsics

  @property
  def image_sizes(self) -> torch.Tensor:
    return self.projection.image_size

  def has_label(self, label: Label) -> torch.Tensor:
    """Indices of the cameras with the given label (labels are bitwise encoded)."""
    return torch.nonzero(self.labels & label.value, as_tuple=True)[0]

  def with_label(self, label: Label) -> "Cameras":
    return self[self.has_label(label)]

  def count_label(self, label: Label) -> int:
    return self.has_label(label).shape[0]

  def move_to(self, r: Optional[torch.Tensor] = None, t: Optional[torch.Tensor] = None) -> "Cameras":
    r = r.transpose(-1, -2) if r is not None else self.camera_t_world[..., :3, :3]
    t = -(r @ t.unsqueeze(-1)).squeeze(-1) if t is not None else self.camera_t_world[..., :3, 3]
    return self.replace(camera_t_world=join_rt(r, t))

  def scaled(self, scale: float) -> "Cameras":
    return self.move_to(t=self.positions * scale)

  def translated(self, translation: torch.Tensor) -> "Cameras":
    return self.move_to(t=self.positions + translation)

  def clamp_near(self, near: float) -> "Cameras":
    depth_range = torch.clamp_min(self.projection.depth_range, near)
    return self.replace(projection=self.projection.replace(depth_range=depth_range))

  def item(self) -> Camera:
    if self.batch_size and self.batch_size[0] != 1:
      raise ValueError(f"Expected batch size 1, got shape: {tuple(self.batch_size)}")
    return Camera(
        intrinsics=self.intrinsics.reshape(4),
        camera_t_world=self.camera_t_world.reshape(4, 4),
        image_size=tuple(self.image_sizes.reshape(2).cpu().tolist()),
        depth_range=tuple(self.projection.depth_range.reshape(2).cpu().tolist()),
        camera_idx=int(self.camera_idx.item()),
        frame_idx=int(self.frame_idx.item()),
        label=Label(int(self.labels.item())),
        image_name=self.image_names[0])

  def __repr__(self):
    return f"Cameras(batch_size={tuple(self.batch_size)}, device={self.device})"


# ---- camera tables ---------------------------------------------------------------------------------------------------

class _ProjectionTable(nn.Module):
  """The projection table's three tensors as frozen parameters (the reference wraps a tensordict in TensorDictParams)."""

  def __init__(self, projection: Projections):
    super().__init__()
    self.intrinsics = nn.Parameter(projection.intrinsics.detach().clone(), requires_grad=False)
    self.image_size = nn.Parameter(projection.image_size.detach().clone(), requires_grad=False)
    self.depth_range = nn.Parameter(projection.depth_range.detach().clone(), requires_grad=False)

  def projections(self) -> Projections:
    return Projections(self.intrinsics.data, self.image_size.data, self.depth_range.data)


class CameraTable(nn.Module, metaclass=abc.ABCMeta):

  @abc.abstractmethod
  def forward(self, image_idx: torch.Tensor) -> Cameras:
    raise NotImplementedError

  @property
  def num_projections(self) -> int:
    return self.projections.batch_size[0]

  @property
  def projections(self) -> Projections:
    return self._camera_projection.projections()

  @property
  @abc.abstractmethod
  def num_frames(self) -> int:
    raise NotImplementedError

  @property
  @abc.abstractmethod
  def num_images(self) -> int:
    raise NotImplementedError

  def __len__(self):
    return self.num_images

  @property
  def device(self) -> torch.device:
    return self.projections.device

  @property
  def image_names(self) -> List[str]:
    return self._image_names

  @property
  def cameras(self) -> Cameras:
    return self.forward(torch.arange(self.num_images))

  def __getitem__(self, image_idx) -> Cameras:
    if isinstance(image_idx, int):
      image_idx = torch.tensor([image_idx])
    return self.forward(image_idx)

  def _names(self, image_idx: Any) -> List[str]:
    """The names of the selected images.  The list is read on the host (of a device index that is a wait, as in the
    reference), so the range check it allows is made here."""
    rows = torch.as_tensor(image_idx).reshape(-1).tolist()
    for i in rows:
      if not 0 <= i < self.num_images:
        raise _lib.GsplatHipError(f"image_idx out of range: {i} is not in [0, {self.num_images})")
    return [self._image_names[i] for i in rows]


class CameraRigTable(CameraTable):
  def __init__(self, rig_t_world: torch.Tensor,      # (N, 4, 4) poses of the whole camera rig
               camera_t_rig: torch.Tensor,           # (C, 4, 4) camera poses inside the rig
               projection: Projections,              # (C,) camera projections
               image_names: List[str],               # (N * C,)
               labels: torch.Tensor):                # (N * C,)
    super().__init__()
    num_cameras, num_frames = camera_t_rig.shape[0], rig_t_world.shape[0]
    if projection.shape[0] != num_cameras:
      raise ValueError(f"Expected equal number of cameras and projections, got: {projection.shape[0]} != {num_cameras}")
    if len(image_names) != num_cameras * num_frames:
      raise ValueError(f"Incorrect number of image names, got: {len(image_names)} != {num_cameras * num_frames}")
    self._camera_projection = _ProjectionTable(projection)
    self._camera_poses = RigPoseTable(rig_t_world=rig_t_world, camera_t_rig=camera_t_rig)
    self._camera_poses.requires_grad_(False)
    self._image_names = list(image_names)
    self.register_buffer("_labels", labels)

  def forward(self, image_idx: torch.Tensor) -> Cameras:
    names = self._names(image_idx)
    image_idx = _index(image_idx, self.num_images, self.device, "image_idx")
    num_cameras = self._camera_poses.num_cameras
    frame_idx = image_idx // num_cameras
    camera_idx = image_idx % num_cameras
    return Cameras(camera_t_world=self._camera_poses(frame_idx, camera_idx), projection=self.projections[camera_idx],
                   camera_idx=camera_idx, frame_idx=frame_idx, batch_size=image_idx.shape,
                   labels=self._labels[image_idx], image_names=names)

  @property
  def num_images(self) -> int:
    return self._camera_poses.num_frames * self._camera_poses.num_cameras

  @property
  def num_frames(self) -> int:
    return self._camera_poses.num_frames


class MultiCameraTable(CameraTable):
  """A table of camera poses and intrinsics: cameras can have different intrinsics, which are stored in the projection
  table."""

  def __init__(self, camera_t_world: torch.Tensor,   # (N, 4, 4)
               camera_idx: torch.Tensor,             # (N,) index into the projection table (0 .. P-1)
               projection: Projections,              # (P,)
               image_names: List[str],               # (N,)
               labels: torch.Tensor):                # (N,)
    super().__init__()
    if camera_t_world.shape[0] != camera_idx.shape[0]:
      raise ValueError(f"Expected equal number of cameras and indices, got: {camera_t_world.shape[0]} != "
                       f"{camera_idx.shape[0]}")
    if len(image_names) != camera_t_world.shape[0]:
      raise ValueError(f"Expected equal number of image names and cameras, got: {len(image_names)} != "
                       f"{camera_t_world.shape[0]}")
    self._camera_projection = _ProjectionTable(projection)
    self.register_buffer("_camera_idx", camera_idx)
    self._camera_t_world = PoseTable(camera_t_world)
    self._camera_t_world.requires_grad_(False)
    self._image_names = list(image_names)
    self.register_buffer("_labels", labels)

  def forward(self, image_idx: torch.Tensor) -> Cameras:
    names = self._names(image_idx)
    image_idx = _index(image_idx, self.num_images, self.device, "image_idx")
    cam_idx = self._camera_idx[image_idx]
    return Cameras(camera_t_world=self._camera_t_world(image_idx), projection=self.projections[cam_idx],
                   camera_idx=cam_idx, frame_idx=image_idx, batch_size=image_idx.shape, labels=self._labels[image_idx],
                   image_names=names)

  @property
  def num_images(self) -> int:
    return len(self._camera_t_world)

  @property
  def num_frames(self) -> int:
    return self.num_images


# ---- functions -------------------------------------------------------------------------------------------------------

def camera_scene_extents(cameras: Cameras) -> Tuple[torch.Tensor, float]:
  """Centroid and "diagonal" of the camera centres, exactly as the reference computes them: the norm runs over
  dimension 0 (the cameras), per coordinate, and the largest of the three is scaled by 1.1."""
  cam_centers = cameras.positions.reshape(-1, 3)
  avg_cam_center = torch.mean(cam_centers, dim=0, keepdim=True)
  distances = torch.norm(cam_centers - avg_cam_center, dim=0, keepdim=True)
  diagonal = torch.max(distances)
  return avg_cam_center.reshape(3), (diagonal * 1.1).item()


def pose_adjacency(poses1: torch.Tensor, poses2: torch.Tensor, k: int = 8) -> torch.Tensor:
  """Similarity between every pose of ``poses1`` (N, 4, 4) and of ``poses2`` (M, 4, 4): higher for poses that are
  closer and similarly oriented, the distance scaled by the median of the k + 1 nearest distances."""
  forward1, forward2 = poses1[..., :3, 2], poses2[..., :3, 2]
  dir_similarity = torch.einsum('id,jd->ij', forward1, forward2)
  pos1, pos2 = poses1[..., :3, 3], poses2[..., :3, 3]
  distance = torch.cdist(pos1, pos2)
  knn_distances, _ = torch.topk(distance, k=min(k + 1, distance.shape[1]), dim=1, largest=False)
  local_scale = knn_distances.median()
  dist_similarity = 1.0 / (1.0 + distance / local_scale)
  return dir_similarity * dist_similarity


def camera_similarity(cameras: Cameras, world_t_camera: torch.Tensor) -> torch.Tensor:
  if world_t_camera.shape != (4, 4):
    raise ValueError(f"Expected shape (4, 4), got: {tuple(world_t_camera.shape)}")
  return pose_adjacency(cameras.world_t_camera, world_t_camera.unsqueeze(0))


def camera_adjacency_matrix(cameras: Cameras) -> torch.Tensor:
  return pose_adjacency(cameras.world_t_camera, cameras.world_t_camera)


def camera_json(cameras: Cameras):
  def export_camera(i):
    camera = cameras[i].item()
    fx, fy, cx, cy = camera.intrinsics.tolist()
    near, far = camera.depth_range
    width, height = camera.image_size
    return {"id": i, "position": camera.position.tolist(), "rotation": camera.rotation.tolist(),
            "fx": fx, "fy": fy, "cx": cx, "cy": cy, "width": width, "height": height, "near": near, "far": far,
            "img_name": camera.image_name}

  return [export_camera(i) for i in range(len(cameras))]
