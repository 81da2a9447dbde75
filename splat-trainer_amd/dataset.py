"""The data interfaces the trainer is written against (the reference's ``dataset/dataset.py``, ``dataset/util.py`` and
``util/pointcloud.py``): ``ImageView``, the abstract ``Dataset``, ``PointCloud``, the split helpers, and ``TensorDataset``,
a dataset held in memory.  The COLMAP loader is ``colmap.COLMAPDataset``; the reference's scan loader needs a package
this project does not depend on and is not here: for other sources a user fills a ``TensorDataset`` or subclasses
``Dataset``.
"""
from __future__ import annotations

from abc import ABCMeta, abstractmethod
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ply_io
from .camera_table import CameraTable, Label
from .normalization import Normalization, NormalizationConfig


@dataclass
class ImageView:
  filename: str
  image_idx: int
  image: torch.Tensor            # (H, W, 3): uint8 as a dataset hands it out, float in [0, 1] once the trainer has loaded it


class PointCloud:
  """Points (N, 3) and colours (N, 3, in [0, 1]) on one device."""

  def __init__(self, points: torch.Tensor, colors: torch.Tensor, batch_size=None):
    if points.dim() != 2 or points.shape[1] != 3 or tuple(colors.shape) != tuple(points.shape):
      raise ValueError(f"points and colors must both be (N, 3), got {tuple(points.shape)} and {tuple(colors.shape)}")
    if batch_size is not None and tuple(batch_size) != (points.shape[0],):
      raise ValueError(f"batch_size {tuple(batch_size)} does not match {points.shape[0]} points")
    self.points, self.colors = points, colors

  @property
  def num_points(self) -> int:
    return self.points.shape[0]

  @property
  def batch_size(self) -> Tuple[int]:
    return (self.points.shape[0],)

  @property
  def device(self) -> torch.device:
    return self.points.device

  def __len__(self) -> int:
    return self.num_points

  def __repr__(self):
    return f"PointCloud({self.num_points} points, {self.device})"

  def __getitem__(self, key) -> "PointCloud":
    if isinstance(key, int):
      key = slice(key, key + 1) if key != -1 else slice(key, None)
    return PointCloud(self.points[key], self.colors[key])

  def to(self, device) -> "PointCloud":
    return PointCloud(self.points.to(device), self.colors.to(device))

  @staticmethod
  def from_numpy(xyz: np.ndarray, rgb: np.ndarray) -> "PointCloud":
    if rgb.dtype == np.uint8:
      rgb = rgb.astype(np.float32) / 255.0
    return PointCloud(torch.from_numpy(xyz.astype(np.float32)), torch.from_numpy(rgb.astype(np.float32)))

  def append(self, other: "PointCloud") -> "PointCloud":
    return PointCloud(torch.cat([self.points, other.points], dim=0), torch.cat([self.colors, other.colors], dim=0))

  def translated(self, translation: torch.Tensor) -> "PointCloud":
    return PointCloud(self.points + translation, self.colors)

  def scaled(self, scale: float) -> "PointCloud":
    return PointCloud(self.points * scale, self.colors)

  def save_ply(self, filename: Union[str, Path]) -> None:
    """x, y, z and red, green, blue (0..255) as the float properties ``ply_io.write_ply`` writes."""
    vertex = np.zeros(self.num_points, dtype=[(n, "<f4") for n in ("x", "y", "z", "red", "green", "blue")])
    xyz = self.points.detach().cpu().numpy()
    rgb = np.floor(self.colors.detach().cpu().numpy().clip(0.0, 1.0) * 255.0)
    for i, name in enumerate(("x", "y", "z")):
      vertex[name] = xyz[:, i]
    for i, name in enumerate(("red", "green", "blue")):
      vertex[name] = rgb[:, i]
    ply_io.write_ply(filename, vertex)

  @staticmethod
  def load_ply(filename: Union[str, Path]) -> "PointCloud":
    vertex = ply_io.read_ply(filename)
    xyz = np.stack([vertex[n] for n in ("x", "y", "z")], axis=1)
    rgb = np.stack([vertex[n] for n in ("red", "green", "blue")], axis=1).astype(np.float32) / 255.0
    return PointCloud.from_numpy(xyz, rgb)


class Dataset(metaclass=ABCMeta):
  @abstractmethod
  def loader(self, idx: torch.Tensor, shuffle: bool = False) -> Sequence[ImageView]:
    raise NotImplementedError

  @property
  @abstractmethod
  def to_original(self) -> Normalization:
    """The transform back to the original coordinates."""
    raise NotImplementedError

  @abstractmethod
  def train(self, shuffle: bool = True) -> Sequence[ImageView]:
    raise NotImplementedError

  @abstractmethod
  def val(self) -> Sequence[ImageView]:
    raise NotImplementedError

  @property
  @abstractmethod
  def camera_table(self) -> CameraTable:
    raise NotImplementedError

  @abstractmethod
  def pointcloud(self) -> Optional[PointCloud]:
    raise NotImplementedError

  @abstractmethod
  def load_images(self):
    raise NotImplementedError


def partition_stride(idx: torch.Tensor, val_stride: int) -> Tuple[torch.Tensor, torch.Tensor]:
  """(train, val): every ``val_stride``-th entry of ``idx`` is validation; training keeps the entries whose VALUE is no
  multiple of ``val_stride`` (as the reference does: with a ``padding`` that is no multiple of the stride the two differ)."""
  if val_stride == 0:
    raise ValueError("val_stride must not be 0")
  return idx[idx % val_stride != 0], idx[::val_stride]


def split_every(n: int, test_every: int = 8, padding: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
  """(train, val) indices of ``n`` frames less ``padding`` at both ends: every ``test_every``-th is validation, none with
  ``test_every`` <= 0."""
  idx = torch.arange(padding, n - padding, dtype=torch.long)
  if test_every > 0:
    return partition_stride(idx, test_every)
  return idx, torch.empty(0, dtype=torch.long)


def expand_index(idx: torch.Tensor, num_cameras: int) -> torch.Tensor:
  """Frame indices to image indices of a rig of ``num_cameras``: frame f becomes f * num_cameras + (0 .. num_cameras - 1)."""
  return (idx.reshape(-1, 1) * num_cameras + torch.arange(num_cameras, device=idx.device).reshape(1, -1)).reshape(-1)


class TensorDataset(Dataset):
  """A dataset in memory: a camera table (already in normalised coordinates), one uint8 (H, W, 3) image per row of it, an
  optional point cloud (normalised too) and the ``Normalization`` that was applied.  ``train_idx`` / ``val_idx`` default
  to the rows labelled ``Label.Training`` / ``Label.Validation``.  Nothing here touches the GPU.  (The images stay in
  pageable memory: page-locked ones made the trainer's per-step upload of a small image slower, not faster, when
  measured -- profiles/r22_trainer.txt.)"""

  def __init__(self, camera_table: CameraTable, images: Sequence[torch.Tensor], cloud: Optional[PointCloud] = None,
               normalization: Optional[Normalization] = None, train_idx: Optional[torch.Tensor] = None,
               val_idx: Optional[torch.Tensor] = None):
    images = list(images)
    if len(images) != camera_table.num_images:
      raise ValueError(f"{len(images)} images for a camera table of {camera_table.num_images}")
    for i, image in enumerate(images):
      if image.dtype is not torch.uint8 or image.dim() != 3 or image.shape[2] != 3 or image.is_cuda:
        raise ValueError(f"image {i} must be a uint8 (H, W, 3) CPU tensor, got {image.dtype} {tuple(image.shape)} "
                         f"on {image.device}")
    self._camera_table = camera_table
    self._images = images
    self._cloud = cloud
    self._normalization = normalization or Normalization(config=NormalizationConfig(), translation=torch.zeros(3),
                                                          scaling=1.0)
    labels = camera_table._labels.cpu()
    by_label = lambda label: torch.tensor([i for i, v in enumerate(labels.tolist()) if Label(v) & label], dtype=torch.long)
    self.train_idx = by_label(Label.Training) if train_idx is None else train_idx.cpu().to(torch.long)
    self.val_idx = by_label(Label.Validation) if val_idx is None else val_idx.cpu().to(torch.long)

  def __repr__(self):
    return f"TensorDataset({len(self._images)} images, train {len(self.train_idx)}, val {len(self.val_idx)})"

  def _view(self, i: int) -> ImageView:
    return ImageView(self._camera_table.image_names[i], i, self._images[i])

  def loader(self, idx: torch.Tensor, shuffle: bool = False) -> List[ImageView]:
    rows = torch.as_tensor(idx).reshape(-1).cpu()
    if shuffle:
      rows = rows[torch.randperm(rows.shape[0])]
    return [self._view(int(i)) for i in rows.tolist()]

  @property
  def to_original(self) -> Normalization:
    return self._normalization.inverse

  def train(self, shuffle: bool = True) -> List[ImageView]:
    return self.loader(self.train_idx, shuffle=shuffle)

  def val(self) -> List[ImageView]:
    return self.loader(self.val_idx)

  @property
  def camera_table(self) -> CameraTable:
    return self._camera_table

  def pointcloud(self) -> Optional[PointCloud]:
    return self._cloud

  def load_images(self):
    pass                                   # (already in memory)
