"""Scene normalisation: the reference's ``splat_trainer.dataset.normalization`` (``Normalization``,
``NormalizationConfig``, ``median_knn``).  A normalisation is a translation followed by a uniform scaling,
``x -> scaling * (x + translation)``, applied alike to points, Gaussians, cameras and rigid transforms.

``median_knn`` goes through the native brute-force ``knn`` (csrc/neighbours.hip) in place of the reference's N x N
``cdist`` and sort.  The reference takes column ``k - 1`` of the sorted distances with the point itself in column 0; the
native ``knn`` leaves the point itself out, so that column is the ``k - 1``-th nearest other point (and ``k = 1`` is the
point itself, distance 0).  ``knn`` holds at most 16 neighbours: ``k`` above 17 raises (the reference's default
``normalize_knn = 20`` is out of reach; there is no second path).  Points on the HIP device only.

``transform_cloud`` takes a ``dataset.PointCloud``; that module imports this one, so the class is looked up on the call.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from .camera_table import Cameras, join_rt, split_rt
from .data_types import Gaussians3D
from .neighbours import knn


def median_knn(positions: torch.Tensor, k: int = 10) -> torch.Tensor:
  """The median over the points of the distance to the ``k - 1``-th nearest other point: a 0-D float32 tensor."""
  if isinstance(k, bool) or not isinstance(k, int) or k < 1:
    raise ValueError(f"k must be an int >= 1, got {k!r}")
  if k - 1 > _lib.KNN_MAX_K:
    raise ValueError(f"median_knn with k={k} needs {k - 1} neighbours; the native kNN holds at most {_lib.KNN_MAX_K}")
  if k == 1:
    return torch.zeros((), dtype=torch.float32, device=positions.device)
  dist2, _ = knn(positions.to(torch.float32), k - 1)
  return torch.median(torch.sqrt(dist2[:, k - 2]))


@dataclass
class Normalization:
  config: 'NormalizationConfig'
  translation: torch.Tensor
  scaling: float

  def transform_gaussians(self, gaussians: Gaussians3D) -> Gaussians3D:
    return gaussians.translated(self.translation.to(gaussians.position.device)).scaled(self.scaling)

  def transform_cameras(self, cameras: Cameras) -> Cameras:
    return cameras.translated(self.translation.to(cameras.device)).scaled(self.scaling)

  def transform_points(self, points: torch.Tensor) -> torch.Tensor:      # (..., 3) -> (..., 3)
    t = self.translation.to(points.device)
    while len(t.shape) < len(points.shape):
      t = t.unsqueeze(0)
    return self.scaling * (points + t)

  def transform_cloud(self, cloud):
    """A ``PointCloud`` with the points transformed and the colours as they are."""
    from .dataset import PointCloud
    return PointCloud(self.transform_points(cloud.points), cloud.colors)

  def transform_rigid(self, rigid: torch.Tensor) -> torch.Tensor:
    r, t = split_rt(rigid)
    return join_rt(r, self.transform_points(t))

  @property
  def inverse(self) -> 'Normalization':
    return Normalization(config=self.config, translation=self.scaling * -self.translation, scaling=1.0 / self.scaling)

  def __repr__(self):
    translation_str = [f"{val:.3f}" for val in self.translation.tolist()]
    return f"Normalization(translation={translation_str}, scaling={self.scaling:.3f})"


@dataclass
class NormalizationConfig:
  centering: bool = True
  scaling_method: str = "none"  # 'none', 'median_knn'
  normalize_knn: int = 20

  def get_transform(self, positions: torch.Tensor) -> Normalization:
    if self.scaling_method == "none":
      scale = 1.0
    elif self.scaling_method == "median_knn":
      scale = float(median_knn(positions, k=self.normalize_knn))
    else:
      raise ValueError(f"Unknown scaling method: {self.scaling_method}, options are: none, median_knn")
    mean = (torch.mean(positions, dim=0).to(torch.float32) if self.centering
            else torch.zeros(3, dtype=torch.float32))
    return Normalization(config=self, translation=-mean, scaling=1.0 / scale)

  def __repr__(self) -> str:
    return (f"NormalizationConfig(centering={self.centering}, scaling_method={self.scaling_method}, "
            f"normalize_knn={self.normalize_knn})")
