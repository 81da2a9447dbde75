"""Initial Gaussians from a point cloud (the reference's ``gaussians/loading.py`` and ``trainer/init.py``) over this
package's ``crop_cloud``, ``balanced_cloud`` (frustum queries, visibility.py) and ``estimate_scale`` (native kNN,
neighbours.py).

Every random draw made here -- the subsample of a cloud that is over the limit, the initial rotations -- takes an
optional CPU ``generator``; ``balanced_cloud``, which fills up with random points inside the frusta, draws on the device
from torch's global generator as it always has.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from .data_types import Gaussians3D
from .dataset import Dataset, PointCloud
from .neighbours import estimate_scale
from .visibility import balanced_cloud, crop_cloud


@dataclass(frozen=True, kw_only=True)
class CloudInitConfig:
  num_neighbors: int
  initial_point_scale: float
  initial_alpha: float

  limit_points: Optional[int] = None
  initial_points: Optional[int] = None

  min_view_overlap: int = 4
  clamp_near: float = 0.0


def inverse_sigmoid(x: float) -> float:
  return math.log(x / (1.0 - x))


def from_scaled_pointcloud(pcd: PointCloud, scales: torch.Tensor, initial_alpha: float = 0.5,
                           generator: Optional[torch.Generator] = None) -> Gaussians3D:
  """Isotropic Gaussians at the points with the given scales (N,), random unit rotations, opacity ``initial_alpha`` (less
  1e-4, so that 1 stays finite) and the cloud's colours as the feature."""
  n, device = pcd.num_points, pcd.points.device
  rotation = F.normalize(torch.randn(n, 4, generator=generator), dim=1).to(device)
  return Gaussians3D(position=pcd.points, log_scaling=torch.log(scales).unsqueeze(1).expand(-1, 3).contiguous(),
                     rotation=rotation,
                     alpha_logit=torch.full((n, 1), inverse_sigmoid(initial_alpha - 1e-4), device=device),
                     feature=pcd.colors, batch_size=(n,))


def from_pointcloud(pcd: PointCloud, initial_scale: float = 0.5, initial_alpha: float = 0.5, num_neighbors: int = 3,
                    generator: Optional[torch.Generator] = None) -> Gaussians3D:
  scales = estimate_scale(pcd, num_neighbors=num_neighbors) * initial_scale
  return from_scaled_pointcloud(pcd, scales, initial_alpha, generator=generator)


def to_pointcloud(gaussians: Gaussians3D) -> PointCloud:
  return PointCloud(gaussians.position.detach(), gaussians.feature.detach())


def get_initial_gaussians(config: CloudInitConfig, dataset: Dataset, device, generator: Optional[torch.Generator] = None
                          ) -> Gaussians3D:
  """trainer/init.py: the dataset's cloud cropped to what the cameras see and cut down to ``limit_points`` /
  ``initial_points`` at random, filled up to ``initial_points`` (or made from nothing) with random points that at least
  ``min_view_overlap`` cameras see, scaled by the mean distance to the ``num_neighbors`` nearest points."""
  device = torch.device(device)
  cameras = dataset.camera_table.to(device).cameras
  points = dataset.pointcloud()
  if points is not None:
    points = crop_cloud(cameras, points.to(device))
    if points.num_points == 0:
      raise ValueError("No points visible in dataset images, check input data!")
    limit = points.num_points if config.limit_points is None else config.limit_points
    if config.initial_points is not None:
      limit = min(limit, config.initial_points)
    if limit < points.num_points:
      points = points[torch.randperm(points.num_points, generator=generator)[:limit].to(device)]
  if config.initial_points is not None or points is None:
    n = config.initial_points or 0
    if n == 0:
      raise ValueError("the dataset has no point cloud and CloudInitConfig.initial_points is not set")
    points = PointCloud(*balanced_cloud(cameras.clamp_near(config.clamp_near), n, config.min_view_overlap, points))
  scales = estimate_scale(points, num_neighbors=config.num_neighbors)
  return from_scaled_pointcloud(points, scales * config.initial_point_scale, initial_alpha=config.initial_alpha,
                                generator=generator)
