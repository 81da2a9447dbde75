"""Brute-force neighbour searches over 3-D points: drop-ins for the two pykeops users of the reference,
``splat_trainer.gaussians.loading.estimate_scale`` and ``splat_trainer.visibility.cluster`` (``assign_clusters``,
``kmeans_iter``, ``kmeans``), on HIP kernels (csrc/neighbours.hip).  Same signatures as the reference.

The squared distance is pinned, ``d = fmaf(dz, dz, fmaf(dy, dy, dx * dx))`` with ``dx = q.x - c.x`` and so on, and
every sum has a fixed order (no float atomics): results are bit-reproducible.  Inputs are (N, 3) / (K, 3) float32
tensors on the HIP device (non-contiguous ones are copied); anything else raises ValueError.  There is no CPU fallback.

One departure from the reference: a cluster that receives no points keeps its previous centroid (the reference divides
0 by 0 there).
"""
from __future__ import annotations

from typing import Any, Tuple

import torch

from . import _lib
from ._args import require
from ._lib import ptr as _ptr


def _cloud(x: Any, name: str) -> torch.Tensor:
  """``x`` as the searches take it: (N, 3) float32 on the HIP device (ValueError otherwise), 1..NEIGHBOURS_MAX_N rows,
  contiguous."""
  require(name, x, shape=("N", 3), dtype=torch.float32, what="the neighbour search", device_error=ValueError)
  if not 1 <= x.shape[0] <= _lib.NEIGHBOURS_MAX_N:
    raise ValueError(f"{name} must hold 1..{_lib.NEIGHBOURS_MAX_N} points, got {x.shape[0]}")
  return x if x.is_contiguous() else x.contiguous()


def _knn(points: torch.Tensor, k: int, want_scale: bool):
  p = _cloud(points, "points")
  N = p.shape[0]
  if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.KNN_MAX_K:
    raise ValueError(f"k must be an int in 1..{_lib.KNN_MAX_K}, got {k!r}")
  if N < k + 1:
    raise ValueError(f"kNN with k={k} needs at least k + 1 = {k + 1} points, got {N}")
  with _lib.on_device(p.device) as stream:
    dist2 = torch.empty((N, k), dtype=torch.float32, device=p.device)
    idx = torch.empty((N, k), dtype=torch.int64, device=p.device)
    scale = torch.empty(N, dtype=torch.float32, device=p.device) if want_scale else None
    ws = _lib.workspace(_lib.load().gsr_knn_workspace_bytes(N, k), p.device)
    _lib.call("gsr_knn", _ptr(p), N, k, _ptr(dist2), _ptr(idx), _ptr(scale), _ptr(ws), ws.numel(), stream)
  return dist2, idx, scale


def knn(points: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
  """For each point i the k nearest points j != i: ``(dist2 (N, k) float32, idx (N, k) int64)``, ascending squared
  distance, equal distances by lower j.  1 <= k <= 16 and N >= k + 1."""
  dist2, idx, _ = _knn(points, k, False)
  return dist2, idx


def estimate_scale(pointcloud: Any, num_neighbors: int = 3) -> torch.Tensor:
  """The mean distance to the ``num_neighbors`` nearest other points, (N,) float32: sqrt of each squared distance,
  summed in ascending order, divided by ``num_neighbors``.  ``pointcloud`` is an (N, 3) tensor or any object with a
  ``.points`` tensor (the reference's PointCloud)."""
  points = pointcloud if isinstance(pointcloud, torch.Tensor) else getattr(pointcloud, "points", pointcloud)
  return _knn(points, num_neighbors, True)[2]


def _centroids(centroids: Any, x: torch.Tensor) -> torch.Tensor:
  c = _cloud(centroids, "centroids")
  if c.device != x.device:
    raise ValueError(f"x on {x.device} and centroids on {c.device}")
  return c


def assign_clusters(x: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
  """The nearest centroid of every point, (N,) int64: argmin over j of the squared distance, ties to the lowest j; a
  point whose distances are all NaN gets 0."""
  xp = _cloud(x, "x")
  c = _centroids(centroids, xp)
  with _lib.on_device(xp.device) as stream:
    labels = torch.empty(xp.shape[0], dtype=torch.int64, device=xp.device)
    _lib.call("gsr_assign_clusters", _ptr(xp), xp.shape[0], _ptr(c), c.shape[0], _ptr(labels), stream)
  return labels


def kmeans_iter(x: torch.Tensor, centroids: torch.Tensor, iters: int = 100) -> Tuple[torch.Tensor, torch.Tensor]:
  """``iters`` Lloyd iterations, enqueued by one native call: assign every point, then set each centroid to the float32
  mean of its points (an empty cluster keeps its centroid).  Updates ``centroids`` in place and returns
  ``(labels, centroids)``; the labels are those of the last assignment, made before the last update."""
  xp = _cloud(x, "x")
  c = _centroids(centroids, xp)           # a copy when centroids is not contiguous: written back below
  if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= 2**31 - 1:
    raise ValueError(f"iters must be an int >= 1, got {iters!r}")
  N, K = xp.shape[0], centroids.shape[0]
  with _lib.on_device(xp.device) as stream:
    labels = torch.empty(N, dtype=torch.int64, device=xp.device)
    ws = _lib.workspace(_lib.load().gsr_kmeans_workspace_bytes(N, K), xp.device)
    _lib.call("gsr_kmeans_iter", _ptr(xp), N, _ptr(c), K, iters, _ptr(labels), _ptr(ws), ws.numel(), stream)
    if c is not centroids:
      centroids.copy_(c)
  return labels, centroids


def kmeans(x: torch.Tensor, k: int = 10, iters: int = 100) -> Tuple[torch.Tensor, torch.Tensor]:
  """k-means from k distinct points of ``x`` chosen as the reference does: ``x[torch.randperm(N)[:k]]`` on the CPU
  default generator (the same rows under the same seed).  Returns ``(labels, centroids)``."""
  xp = _cloud(x, "x")
  if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= xp.shape[0]:
    raise ValueError(f"k must be an int in 1..N = {xp.shape[0]}, got {k!r}")
  centroid_idx = torch.randperm(xp.shape[0])[:k]
  centroids = xp[centroid_idx.to(xp.device)]
  return kmeans_iter(xp, centroids, iters)
