"""View clustering, overlap batch sampling and frustum point queries: drop-ins for the reference's
``splat_trainer.visibility.cluster`` (``PointClusters``, ``ViewClustering`` and the sampling functions; the k-means half
lives in neighbours.py), ``splat_trainer.visibility.query_points`` and the two samplers of
``splat_trainer.trainer.view_selection``, with the two reductions on HIP kernels (csrc/visibility.hip).

Frustum test.  A camera is a record of 16 floats: the first three rows of ``image_t_world = expand_proj(K) @
camera_t_world`` (computed in torch as the reference does), then ``w, h, near, far``.  With ``h_r = fmaf(M[r][2], z,
fmaf(M[r][1], y, fmaf(M[r][0], x, M[r][3])))`` and ``d = h_2`` a point is inside when ``h_0 >= 0 and h_0 < w * d and
h_1 >= 0 and h_1 < h * d and d > near and d < min(far, depth_below)``.  The one departure from the reference: it divides
(``xy = h_01 / d`` against ``0`` and ``w, h``); here the division is multiplied out, which is the same test in exact
arithmetic for ``d > near >= 0`` and drops two IEEE divisions per (camera, point) pair.  One pass over the points gives
both counts, as exact int32, with no host sync.

View features.  ``PointClusters.view_features`` is the per-cluster sum of the visibilities above a threshold.  The
reference scatter-adds with float atomics; here the listed values go to a dense scratch and every cluster is summed in a
fixed order, so the row is a function of the *set* of ``(idx, vis)`` pairs: bit-identical between runs and under any
permutation of the list.  ``point_idx`` must hold distinct indices in ``[0, N)`` (what ``Rendering.points.idx`` gives);
duplicates, which the reference would add up, are not supported (``validate=True`` checks, at the cost of one sync).

Device tensors only: CPU tensors, wrong dtypes and shapes raise ValueError; there is no CPU fallback for the native
calls.  The sampling functions and ``ViewClustering`` are plain torch and run wherever their tensors live.

Left out: ``select_weighted`` (dead), ``plot_visibility`` (matplotlib), ``TargetOverlap`` (cannot run as written),
``PointCloud`` (clouds are ``(points, colors)`` pairs or any object with ``.points`` / ``.colors``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from .data_types import CameraParams
from ._args import require
from ._lib import ptr as _ptr
from .neighbours import _cloud, assign_clusters, kmeans


# ---- cameras ------------------------------------------------------------------------------------------------------

def _expand_proj(intrinsics: torch.Tensor) -> torch.Tensor:
  """(V, 4) fx, fy, cx, cy -> (V, 4, 4), the reference's util/transforms.py expand_proj."""
  expanded = torch.zeros((intrinsics.shape[0], 4, 4), dtype=intrinsics.dtype, device=intrinsics.device)
  fx, fy, cx, cy = intrinsics.unbind(-1)
  expanded[:, 0, 0] = fx
  expanded[:, 1, 1] = fy
  expanded[:, 0, 2] = cx
  expanded[:, 1, 2] = cy
  expanded[:, 2, 2] = 1.0
  expanded[:, 3, 3] = 1.0
  return expanded


@dataclass
class CameraBatch:
  """V pinhole cameras as four tensors on one device (the attributes of the reference's ``Cameras`` that the point
  queries read)."""
  camera_t_world: torch.Tensor      # (V, 4, 4) float32
  intrinsics: torch.Tensor          # (V, 4) float32  fx, fy, cx, cy
  image_sizes: torch.Tensor         # (V, 2) int      w, h
  depth_ranges: torch.Tensor        # (V, 2) float32  near, far

  def __post_init__(self):
    V = self.camera_t_world.shape[0] if isinstance(self.camera_t_world, torch.Tensor) and self.camera_t_world.dim() else -1
    for name, shape, dtype in (("camera_t_world", ("V", 4, 4), torch.float32), ("intrinsics", (V, 4), torch.float32),
                               ("image_sizes", (V, 2), None), ("depth_ranges", (V, 2), torch.float32)):
      t = require(name, getattr(self, name), shape=shape, dtype=dtype)
      if dtype is None and (t.dtype.is_floating_point or t.dtype is torch.bool or t.dtype.is_complex):
        raise ValueError(f"image_sizes must be an integer tensor, got {t.dtype}")
      if t.device != self.camera_t_world.device:
        raise ValueError(f"{name} on {t.device} and camera_t_world on {self.camera_t_world.device}")
    if not 1 <= V <= _lib.VISIBILITY_MAX_CAMERAS:
      raise ValueError(f"a CameraBatch holds 1..{_lib.VISIBILITY_MAX_CAMERAS} cameras, got {V}")
    self._records = None

  @staticmethod
  def from_params(cameras: Sequence[CameraParams]) -> "CameraBatch":
    cameras = list(cameras)
    if not cameras:
      raise ValueError("a CameraBatch holds at least one camera (V = 0)")
    device = cameras[0].T_camera_world.device
    return CameraBatch(
        torch.stack([c.T_camera_world.detach().to(torch.float32) for c in cameras]),
        torch.stack([c.projection.detach().to(torch.float32) for c in cameras]),
        torch.tensor([[int(c.image_size[0]), int(c.image_size[1])] for c in cameras], dtype=torch.int64, device=device),
        torch.tensor([[float(c.near_plane), float(c.far_plane)] for c in cameras], dtype=torch.float32, device=device))

  @staticmethod
  def of(obj: Any) -> "CameraBatch":
    """``obj`` as a CameraBatch: one itself, a sequence of CameraParams, or any object with the reference's ``Cameras``
    attributes (``camera_t_world``, ``projection.intrinsics``, ``projection.image_size``, ``projection.depth_range``)."""
    if isinstance(obj, CameraBatch):
      return obj
    if isinstance(obj, CameraParams):
      return CameraBatch.from_params([obj])
    if isinstance(obj, (list, tuple)):
      return CameraBatch.from_params(obj)
    proj = getattr(obj, "projection", None)
    if hasattr(obj, "camera_t_world") and all(hasattr(proj, a) for a in ("intrinsics", "image_size", "depth_range")):
      return CameraBatch(obj.camera_t_world.detach(), proj.intrinsics.detach(), proj.image_size, proj.depth_range)
    raise ValueError(f"cannot read cameras from {type(obj).__name__}")

  @property
  def device(self) -> torch.device:
    return self.camera_t_world.device

  @property
  def batch_size(self) -> Tuple[int]:
    return (self.camera_t_world.shape[0],)

  def __len__(self) -> int:
    return self.camera_t_world.shape[0]

  def image_t_world(self) -> torch.Tensor:
    """(V, 4, 4): ``expand_proj(K) @ camera_t_world`` (query_points.py:74)."""
    return _expand_proj(self.intrinsics) @ self.camera_t_world

  def records(self) -> torch.Tensor:
    """The (V, 16) float32 table the native frustum test reads, cached."""
    if self._records is None:
      rows = self.image_t_world()[:, :3, :].reshape(-1, 12)
      self._records = torch.cat([rows, self.image_sizes.to(torch.float32), self.depth_ranges], dim=1).contiguous()
    return self._records


# ---- frustum point queries (visibility/query_points.py) --------------------------------------------------------------

def _query_args(cameras: Any, points: torch.Tensor) -> Tuple[CameraBatch, torch.Tensor]:
  cams = CameraBatch.of(cameras)
  p = _cloud(points, "points")
  if not cams.camera_t_world.is_cuda:
    raise ValueError("cameras must be on the HIP device (cuda); there is no CPU fallback")
  if cams.device != p.device:
    raise ValueError(f"points on {p.device} and cameras on {cams.device}")
  return cams, p


def _frustum(cameras: Any, points: torch.Tensor, depth_below, want_points: bool, want_cameras: bool):
  cams, p = _query_args(cameras, points)
  below = math.inf if depth_below is None else float(depth_below)
  with _lib.on_device(p.device) as stream:
    rec = cams.records()
    V = rec.shape[0]
    pc = torch.empty(p.shape[0], dtype=torch.int32, device=p.device) if want_points else None
    cc = torch.empty(V, dtype=torch.int32, device=p.device) if want_cameras else None
    _lib.call("gsr_frustum_counts", _ptr(p), p.shape[0], _ptr(rec), V, below, _ptr(pc), _ptr(cc), stream)
  return pc, cc


def frustum_counts(cameras: Any, points: torch.Tensor, depth_below: Optional[float] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
  """``(point_counts (N,) int32, camera_counts (V,) int32)`` from one pass: the cameras that see each point and the
  points each camera sees.  ``depth_below`` additionally requires ``d < depth_below``."""
  return _frustum(cameras, points, depth_below, True, True)


def point_visibility(cameras: Any, points: torch.Tensor) -> torch.Tensor:
  """The number of cameras that see each point, (N,) int32."""
  return _frustum(cameras, points, None, True, False)[0]


def camera_counts(cameras: Any, points: torch.Tensor) -> torch.Tensor:
  """The number of points each camera sees, (V,) int32."""
  return _frustum(cameras, points, None, False, True)[1]


def _cloud_parts(pcd: Any) -> Tuple[torch.Tensor, torch.Tensor]:
  if isinstance(pcd, (tuple, list)) and len(pcd) == 2:
    return pcd[0], pcd[1]
  if hasattr(pcd, "points") and hasattr(pcd, "colors"):
    return pcd.points, pcd.colors
  raise ValueError(f"a cloud is a (points, colors) pair or has .points / .colors, got {type(pcd).__name__}")


def crop_cloud(cameras: Any, pcd: Any) -> Any:
  """The part of the cloud seen by at least one camera: a ``(points, colors)`` pair for a pair, ``pcd[mask]`` otherwise."""
  points, colors = _cloud_parts(pcd)
  mask = point_visibility(cameras, points) > 0
  if isinstance(pcd, (tuple, list)):
    return points[mask], colors[mask]
  return pcd[mask]


def inverse_ndc_depth(ndc_depth: torch.Tensor, near: float, far: float) -> torch.Tensor:
  # ndc from 0 to 1 (instead of -1 to 1)
  return (near * far - ndc_depth * near) / (far - ndc_depth * (far - near))


def random_ndc(n: int, depth_range: Tuple[float, float], device=None) -> torch.Tensor:
  if device is None:
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
  depths = torch.rand((n, 1), device=device)
  return inverse_ndc_depth(depths, *depth_range)


def random_points(cameras: Any, count: int, weighting: Optional[torch.Tensor] = None) -> torch.Tensor:
  """``count`` random points, each inside the frustum of a random camera (chosen uniformly, or by ``weighting``), at a
  depth uniform in NDC over the FIRST camera's depth range, as the reference draws them (same RNG calls, same order)."""
  cams = CameraBatch.of(cameras)
  near, far = cams.depth_ranges[0].tolist()
  world_t_image = torch.inverse(cams.image_t_world())
  device = world_t_image.device
  if weighting is None:
    camera_idx = torch.randint(0, world_t_image.shape[0], (count,), device=device)
  else:
    camera_idx = torch.multinomial(F.normalize(weighting, p=1, dim=0), count, replacement=True)
  norm_points = torch.rand(count, 2, device=device)
  image_points = norm_points * cams.image_sizes[camera_idx]
  depths = random_ndc(count, (near, far), device=device)
  ones = torch.ones((count, 1), device=device)
  homog = torch.cat([image_points * depths, depths, ones], dim=1)
  points_unproj = torch.bmm(world_t_image[camera_idx], homog.unsqueeze(2)).squeeze(-1)
  return points_unproj[..., :3] / points_unproj[..., 3:4]


def balanced_points(cameras: Any, count: int, min_overlap: int = 4, existing_points: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
  """Random points each seen by at least ``min_overlap`` cameras, drawn towards the cameras that see the fewest so far.
  Returns ``(points (count, 3), camera_counts (V,) int32)``.  Every rejection round is one native pass for the
  per-point counts and one for the per-camera counts of the survivors."""
  cams = CameraBatch.of(cameras)
  if existing_points is not None:
    valid_points = existing_points
    cam_counts = camera_counts(cams, valid_points)
  else:
    valid_points = torch.empty((0, 3), device=cams.device)
    cam_counts = torch.zeros(len(cams), dtype=torch.int32, device=cams.device)
  while valid_points.shape[0] < count:
    points = random_points(cams, count // 8, weighting=1 / (cam_counts + 1))
    points = points[point_visibility(cams, points) >= min_overlap]
    if points.shape[0] > 0:
      cam_counts += camera_counts(cams, points)
    valid_points = torch.cat([valid_points, points])
  return valid_points[:count], cam_counts


def random_cloud(cameras: Any, count: int) -> Tuple[torch.Tensor, torch.Tensor]:
  points = random_points(cameras, count)
  colors = torch.rand(count, 3, device=points.device)
  return points, colors


def balanced_cloud(cameras: Any, count: int, min_overlap: int = 4, existing_points: Any = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
  if existing_points is not None:
    old_points, old_colors = _cloud_parts(existing_points)
    points, _ = balanced_points(cameras, count, min_overlap, old_points)
    colors = old_colors[:count]
    if colors.shape[0] < count:
      colors = torch.cat([colors, torch.rand(count - colors.shape[0], 3, device=colors.device)])
  else:
    points, _ = balanced_points(cameras, count, min_overlap)
    colors = torch.rand(count, 3, device=points.device)
  return points, colors


def _first_camera_quantile(cams: CameraBatch, points: torch.Tensor, quantile: float) -> torch.Tensor:
  """The quantile of the depths of the points the first camera sees, in the reference's torch form (one camera)."""
  m = cams.image_t_world()[0]
  homog = torch.cat([points, torch.ones_like(points[:, :1])], dim=1)
  proj = (m.reshape(1, 4, 4) @ homog.reshape(-1, 4, 1))[..., 0]
  depth = proj[:, 2]
  xy = proj[:, :2] / depth.unsqueeze(-1)
  w, h = cams.image_sizes[0].tolist()
  near, far = cams.depth_ranges[0].tolist()
  mask = ((xy[:, 0] >= 0) & (xy[:, 0] < w) & (xy[:, 1] >= 0) & (xy[:, 1] < h) & (depth > near) & (depth < far))
  return torch.quantile(depth[mask], quantile)


def foreground_visibility(cameras: Any, points: torch.Tensor, far_threshold: Optional[float] = None,
                          quantile: float = 1.0) -> torch.Tensor:
  """The number of cameras that see each point nearer than ``far_threshold``, (N,) int32.  With ``far_threshold=None``
  the threshold is the ``quantile`` of the depths of the points the FIRST camera sees and then holds for every camera
  (the reference assigns it once, in its first iteration); that quantile is one torch call on the first camera (and one
  sync), everything else is the native pass with ``depth_below``."""
  cams, p = _query_args(cameras, points)
  if far_threshold is None:
    far_threshold = float(_first_camera_quantile(cams, p, quantile))
  return _frustum(cams, p, far_threshold, True, False)[0]


def foreground_points(cameras: Any, points: torch.Tensor, far_threshold: Optional[float] = None, quantile: float = 0.25,
                      min_overlap: float = 0.01) -> torch.Tensor:
  near_counts = foreground_visibility(cameras, points, far_threshold, quantile=quantile)
  num_views = len(CameraBatch.of(cameras))
  return near_counts > (min_overlap * num_views)


# ---- point clusters and view features (visibility/cluster.py) --------------------------------------------------------

class PointClusters:
  """k-means clusters of the scene's points, and the per-cluster visibility row of a rendering."""

  def __init__(self, point_labels: torch.Tensor, centroids: torch.Tensor):
    self.view_visibility = {}
    self.centroids = centroids
    self.point_labels = point_labels
    self._order = None          # (sorted labels, sorted point indices, [K, 2] ranges, dense scratch, slot scratch)

  @staticmethod
  def cluster(points: torch.Tensor, num_clusters: int) -> "PointClusters":
    point_labels, centroids = kmeans(points, min(num_clusters, points.shape[0]))
    return PointClusters(point_labels, centroids)

  def assign_clusters(self, points: torch.Tensor) -> torch.Tensor:
    return assign_clusters(points, self.centroids)

  @property
  def num_clusters(self) -> int:
    return self.centroids.shape[0]

  def _cluster_order(self):
    """Built once (the labels do not change between the calls of one evaluation): the points in stable label order and
    every cluster's [start, end) in it, plus the two scratch arrays every call reuses."""
    if self._order is not None:
      return self._order
    labels = self.point_labels
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype is not torch.int64:
      raise ValueError("point_labels must be an (N,) int64 tensor")
    if not labels.is_cuda:
      raise ValueError("point_labels must be on the HIP device (cuda); there is no CPU fallback")
    N, K = labels.shape[0], self.num_clusters
    if not 1 <= N <= _lib.NEIGHBOURS_MAX_N or K < 1:
      raise ValueError(f"PointClusters needs 1..{_lib.NEIGHBOURS_MAX_N} points and at least one cluster, got {N}, {K}")
    dev = labels.device
    with _lib.on_device(dev) as stream:
      if bool(((labels < 0) | (labels >= K)).any()):
        raise ValueError(f"point_labels must lie in [0, {K})")
      keys_a = labels.to(torch.int32)
      vals_a, keys_b, vals_b = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
      ws = _lib.workspace(_lib.load().gsr_sort_workspace_bytes(N), dev)
      where = _lib.call("gsr_sort_pairs_u32", _ptr(keys_a), _ptr(vals_a), _ptr(keys_b), _ptr(vals_b), N, 1, 0,
                        max(1, (K - 1).bit_length()), _ptr(ws), ws.numel(), None, stream)
      skeys, svals = (keys_b, vals_b) if where else (keys_a, vals_a)
      ranges = torch.zeros((K, 2), dtype=torch.int32, device=dev)
      _lib.call("gsr_tile_ranges", _ptr(skeys), N, K, _ptr(ranges), None, stream)
      dense = torch.empty(N, dtype=torch.float32, device=dev)
      slots = torch.empty(N, dtype=torch.float32, device=dev)
    self._order = (skeys, svals, ranges, dense, slots)
    return self._order

  def view_features(self, point_idx: torch.Tensor, point_vis: torch.Tensor, vis_threshold: float = 0.01,
                    point_visible: Optional[torch.Tensor] = None, validate: bool = False) -> torch.Tensor:
    """(K,) float32: per cluster the sum of ``point_vis[j]`` over the listed points with ``point_vis[j] >
    vis_threshold``.  ``point_idx`` (M,) int64 holds distinct indices in [0, N).  ``point_visible`` (N,) int32, if given,
    is incremented at every listed index (the evaluation loop's ``point_visible[points.idx] += 1``) by the same call.
    ``validate=True`` checks range and distinctness (one sync) and raises ValueError."""
    labels = self.point_labels
    for t, name, dtype in ((point_idx, "point_idx", torch.int64), (point_vis, "point_vis", torch.float32)):
      require(name, t, shape=("M",), dtype=dtype, what="a view's features", device_error=ValueError)
      if isinstance(labels, torch.Tensor) and t.device != labels.device:
        raise ValueError(f"{name} on {t.device} and point_labels on {labels.device}")
    if point_idx.shape != point_vis.shape:
      raise ValueError(f"point_idx {tuple(point_idx.shape)} and point_vis {tuple(point_vis.shape)} differ in length")
    skeys, svals, ranges, dense, slots = self._cluster_order()
    N, K, M = labels.shape[0], self.num_clusters, point_idx.shape[0]
    if M > _lib.NEIGHBOURS_MAX_N:
      raise ValueError(f"at most {_lib.NEIGHBOURS_MAX_N} listed points, got {M}")
    if point_visible is not None:
      if (not isinstance(point_visible, torch.Tensor) or point_visible.shape != (N,) or
          point_visible.dtype is not torch.int32 or point_visible.device != labels.device or
          not point_visible.is_contiguous()):
        raise ValueError(f"point_visible must be a contiguous ({N},) int32 tensor on {labels.device}")
    idx = point_idx.contiguous()
    vis = point_vis.detach().contiguous()
    with _lib.on_device(labels.device) as stream:
      if validate and M > 0:
        ordered = idx.sort().values
        bad = (ordered[0] < 0) | (ordered[-1] >= N) | (ordered[1:] == ordered[:-1]).any()
        if bool(bad):
          raise ValueError(f"point_idx must hold distinct indices in [0, {N})")
      out = torch.empty(K, dtype=torch.float32, device=labels.device)
      _lib.call("gsr_view_features", _ptr(idx), _ptr(vis), M, float(vis_threshold), _ptr(skeys), _ptr(svals), _ptr(ranges),
                N, K, _ptr(dense), _ptr(slots), _ptr(out), _ptr(point_visible), stream)
    return out

  def rendering_features(self, rendering: Any, vis_threshold: float = 0.01,
                         point_visible: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``view_features`` of a rendering made with ``compute_visibility``.  The listed indices and visibilities go straight
    through: the threshold subsumes the reference's ``visibility > 0`` filter, so no mask and no sync are needed."""
    return self.view_features(rendering.points.idx, rendering.points.visibility, vis_threshold, point_visible)

  def state_dict(self):
    return {"point_labels": self.point_labels, "centroids": self.centroids}

  @classmethod
  def from_state_dict(cls, state_dict):
    return cls(state_dict["point_labels"], state_dict["centroids"])


class ViewClustering:
  """The (V, K) table of every view's cluster visibilities and the view-to-view similarity drawn from it."""

  def __init__(self, point_clusters: PointClusters, cluster_visibility: torch.Tensor, metric: str = "cosine"):
    if metric not in ("cosine", "euclidean"):
      raise ValueError(f"Unknown metric: {metric}, expected 'cosine' or 'euclidean'")
    self.point_clusters = point_clusters
    self.cluster_visibility = cluster_visibility
    self.metric = metric
    self._normalized = None
    self._similarity = None

  @property
  def normalized_visibility(self) -> torch.Tensor:
    if self._normalized is None:
      by_cluster = F.normalize(self.cluster_visibility, dim=0, p=2)
      self._normalized = F.normalize(by_cluster, dim=1, p=2)        # then by view
    return self._normalized

  @property
  def view_similarity(self) -> torch.Tensor:
    if self._similarity is None:
      self._similarity = self.overlaps_with(self.normalized_visibility)
    return self._similarity

  def overlaps_with(self, visibility_vec: torch.Tensor) -> torch.Tensor:
    if self.metric == "cosine":
      return visibility_vec @ self.normalized_visibility.T
    return torch.cdist(visibility_vec, self.normalized_visibility, p=2)

  def select_batch(self, weighting: torch.Tensor, min_batch_size: int, overlap_threshold: float = 0.5) -> torch.Tensor:
    return select_batch(self.view_similarity, weighting, min_size=min_batch_size, threshold=overlap_threshold)

  def sample_batch(self, weighting: torch.Tensor, batch_size: int, temperature: float = 1.0) -> torch.Tensor:
    return sample_batch(self.view_similarity, weighting, batch_size, temperature)

  def visible_points(self, batch_indices: torch.Tensor) -> torch.Tensor:
    """The indices of the points whose cluster any view of the batch sees: ``nonzero(cluster_visibility[labels] > 0)``.
    (The reference indexes that per-point mask by the labels a second time, which only means something by accident.)"""
    cluster_visibility = self.cluster_visibility[batch_indices].sum(dim=0)
    return torch.nonzero(cluster_visibility[self.point_clusters.point_labels] > 0).squeeze(1)

  def state_dict(self):
    return {"point_clusters": self.point_clusters.state_dict(), "cluster_visibility": self.cluster_visibility,
            "metric": self.metric}

  @classmethod
  def from_state_dict(cls, state_dict):
    return cls(PointClusters.from_state_dict(state_dict["point_clusters"]), state_dict["cluster_visibility"],
               state_dict["metric"])


def sample_with_temperature(p: torch.Tensor, temperature: float = 1.0, n: int = 1,
                            weighting: Optional[torch.Tensor] = None) -> torch.Tensor:
  """``n`` indices drawn without replacement with probability proportional to ``p ** (1 / temperature)`` (times
  ``weighting``); temperature 0 is top-k."""
  if temperature == 0:
    if weighting is not None:
      p = p * weighting
    return torch.topk(p, k=n, dim=0).indices
  p = F.softmax(p.log() / temperature, dim=0)
  if weighting is not None:
    p = F.normalize(p * weighting, dim=0, p=1)
  return torch.multinomial(p, n, replacement=False)


def select_batch(view_similarity: torch.Tensor, weighting: torch.Tensor, threshold: float = 0.4, min_size: int = 25
                 ) -> torch.Tensor:
  """A master view drawn by ``weighting`` and the views whose similarity to it exceeds ``threshold`` (at least
  ``min_size``), in descending similarity, the master first."""
  index = torch.multinomial(weighting, 1, replacement=False)
  group_mask = view_similarity[index] > threshold
  n = max(group_mask.sum().item(), min_size)
  return torch.topk(view_similarity[index], k=n, sorted=True).indices.squeeze(0)


def sample_batch(view_overlaps: torch.Tensor, weighting: torch.Tensor, batch_size: int, temperature: float = 1.0
                 ) -> torch.Tensor:
  """A first view drawn by ``weighting``, then ``batch_size - 1`` others by their overlap with it.  The row of the first
  view is copied before its own entry is zeroed (the reference zeroes it inside ``view_overlaps``, which here is the
  cached similarity matrix); the draws are the same."""
  index = torch.multinomial(weighting, 1, replacement=False)
  if batch_size > 1:
    probs = view_overlaps[index.squeeze(0)].clone()
    probs[index.squeeze(0)] = 0
    other_index = sample_with_temperature(probs, temperature=temperature, n=batch_size - 1, weighting=weighting)
    return torch.cat([index, other_index], dim=0)
  return index


def sample_batch_grouped(batch_size: int, view_overlaps: torch.Tensor, weighting: torch.Tensor, temperature: float = 1.0
                         ) -> torch.Tensor:
  """A first view drawn by ``weighting``, then one view at a time by its summed overlap with those already chosen."""
  index = torch.multinomial(weighting, 1, replacement=False)
  overlaps = view_overlaps[index.squeeze(0)].clone()
  selected = index
  for _ in range(batch_size - 1):
    overlaps[selected] = 0
    other_index = sample_with_temperature(overlaps, temperature=temperature, n=1)
    overlaps += view_overlaps[other_index.squeeze(0)]
    selected = torch.cat([selected, other_index], dim=0)
  return selected


def sinkhorn(matrix: torch.Tensor, num_iter: int, epsilon: float = 1e-8) -> torch.Tensor:
  """Sinkhorn-Knopp: symmetrise, normalise rows, normalise columns, ``num_iter`` times."""
  for _ in range(num_iter):
    matrix = (matrix + matrix.T) / 2
    matrix = matrix / (matrix.sum(dim=1, keepdim=True) + epsilon)
    matrix = matrix / (matrix.sum(dim=0, keepdim=True) + epsilon)
  return matrix


# ---- view selection (trainer/view_selection.py) ------------------------------------------------------------------------

@dataclass(frozen=True)
class BatchOverlapSamplerConfig:
  batch_size: int
  overlap_temperature: float

  def create(self, train_idx: torch.Tensor) -> "BatchOverlapSampler":
    return BatchOverlapSampler(self, train_idx)

  def from_state_dict(self, state_dict: dict, train_idx: torch.Tensor) -> "BatchOverlapSampler":
    return BatchOverlapSampler(self, train_idx, state_dict["view_counts"])


class BatchOverlapSampler:
  """Selects the batch of images of one gradient step by sampling views of similar cluster visibility; every view is
  used once before any is used again, and views used less often are preferred as the first of a batch."""

  def __init__(self, config: BatchOverlapSamplerConfig, train_idx: torch.Tensor, view_counts: Optional[torch.Tensor] = None):
    self.train_idx = train_idx
    self.config = config
    self.used_mask = torch.zeros_like(train_idx, dtype=torch.bool)
    self.view_counts = view_counts if view_counts is not None else torch.zeros(len(train_idx), device=train_idx.device)

  def state_dict(self) -> dict:
    return dict(view_counts=self.view_counts)

  def select_images(self, view_clustering: ViewClustering, progress: Any = None) -> torch.Tensor:
    if self.used_mask.all():
      self.used_mask.fill_(False)
    weighting = F.normalize(1 / (self.view_counts + 1), p=1, dim=0)
    weighting[self.used_mask] = 0
    batch_idx = view_clustering.sample_batch(weighting, self.config.batch_size, self.config.overlap_temperature)
    self.used_mask[batch_idx] = True
    self.view_counts[batch_idx] += 1
    return batch_idx


@dataclass(frozen=True)
class RandomSamplerConfig:
  batch_size: int

  def create(self, train_idx: torch.Tensor, next: Optional[torch.Tensor] = None) -> "RandomSampler":
    return RandomSampler(self, train_idx, next)

  def from_state_dict(self, state_dict: dict, train_idx: torch.Tensor) -> "RandomSampler":
    return self.create(train_idx, state_dict["next"])


class RandomSampler:
  """Walks a random permutation of the training views, reshuffling when fewer than a batch remain."""

  def __init__(self, config: RandomSamplerConfig, train_idx: torch.Tensor, next: Optional[torch.Tensor] = None):
    self.train_idx = train_idx
    if next is None:
      next = self.train_idx[torch.randperm(len(train_idx))]
    self.next = next
    self.config = config

  def state_dict(self) -> dict:
    return dict(next=self.next)

  def select_images(self, _: Any = None, progress: Any = None) -> torch.Tensor:
    batch_size = self.config.batch_size
    if self.next.shape[0] < batch_size:
      perm = torch.randperm(len(self.train_idx))
      self.next = self.train_idx[perm]
    indices = self.next[:batch_size]
    self.next = self.next[batch_size:]
    return indices


@dataclass(frozen=True)
class TargetOverlapConfig:
  batch_size: int = 1
  overlap_temperature: float = 0.5
  history_size: int = 2
  target_overlap: float = 0.5

  def create(self, train_idx: torch.Tensor) -> "TargetOverlap":
    return TargetOverlap(self, train_idx)

  def from_state_dict(self, state_dict: dict, train_idx: torch.Tensor) -> "TargetOverlap":
    return TargetOverlap(self, train_idx, state_dict["history_idx"], state_dict["available_mask"])


class TargetOverlap:
  """Selects views whose overlap with a short history of the last selected views is near ``target_overlap``; every view
  is used once before any is used again.  ``history_idx`` and ``available_mask`` index ``train_idx`` and with it the rows
  of the view clustering, which the trainer builds over the training views in that order; ``select_images`` returns
  entries of ``train_idx``.

  One deviation from the reference: it updates the history with ``history_idx[batch_idx:]``, a slice by a tensor, which
  only works for a batch of one; here the new history is ``cat([batch, history])[:history_size]``, for any batch size."""

  def __init__(self, config: TargetOverlapConfig, train_idx: torch.Tensor, history_idx: Optional[torch.Tensor] = None,
               available_mask: Optional[torch.Tensor] = None):
    self.train_idx = train_idx
    self.config = config
    if available_mask is None:
      available_mask = torch.ones(len(train_idx), device=train_idx.device, dtype=torch.bool)
    if history_idx is None:
      history_idx = torch.randperm(len(train_idx))[:config.history_size].to(train_idx.device)
    self.available_mask = available_mask
    self.history_idx = history_idx

  def state_dict(self) -> dict:
    return dict(history_idx=self.history_idx, available_mask=self.available_mask)

  def select_images(self, view_clustering: ViewClustering, progress: Any = None) -> torch.Tensor:
    batch_size = self.config.batch_size
    if int(self.available_mask.sum()) < batch_size:
      self.available_mask.fill_(True)
    vis = F.normalize(view_clustering.normalized_visibility[self.history_idx].sum(0), dim=0, p=2)
    overlaps = view_clustering.overlaps_with(vis)
    score = 1 - (self.config.target_overlap - overlaps[self.available_mask]).pow(2)
    available = torch.nonzero(self.available_mask).squeeze(1)
    chosen = available[sample_with_temperature(score + 1e-6, temperature=self.config.overlap_temperature, n=batch_size)]
    self.available_mask[chosen] = False
    self.history_idx = torch.cat([chosen, self.history_idx])[:self.config.history_size]
    return self.train_idx[chosen]
