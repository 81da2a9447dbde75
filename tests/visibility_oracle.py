"""Oracles for splat_trainer_amd.visibility.  The reference's visibility/ modules import pykeops, taichi_splatting and
tensordict, so nothing of them is imported: the frustum test and the view-feature sums are restated in fp64 numpy, and the
few torch lines of the reference that the sampling and query functions consist of are restated with their file and line
(splat_trainer/visibility/cluster.py, visibility/query_points.py).  Also the wrappers of the host shim and the ring
scene the checks use."""

import numpy as np
import torch
import torch.nn.functional as F

TOL = 8.0 * 2.0 ** -24      # twice the modelled rounding of one comparison: four roundings per h_r and one for the product


# ---- scene -----------------------------------------------------------------------------------------------------------

def ring_cameras(V, radius=6.0, seed=0, size=(640, 480), focal=(400.0, 700.0), near=0.1, far=100.0, height=0.0):
  """V cameras on a ring of ``radius`` about the y axis looking at the origin (+z forward, y down), fx = fy uniform in
  ``focal``, principal point at the image centre.  Returns float32 / int64 numpy arrays (camera_t_world (V, 4, 4),
  intrinsics (V, 4), image_sizes (V, 2), depth_ranges (V, 2))."""
  rng = np.random.default_rng(seed)
  ctw = np.zeros((V, 4, 4))
  for i in range(V):
    a = 2 * np.pi * i / V
    c = np.array([radius * np.cos(a), height, radius * np.sin(a)])
    z = -c / np.linalg.norm(c)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    ctw[i, :3, :3] = R
    ctw[i, :3, 3] = -R @ c
    ctw[i, 3, 3] = 1
  f = rng.uniform(focal[0], focal[1], V)
  intr = np.stack([f, f, np.full(V, size[0] / 2), np.full(V, size[1] / 2)], 1)
  sizes = np.tile(np.array(size, dtype=np.int64), (V, 1))
  ranges = np.tile(np.array([near, far]), (V, 1))
  return ctw.astype(np.float32), intr.astype(np.float32), sizes, ranges.astype(np.float32)


def ring_points(n, seed=0, sigma=(3.0, 1.5, 3.0)):
  return (np.random.default_rng(seed).standard_normal((n, 3)) * np.array(sigma)).astype(np.float32)


def camera_batch(sta_visibility, cams, device="cpu"):
  ctw, intr, sizes, ranges = cams
  return sta_visibility.CameraBatch(torch.from_numpy(ctw).to(device), torch.from_numpy(intr).to(device),
                                    torch.from_numpy(sizes).to(device), torch.from_numpy(ranges).to(device))


# ---- fp64 frustum test -------------------------------------------------------------------------------------------------

def frustum_fp64(points, records, depth_below=np.inf):
  """The inside test of every (camera, point) pair in fp64 on the float32 records and points, and which pairs are *near a
  boundary*: one of the six comparisons has its sides within TOL * s of each other, s the sum of the magnitudes of the
  terms of the sums compared.  Returns ``(inside (V, N) bool, near (V, N) bool)``."""
  p = points.astype(np.float64)
  V, N = records.shape[0], p.shape[0]
  inside = np.zeros((V, N), dtype=bool)
  near_b = np.zeros((V, N), dtype=bool)
  for c in range(V):
    r = records[c].astype(np.float64)
    M = r[:12].reshape(3, 4)
    w, h, near, far = r[12:]
    terms = M[:, None, :3] * p[None, :, :]                        # (3, N, 3)
    hr = terms.sum(-1) + M[:, 3:4]                                # (3, N)
    sr = np.abs(terms).sum(-1) + np.abs(M[:, 3:4])
    h0, h1, d = hr
    s0, s1, s2 = sr
    lim = min(far, depth_below)
    with np.errstate(invalid="ignore"):
      inside[c] = (h0 >= 0) & (h0 < w * d) & (h1 >= 0) & (h1 < h * d) & (d > near) & (d < lim)
      nb = (np.abs(h0) <= TOL * s0) | (np.abs(h0 - w * d) <= TOL * (s0 + w * s2))
      nb |= (np.abs(h1) <= TOL * s1) | (np.abs(h1 - h * d) <= TOL * (s1 + h * s2))
      nb |= np.abs(d - near) <= TOL * (s2 + abs(near))
      if np.isfinite(lim):
        nb |= np.abs(d - lim) <= TOL * (s2 + abs(lim))
    near_b[c] = nb
  return inside, near_b


# ---- fp64 view features ------------------------------------------------------------------------------------------------

def view_features_fp64(labels, K, idx, vis, threshold=0.01):
  """(sum (K,) float64, member count (K,)): per cluster the sum of vis[j] > float32(threshold) over the listed points
  (cluster.py:36-47 with distinct indices)."""
  keep = vis > np.float32(threshold)
  s = np.bincount(labels[idx[keep]], weights=vis[keep].astype(np.float64), minlength=K)
  return s, np.bincount(labels, minlength=K)


# ---- host shim -------------------------------------------------------------------------------------------------------

def shim_frustum(lib, points, records, depth_below=np.inf, want_points=True, want_cameras=True):
  points = np.ascontiguousarray(points, dtype=np.float32)
  records = np.ascontiguousarray(records, dtype=np.float32)
  pc = np.empty(points.shape[0], dtype=np.int32) if want_points else None
  cc = np.empty(records.shape[0], dtype=np.int32) if want_cameras else None
  lib.hm_frustum_counts(points, points.shape[0], records, records.shape[0], float(depth_below), pc, cc)
  return pc, cc


def shim_view_features(lib, labels, K, idx, vis, threshold=0.01, point_visible=None):
  labels = np.ascontiguousarray(labels, dtype=np.int64)
  idx = np.ascontiguousarray(idx, dtype=np.int64)
  vis = np.ascontiguousarray(vis, dtype=np.float32)
  out = np.empty(K, dtype=np.float32)
  rc = lib.hm_view_features(labels, labels.shape[0], K, idx, vis, idx.shape[0], float(threshold), out, point_visible)
  assert rc == 0, rc
  return out


# ---- the reference's torch lines ---------------------------------------------------------------------------------------

def projections_torch(image_t_world, image_sizes, depth_ranges, points):
  """query_points.py:73-84 with Projected.visible_mask (:62-70): per camera ``(depth, mask)``."""
  homog = torch.cat([points, torch.ones_like(points[:, :1])], dim=-1)
  for i in range(image_t_world.shape[0]):
    proj = (image_t_world[i].reshape(-1, 4, 4) @ homog.reshape(-1, 4, 1))[..., 0].reshape(-1, 4)
    depth = proj[..., 2]
    xy = proj[..., :2] / depth.unsqueeze(-1)
    w, h = image_sizes[i]
    near, far = depth_ranges[i]
    yield depth, ((xy[..., 0] >= 0) & (xy[..., 0] < w) & (xy[..., 1] >= 0) & (xy[..., 1] < h)
                  & (depth > near) & (depth < far))


def point_visibility_torch(image_t_world, image_sizes, depth_ranges, points):
  """query_points.py:89-93."""
  vis_counts = torch.zeros(points.shape[0], dtype=torch.int32, device=points.device)
  for _, mask in projections_torch(image_t_world, image_sizes, depth_ranges, points):
    vis_counts[mask] += 1
  return vis_counts


def camera_counts_torch(image_t_world, image_sizes, depth_ranges, points):
  """query_points.py:97-102."""
  cam_counts = torch.zeros(image_t_world.shape[0], dtype=torch.int32, device=points.device)
  for i, (_, mask) in enumerate(projections_torch(image_t_world, image_sizes, depth_ranges, points)):
    cam_counts[i] = mask.sum()
  return cam_counts


def foreground_visibility_torch(image_t_world, image_sizes, depth_ranges, points, far_threshold=None, quantile=1.0):
  """query_points.py:190-203: the threshold, when None, is assigned once -- from the first camera."""
  vis_counts = torch.zeros(points.shape[0], dtype=torch.int32, device=points.device)
  for depth, mask in projections_torch(image_t_world, image_sizes, depth_ranges, points):
    if far_threshold is None:
      far_threshold = torch.quantile(depth[mask], quantile)
    vis_counts[mask & (depth < far_threshold)] += 1
  return vis_counts, far_threshold


def view_features_torch(point_labels, K, point_idx, point_vis, vis_threshold=0.01):
  """cluster.py:36-47."""
  vector = torch.zeros(K, device=point_labels.device)
  mask = point_vis > vis_threshold
  vector.scatter_add_(0, point_labels[point_idx[mask]], point_vis[mask])
  return vector


def normalized_visibility_ref(cluster_visibility):
  """cluster.py:76-81."""
  return F.normalize(F.normalize(cluster_visibility, dim=0, p=2), dim=1, p=2)


def overlaps_ref(visibility_vec, normalized, metric):
  """cluster.py:89-92."""
  return visibility_vec @ normalized.T if metric == "cosine" else torch.cdist(visibility_vec, normalized, p=2)


def sample_with_temperature_ref(p, temperature=1.0, n=1, weighting=None):
  """cluster.py:191-200."""
  if temperature == 0:
    if weighting is not None:
      p = p * weighting
    return torch.topk(p, k=n, dim=0).indices
  p = F.softmax(p.log() / temperature, dim=0)
  if weighting is not None:
    p = F.normalize(p * weighting, dim=0, p=1)
  return torch.multinomial(p, n, replacement=False)


def select_batch_ref(view_similarity, weighting, threshold=0.4, min_size=25):
  """cluster.py:219-223."""
  index = torch.multinomial(weighting, 1, replacement=False)
  group_mask = view_similarity[index] > threshold
  n = max(group_mask.sum().item(), min_size)
  return torch.topk(view_similarity[index], k=n, sorted=True).indices.squeeze(0)


def sample_batch_ref(view_overlaps, weighting, batch_size, temperature=1.0):
  """cluster.py:232-241 (on a copy of the matrix: the reference zeroes the first view's own entry in place)."""
  view_overlaps = view_overlaps.clone()
  index = torch.multinomial(weighting, 1, replacement=False)
  if batch_size > 1:
    probs = view_overlaps[index.squeeze(0)]
    probs[index.squeeze(0)] = 0
    other = sample_with_temperature_ref(probs, temperature=temperature, n=batch_size - 1, weighting=weighting)
    return torch.cat([index, other], dim=0)
  return index


def sample_batch_grouped_ref(batch_size, view_overlaps, weighting, temperature=1.0):
  """cluster.py:270-283."""
  index = torch.multinomial(weighting, 1, replacement=False)
  overlaps = view_overlaps[index.squeeze(0)].clone()
  selected = index
  for _ in range(batch_size - 1):
    overlaps[selected] = 0
    other = sample_with_temperature_ref(overlaps, temperature=temperature, n=1)
    overlaps += view_overlaps[other.squeeze(0)]
    selected = torch.cat([selected, other], dim=0)
  return selected
