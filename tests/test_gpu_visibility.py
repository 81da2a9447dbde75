"""splat_trainer_amd.visibility on the MI355X: the frustum counts and the view features bit-identical to the host shim
(the same header), deterministic and independent of the list order; the whole chain renderer -> PointClusters ->
ViewClustering -> sample_batch on a synthetic scene against the oracle; balanced_points / crop_cloud / foreground_points
against the fp64 test and the reference's torch lines; every ValueError."""
import dataclasses

import numpy as np
import pytest
import torch

import hostmath
import splat_trainer_amd as sta
from splat_trainer_amd import synthetic
from splat_trainer_amd import visibility as vis
from visibility_oracle import (camera_batch, foreground_visibility_torch, frustum_fp64, point_visibility_torch,
                               ring_cameras, ring_points, sample_batch_ref, shim_frustum, shim_view_features,
                               view_features_fp64)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim(built_libs):
  return hostmath.load(built_libs)


def _np(t):
  return t.cpu().numpy()


# ---- 1. frustum counts -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,V", [(1, 1), (1000, 3), (65537, 64), (1_000_003, 257)])
def test_frustum_counts_bit_identical_to_host(shim, N, V):
  cams = camera_batch(vis, ring_cameras(V, seed=V), "cuda")
  pts = ring_points(N, seed=N % 97)
  p = torch.from_numpy(pts).cuda()
  pc, cc = vis.frustum_counts(cams, p)
  only_p, only_c = vis.point_visibility(cams, p), vis.camera_counts(cams, p)
  torch.cuda.synchronize()
  assert pc.shape == (N,) and pc.dtype == torch.int32 and cc.shape == (V,) and cc.dtype == torch.int32
  assert torch.equal(only_p, pc) and torch.equal(only_c, cc)
  rec = _np(cams.records())
  if N <= 4096:
    hp, hc = shim_frustum(shim, pts, rec)
    assert np.array_equal(_np(pc), hp)
  else:
    _, hc = shim_frustum(shim, pts, rec, want_points=False)
    for a, b in ((0, 1536), (N - 1536, N)):
      hp, _ = shim_frustum(shim, pts[a:b], rec, want_cameras=False)
      assert np.array_equal(_np(pc[a:b]), hp), (a, b)
  assert np.array_equal(_np(cc), hc)
  assert int(cc.sum()) == int(pc.to(torch.int64).sum())
  if V > 1:
    assert 0 < int(cc.sum()) < N * V


def test_frustum_depth_below_bit_identical_to_host(shim):
  cams = camera_batch(vis, ring_cameras(7, seed=1), "cuda")
  pts = ring_points(5000, seed=5)
  pc, cc = vis.frustum_counts(cams, torch.from_numpy(pts).cuda(), depth_below=6.0)
  hp, hc = shim_frustum(shim, pts, _np(cams.records()), depth_below=6.0)
  assert np.array_equal(_np(pc), hp) and np.array_equal(_np(cc), hc)
  full, _ = vis.frustum_counts(cams, torch.from_numpy(pts).cuda())
  assert (pc <= full).all() and (pc < full).any()


# ---- 2. view features --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,M", [(1, 1, 1), (1000, 7, 400), (200_003, 1024, 150_000), (70_000, 3, 70_000), (5000, 16, 0)])
def test_view_features_bit_identical_to_host_and_deterministic(shim, N, K, M):
  g = torch.Generator().manual_seed(N + K)
  labels = torch.randint(0, K, (N,), generator=g)
  if K > 2:
    labels[labels == K // 2] = 0                                      # an empty cluster
  idx = torch.randperm(N, generator=g)[:M]
  v = torch.rand(M, generator=g) ** 3
  clusters = vis.PointClusters(labels.cuda(), torch.zeros(K, 3, device="cuda"))
  seen = torch.arange(N, dtype=torch.int32, device="cuda") % 3
  out = clusters.view_features(idx.cuda(), v.cuda(), point_visible=seen)
  again = clusters.view_features(idx.cuda(), v.cuda())
  perm = torch.randperm(M, generator=g)
  shuffled = clusters.view_features(idx[perm].cuda(), v[perm].cuda(), validate=True)
  torch.cuda.synchronize()
  assert out.shape == (K,) and out.dtype == torch.float32
  host_seen = (np.arange(N) % 3).astype(np.int32)
  host = shim_view_features(shim, labels.numpy(), K, idx.numpy(), v.numpy(), point_visible=host_seen)
  assert np.array_equal(_np(out).view(np.uint32), host.view(np.uint32))
  assert torch.equal(out, again) and torch.equal(out, shuffled)
  assert np.array_equal(_np(seen), host_seen)
  ref, members = view_features_fp64(labels.numpy(), K, idx.numpy(), v.numpy())
  assert np.all(np.abs(_np(out) - ref) <= members * 2.0 ** -24 * ref)
  other = clusters.view_features(idx.cuda(), v.cuda(), vis_threshold=0.5)       # the scratch is refilled by every call
  host = shim_view_features(shim, labels.numpy(), K, idx.numpy(), v.numpy(), threshold=0.5)
  assert np.array_equal(_np(other).view(np.uint32), host.view(np.uint32))


def test_view_features_validate_and_errors():
  clusters = vis.PointClusters(torch.tensor([0, 1, 1, 0, 2], device="cuda"), torch.zeros(3, 3, device="cuda"))
  ok = clusters.view_features(torch.tensor([4, 1], device="cuda"), torch.tensor([0.5, 0.25], device="cuda"), validate=True)
  assert ok.tolist() == [0.0, 0.25, 0.5]
  one = torch.ones(2, device="cuda")
  with pytest.raises(ValueError):
    clusters.view_features(torch.tensor([1, 1], device="cuda"), one, validate=True)          # duplicate
  with pytest.raises(ValueError):
    clusters.view_features(torch.tensor([1, 5], device="cuda"), one, validate=True)          # out of range
  with pytest.raises(ValueError):
    clusters.view_features(torch.tensor([-1, 2], device="cuda"), one, validate=True)
  with pytest.raises(ValueError):
    clusters.view_features(torch.tensor([1, 2]), one)                                        # CPU tensor
  with pytest.raises(ValueError):
    clusters.view_features(torch.tensor([1, 2], device="cuda", dtype=torch.int32), one)
  with pytest.raises(ValueError):
    clusters.view_features(torch.tensor([1, 2], device="cuda"), one.double())
  with pytest.raises(ValueError):
    clusters.view_features(torch.tensor([1, 2, 3], device="cuda"), one)
  with pytest.raises(ValueError):
    clusters.view_features(torch.tensor([1, 2], device="cuda"), one, point_visible=torch.zeros(5, device="cuda"))
  with pytest.raises(ValueError):
    vis.PointClusters(torch.tensor([0, 3], device="cuda"), torch.zeros(3, 3, device="cuda")).view_features(
        torch.tensor([0], device="cuda"), one[:1])                                            # label out of range
  strided = torch.tensor([4, 9, 1, 9], device="cuda")[::2]                                    # non-contiguous: copied
  assert clusters.view_features(strided, torch.tensor([0.5, 9, 0.25, 9], device="cuda")[::2]).tolist() == [0.0, 0.25, 0.5]


# ---- 3. end to end -----------------------------------------------------------------------------------------------------

def test_renderer_to_view_clustering_end_to_end():
  V, n = 12, 30_000
  g, cams = synthetic.scene_b(n, 160, 120, sh_degree=0, seed=3, num_cameras=V, radius=3.0, sigma_px=2.0)
  position = g.position * 0.45
  position[: n // 2, 0] += 0.8                                          # two well-separated blobs
  position[n // 2:, 0] -= 0.8
  gd = sta.Gaussians3D(position.cuda(), g.rotation.cuda(), g.log_scaling.cuda(), torch.full_like(g.alpha_logit, 2.0).cuda(),
                       g.feature.cuda())
  cfg = sta.RasterConfig(compute_visibility=True)
  torch.manual_seed(0)
  clusters = vis.PointClusters.cluster(gd.position, 64)
  assert clusters.num_clusters == 64 and clusters.point_labels.shape == (n,)
  labels = _np(clusters.point_labels)
  point_visible = torch.zeros(n, dtype=torch.int32, device="cuda")
  rows, listed = [], []
  for cam in cams:
    with torch.no_grad():
      r = sta.render_gaussians(gd, cam.to("cuda"), cfg, use_sh=True)
    row = clusters.rendering_features(r, point_visible=point_visible)
    idx, v = _np(r.points.idx), _np(r.points.visibility)
    ref, members = view_features_fp64(labels, 64, idx, v)
    assert np.all(np.abs(_np(row) - ref) <= members * 2.0 ** -24 * ref)
    assert ref.sum() > 0
    rows.append(row)
    listed.append(idx[v > np.float32(0.01)])
  vc = vis.ViewClustering(clusters, torch.stack(rows))
  sim = vc.view_similarity
  assert sim.shape == (V, V) and torch.allclose(sim, sim.T, atol=1e-6)
  assert torch.allclose(sim.diagonal(), torch.ones(V, device="cuda"), atol=1e-5)
  for i in range(V):
    assert sim[i, (i + 1) % V] > sim[i, (i + V // 2) % V], (i, sim[i].tolist())
  w = torch.ones(V, device="cuda")
  for seed in range(3):
    torch.manual_seed(seed)
    batch = vc.sample_batch(w, 4, 0.5)
    torch.manual_seed(seed)
    assert torch.equal(batch, sample_batch_ref(sim, w, 4, 0.5))
  seen = set(_np(vc.visible_points(batch)).tolist())
  for i in batch.tolist():
    assert set(listed[i].tolist()) <= seen
  assert int(point_visible.sum()) > 0 and int(point_visible.max()) <= V


# ---- 4. clouds -----------------------------------------------------------------------------------------------------------

def _oracle_counts(cams, points):
  inside, near = frustum_fp64(_np(points), _np(cams.records()))
  return inside, near


def test_balanced_points_are_seen_by_enough_cameras():
  cams = camera_batch(vis, ring_cameras(16, seed=2, near=2.0, far=12.0), "cuda")
  torch.manual_seed(0)
  points, cam_counts = vis.balanced_points(cams, 4000, min_overlap=4)
  assert points.shape == (4000, 3) and cam_counts.shape == (16,) and cam_counts.dtype == torch.int32
  inside, near = _oracle_counts(cams, points)
  clear = near.sum(0) == 0                                              # points without a near-boundary pair
  assert clear.mean() > 0.99 and (inside.sum(0)[clear] >= 4).all()
  assert int(cam_counts.sum()) >= int(inside.sum()) - int(near.sum())
  more, _ = vis.balanced_points(cams, 5000, min_overlap=4, existing_points=points)
  assert more.shape == (5000, 3) and torch.equal(more[:4000], points)
  cloud_points, cloud_colors = vis.balanced_cloud(cams, 1000, 3)
  assert cloud_points.shape == (1000, 3) and cloud_colors.shape == (1000, 3)
  grown, colors = vis.balanced_cloud(cams, 1500, 3, existing_points=(cloud_points, cloud_colors))
  assert grown.shape == (1500, 3) and torch.equal(colors[:1000], cloud_colors)
  rp, rc = vis.random_cloud(cams, 500)
  assert rp.shape == (500, 3) and rc.shape == (500, 3) and (vis.point_visibility(cams, rp) >= 1).float().mean() > 0.99


def test_crop_cloud_and_foreground_points_match_the_reference_lines():
  cams = camera_batch(vis, ring_cameras(9, seed=4), "cuda")
  points = torch.from_numpy(ring_points(20_000, seed=8) * 2).cuda()
  colors = torch.rand(20_000, 3, device="cuda")
  args = (cams.image_t_world(), cams.image_sizes.tolist(), cams.depth_ranges.tolist(), points)
  _, near = _oracle_counts(cams, points)
  clear = torch.from_numpy(near.sum(0) == 0).cuda()
  ref_counts = point_visibility_torch(*args)
  assert torch.equal(vis.point_visibility(cams, points)[clear], ref_counts[clear])
  cropped_points, cropped_colors = vis.crop_cloud(cams, (points, colors))
  keep = vis.point_visibility(cams, points) > 0
  assert torch.equal(cropped_points, points[keep]) and torch.equal(cropped_colors, colors[keep])
  assert torch.equal(keep[clear], (ref_counts > 0)[clear]) and 0 < int(keep.sum()) < 20_000

  class Cloud:
    def __init__(self, points, colors):
      self.points, self.colors = points, colors

    def __getitem__(self, mask):
      return Cloud(self.points[mask], self.colors[mask])
  assert torch.equal(vis.crop_cloud(cams, Cloud(points, colors)).points, cropped_points)

  # the first camera's quantile is the threshold of every camera
  ref_near, threshold = foreground_visibility_torch(*args, far_threshold=None, quantile=0.25)
  _, near_t = frustum_fp64(_np(points), _np(cams.records()), depth_below=float(threshold))
  clear_t = torch.from_numpy(near_t.sum(0) == 0).cuda()
  ours = vis.foreground_visibility(cams, points, quantile=0.25)
  assert torch.equal(ours[clear_t], ref_near[clear_t]) and clear_t.float().mean() > 0.99
  assert torch.equal(ours, vis.frustum_counts(cams, points, depth_below=float(threshold))[0])
  assert (ours <= vis.point_visibility(cams, points)).all() and (ours < vis.point_visibility(cams, points)).any()
  mask = vis.foreground_points(cams, points, quantile=0.25, min_overlap=0.2)
  assert torch.equal(mask, ours > 0.2 * 9) and 0 < int(mask.sum()) < 20_000
  fixed = vis.foreground_points(cams, points, far_threshold=5.0)
  ref_fixed, _ = foreground_visibility_torch(*args, far_threshold=5.0)
  _, near_f = frustum_fp64(_np(points), _np(cams.records()), depth_below=5.0)
  clear_f = torch.from_numpy(near_f.sum(0) == 0).cuda()
  assert torch.equal(fixed[clear_f], (ref_fixed > 0.01 * 9)[clear_f])


# ---- 5. errors -----------------------------------------------------------------------------------------------------------

def test_value_errors_and_non_contiguous_points():
  cpu = camera_batch(vis, ring_cameras(3))
  cams = camera_batch(vis, ring_cameras(3), "cuda")
  p = torch.from_numpy(ring_points(100)).cuda()
  for fn in (vis.point_visibility, vis.camera_counts, vis.frustum_counts, vis.foreground_visibility):
    with pytest.raises(ValueError):
      fn(cams, p.cpu())                                                # CPU points
    with pytest.raises(ValueError):
      fn(cpu, p)                                                       # CPU cameras
    with pytest.raises(ValueError):
      fn(cams, p.double())
    with pytest.raises(ValueError):
      fn(cams, p[:, :2])
    with pytest.raises(ValueError):
      fn(cams, p[:0])
    with pytest.raises(ValueError):
      fn("cameras", p)
  with pytest.raises(ValueError):
    vis.CameraBatch(cams.camera_t_world[:0], cams.intrinsics[:0], cams.image_sizes[:0], cams.depth_ranges[:0])   # V = 0
  with pytest.raises(ValueError):
    vis.CameraBatch(cams.camera_t_world, cams.intrinsics[:2], cams.image_sizes, cams.depth_ranges)
  with pytest.raises(ValueError):
    vis.CameraBatch(cams.camera_t_world, cams.intrinsics.double(), cams.image_sizes, cams.depth_ranges)
  with pytest.raises(ValueError):
    vis.CameraBatch(cams.camera_t_world, cams.intrinsics, cams.image_sizes.float(), cams.depth_ranges)
  with pytest.raises(ValueError):
    vis.CameraBatch(cams.camera_t_world, cams.intrinsics.cpu(), cams.image_sizes, cams.depth_ranges)             # devices
  with pytest.raises(ValueError):
    vis.crop_cloud(cams, p)
  wide = torch.zeros(100, 6, device="cuda")
  wide[:, ::2] = p
  assert not wide[:, ::2].is_contiguous()
  assert torch.equal(vis.point_visibility(cams, wide[:, ::2]), vis.point_visibility(cams, p))


def test_camera_batch_from_params_and_reference_cameras_object():
  _, params = synthetic.scene_b(10, 64, 48, sh_degree=0, num_cameras=5)
  params = [c.to("cuda") for c in params]
  batch = vis.CameraBatch.from_params(params)
  assert len(batch) == 5 and batch.batch_size == (5,) and batch.device.type == "cuda"
  assert batch.image_sizes.tolist() == [[64, 48]] * 5 and torch.allclose(batch.depth_ranges[0].cpu(), torch.tensor([0.1, 100.0]))

  @dataclasses.dataclass
  class Projections:
    intrinsics: torch.Tensor
    image_size: torch.Tensor
    depth_range: torch.Tensor

  @dataclasses.dataclass
  class Cameras:
    camera_t_world: torch.Tensor
    projection: Projections
  like = Cameras(batch.camera_t_world, Projections(batch.intrinsics, batch.image_sizes, batch.depth_ranges))
  p = torch.randn(2000, 3, device="cuda")
  a = vis.point_visibility(params, p)
  assert torch.equal(a, vis.point_visibility(like, p)) and torch.equal(a, vis.point_visibility(batch, p))
  assert torch.equal(vis.point_visibility(params[0], p) > 0, vis.frustum_counts(params[:1], p)[0] > 0)
  assert 0 < int(a.sum())
