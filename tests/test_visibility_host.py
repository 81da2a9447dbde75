"""CPU checks of the frustum test and the view-feature sums (csrc/gsr_visibility.h, the source the HIP kernels compile)
through the host shim against fp64 numpy, and of the torch-only parts of splat_trainer_amd.visibility (normalisation,
overlaps, the sampling functions, the two samplers, every state_dict) on CPU tensors against the reference's lines."""
import numpy as np
import pytest
import torch

import hostmath
from splat_trainer_amd import visibility as vis
from visibility_oracle import (camera_batch, frustum_fp64, normalized_visibility_ref, overlaps_ref, ring_cameras,
                               ring_points, sample_batch_grouped_ref, sample_batch_ref, sample_with_temperature_ref,
                               select_batch_ref, shim_frustum, shim_view_features, view_features_fp64)

@pytest.fixture(scope="module")
def shim(built_libs):
  return hostmath.load(built_libs)


# ---- 1. the issue's scene ----------------------------------------------------------------------------------------------

def test_frustum_counts_match_fp64_on_the_ring_scene(shim):
  """64 cameras on a ring of radius 6, 200 000 points N(0, diag(3, 1.5, 3)^2): every pair that is not near a boundary
  agrees with fp64, every count lies within the oracle's +- its near-boundary pairs, and those pairs are rare."""
  records = camera_batch(vis, ring_cameras(64, seed=0)).records().numpy()
  assert records.shape == (64, 16) and records.dtype == np.float32
  points = ring_points(200_000, seed=0)
  inside, near = frustum_fp64(points, records)
  share = near.mean()
  print(f"near-boundary share {share:.3g}, inside {inside.mean():.3f}, "
        f"points seen by >= 4 cameras {(inside.sum(0) >= 4).mean():.4f}")
  assert share < 1e-4
  assert 0.05 < inside.mean() < 0.95                   # both outcomes are exercised
  pc, cc = shim_frustum(shim, points, records)
  assert np.all(np.abs(pc - inside.sum(0)) <= near.sum(0))
  assert np.all(np.abs(cc - inside.sum(1)) <= near.sum(1))
  # pair by pair: one camera at a time through the shim
  disagree = 0
  for c in range(64):
    one, _ = shim_frustum(shim, points, records[c:c + 1], want_cameras=False)
    disagree += int(((one != 0) != inside[c])[~near[c]].sum())
  print(f"disagreements away from a boundary: {disagree} of {inside.size}")
  assert disagree == 0


# ---- 2. hand-made records ----------------------------------------------------------------------------------------------

def _identity_record(w=4.0, h=2.0, near=1.0, far=8.0):
  """h_0 = x, h_1 = y, d = z: the bounds can be hit exactly."""
  return np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, w, h, near, far]], dtype=np.float32)


@pytest.mark.parametrize("point,expect", [
    ((0.0, 0.0, 2.0), 1),        # h_0 = 0 and h_1 = 0: inside
    ((-1e-6, 0.5, 2.0), 0),      # h_0 < 0
    ((8.0, 0.5, 2.0), 0),        # h_0 = w d: outside
    ((7.999, 0.5, 2.0), 1),
    ((0.5, -1e-6, 2.0), 0),      # h_1 < 0
    ((0.5, 4.0, 2.0), 0),        # h_1 = h d: outside
    ((0.5, 3.999, 2.0), 1),
    ((0.5, 0.5, 1.0), 0),        # d = near: outside
    ((0.5, 0.5, 1.0001), 1),
    ((0.5, 0.5, 8.0), 0),        # d = far: outside
    ((0.5, 0.5, 7.999), 1),
    ((0.5, 0.5, -2.0), 0),       # behind the camera: d < 0
    ((-0.5, -0.5, -2.0), 0),     # behind, where the divided form would give positive xy
    ((float("nan"), 0.5, 2.0), 0), ((0.5, float("nan"), 2.0), 0), ((0.5, 0.5, float("nan")), 0),
])
def test_frustum_bounds_exactly(shim, point, expect):
  pc, cc = shim_frustum(shim, np.array([point], dtype=np.float32), _identity_record())
  assert pc[0] == expect and cc[0] == expect


def test_frustum_depth_below_and_counts(shim):
  pts = np.array([[0.5, 0.5, 2.0], [0.5, 0.5, 3.0], [0.5, 0.5, 5.0], [100.0, 0.5, 2.0]], dtype=np.float32)
  rec = np.concatenate([_identity_record(), _identity_record(far=4.0), _identity_record(near=2.5)])
  pc, cc = shim_frustum(shim, pts, rec)
  assert pc.tolist() == [2, 3, 2, 0] and cc.tolist() == [3, 2, 2]
  pc, cc = shim_frustum(shim, pts, rec, depth_below=3.0)            # d < min(far, 3): d = 3 is outside
  assert pc.tolist() == [2, 0, 0, 0] and cc.tolist() == [1, 1, 0]
  only_p, none = shim_frustum(shim, pts, rec, want_cameras=False)
  none2, only_c = shim_frustum(shim, pts, rec, want_points=False)
  assert none is None and none2 is None and only_p.tolist() == [2, 3, 2, 0] and only_c.tolist() == [3, 2, 2]


def test_records_layout():
  cams = ring_cameras(5, seed=3)
  batch = camera_batch(vis, cams)
  rec = batch.records()
  assert rec is batch.records()                                     # cached
  ctw, intr, sizes, ranges = (torch.from_numpy(a) for a in cams)
  K = torch.zeros(5, 4, 4)
  K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2], K[:, 3, 3] = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 1, 1
  assert torch.equal(rec[:, :12], (K @ ctw)[:, :3].reshape(5, 12))
  assert torch.equal(rec[:, 12:14], sizes.float()) and torch.equal(rec[:, 14:], ranges)


# ---- 3. view features --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,M,seed", [(1, 1, 1, 0), (1000, 7, 400, 1), (50_000, 64, 30_000, 2), (20_000, 300, 20_000, 3),
                                        (5000, 3, 0, 4)])
def test_view_features_match_fp64_and_ignore_the_list_order(shim, N, K, M, seed):
  rng = np.random.default_rng(seed)
  labels = rng.integers(0, K, N)
  labels[labels == K // 2] = 0 if K > 2 else labels[0]               # an empty cluster when K > 2
  idx = rng.permutation(N)[:M]
  v = (rng.random(M) ** 3).astype(np.float32)
  out = shim_view_features(shim, labels, K, idx, v)
  ref, members = view_features_fp64(labels, K, idx, v)
  assert np.all(np.abs(out - ref) <= members * 2.0 ** -24 * ref)
  assert np.all(out[members == 0] == 0)
  perm = rng.permutation(M)
  again = shim_view_features(shim, labels, K, idx[perm], v[perm])
  assert np.array_equal(out.view(np.uint32), again.view(np.uint32))


def test_view_features_threshold_is_strict_and_point_visible_counts(shim):
  labels = np.array([0, 0, 1, 1, 2, 2], dtype=np.int64)
  idx = np.array([5, 0, 2, 3], dtype=np.int64)
  v = np.array([0.5, np.float32(0.01), 0.25, 0.0], dtype=np.float32)
  seen = np.array([0, 1, 0, 0, 0, 7], dtype=np.int32)
  out = shim_view_features(shim, labels, 4, idx, v, threshold=0.01, point_visible=seen)
  assert out.tolist() == [0.0, 0.25, 0.5, 0.0]                        # vis == threshold dropped, cluster 3 empty
  assert seen.tolist() == [1, 1, 1, 1, 0, 8]


# ---- 4. the torch-only parts ---------------------------------------------------------------------------------------------

def _clustering(V=12, K=9, seed=0, metric="cosine"):
  g = torch.Generator().manual_seed(seed)
  table = torch.rand(V, K, generator=g) * (torch.rand(V, K, generator=g) > 0.3)
  clusters = vis.PointClusters(torch.randint(0, K, (50,), generator=g), torch.rand(K, 3, generator=g))
  return vis.ViewClustering(clusters, table, metric)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_normalized_visibility_and_overlaps(metric):
  vc = _clustering(metric=metric)
  ref = normalized_visibility_ref(vc.cluster_visibility)
  assert torch.equal(vc.normalized_visibility, ref) and vc.normalized_visibility is vc.normalized_visibility
  assert torch.equal(vc.view_similarity, overlaps_ref(ref, ref, metric))
  assert torch.equal(vc.overlaps_with(ref[:3]), overlaps_ref(ref[:3], ref, metric))
  with pytest.raises(ValueError):
    vis.ViewClustering(vc.point_clusters, vc.cluster_visibility, "manhattan")


@pytest.mark.parametrize("temperature", [0.0, 0.5, 1.0, 2.0])
def test_sampling_functions_draw_the_reference_indices(temperature):
  vc = _clustering(V=16, seed=1)
  sim = vc.view_similarity.clone()
  w = torch.rand(16, generator=torch.Generator().manual_seed(2)) + 0.1
  w[3] = 0
  for seed in range(5):
    for n, weighting in ((1, None), (4, None), (3, w)):
      torch.manual_seed(seed)
      a = vis.sample_with_temperature(sim[0] + 1e-3, temperature, n, weighting)
      torch.manual_seed(seed)
      b = sample_with_temperature_ref(sim[0] + 1e-3, temperature, n, weighting)
      assert torch.equal(a, b)
    for batch_size in (1, 2, 6):
      torch.manual_seed(seed)
      a = vis.sample_batch(sim, w, batch_size, temperature)
      torch.manual_seed(seed)
      b = sample_batch_ref(sim, w, batch_size, temperature)
      assert torch.equal(a, b) and a.shape == (batch_size,)
      torch.manual_seed(seed)
      a = vc.sample_batch(w, batch_size, temperature)
      assert torch.equal(a, b)
      torch.manual_seed(seed)
      a = vis.sample_batch_grouped(batch_size, sim, w, temperature)
      torch.manual_seed(seed)
      b = sample_batch_grouped_ref(batch_size, sim, w, temperature)
      assert torch.equal(a, b) and a.shape == (batch_size,)
  assert torch.equal(vc.view_similarity, sim)                      # the cached matrix is not written


def test_select_batch_draws_the_reference_indices():
  vc = _clustering(V=16, seed=3)
  w = torch.ones(16)
  for seed in range(5):
    for threshold, min_size in ((0.4, 3), (0.9, 5), (0.0, 1)):
      torch.manual_seed(seed)
      a = vc.select_batch(w, min_size, threshold)
      torch.manual_seed(seed)
      b = select_batch_ref(vc.view_similarity, w, threshold, min_size)
      assert torch.equal(a, b) and a.shape[0] >= min_size
      torch.manual_seed(seed)
      assert torch.equal(vis.select_batch(vc.view_similarity, w, threshold, min_size), b)


def test_sinkhorn_is_doubly_stochastic():
  m = vis.sinkhorn(torch.rand(8, 8, generator=torch.Generator().manual_seed(0)) + 0.1, 50)
  assert torch.allclose(m.sum(0), torch.ones(8), atol=1e-4) and torch.allclose(m.sum(1), torch.ones(8), atol=1e-3)


def test_visible_points_and_inverse_ndc_depth():
  labels = torch.tensor([0, 2, 1, 2, 0, 3])
  clusters = vis.PointClusters(labels, torch.zeros(4, 3))
  vc = vis.ViewClustering(clusters, torch.tensor([[1.0, 0, 0, 0], [0, 0, 0.5, 0], [0, 0, 0, 0]]))
  assert vc.visible_points(torch.tensor([0])).tolist() == [0, 4]
  assert vc.visible_points(torch.tensor([0, 1])).tolist() == [0, 1, 3, 4]
  assert vc.visible_points(torch.tensor([2])).tolist() == []
  assert clusters.num_clusters == 4
  d = vis.inverse_ndc_depth(torch.tensor([0.0, 1.0]), 0.1, 100.0)
  assert torch.allclose(d, torch.tensor([0.1, 99.0]), rtol=1e-3)   # query_points.py:47 as written: (nf - n) / n at 1
  torch.manual_seed(0)
  r = vis.random_ndc(1000, (0.1, 100.0), device="cpu")
  assert r.shape == (1000, 1) and (r >= 0.1).all() and (r <= 100.0).all()


def test_batch_overlap_sampler_bookkeeping():
  vc = _clustering(V=10, seed=4)
  cfg = vis.BatchOverlapSamplerConfig(batch_size=4, overlap_temperature=0.5)
  sampler = cfg.create(torch.arange(10))
  torch.manual_seed(0)
  used = []
  for step in range(2):
    expect_w = torch.nn.functional.normalize(1 / (sampler.view_counts + 1), p=1, dim=0)
    expect_w[sampler.used_mask] = 0
    state = torch.get_rng_state()
    batch = sampler.select_images(vc, None)
    torch.set_rng_state(state)
    assert torch.equal(batch, sample_batch_ref(vc.view_similarity, expect_w, 4, 0.5))
    assert batch.shape == (4,) and len(set(batch.tolist())) == 4 and not set(batch.tolist()) & set(used)
    used += batch.tolist()
  assert sampler.used_mask.sum() == 8 and sampler.view_counts.sum() == 8
  sampler.used_mask.fill_(True)                                     # all used: the mask resets before the next draw
  batch = sampler.select_images(vc)
  assert sampler.used_mask.sum() == 4 and sampler.view_counts.sum() == 12
  again = cfg.from_state_dict(sampler.state_dict(), torch.arange(10))
  assert torch.equal(again.view_counts, sampler.view_counts) and not again.used_mask.any()


def test_random_sampler_walks_a_permutation_and_reshuffles():
  cfg = vis.RandomSamplerConfig(batch_size=4)
  train_idx = torch.arange(100, 110)
  torch.manual_seed(5)
  sampler = cfg.create(train_idx)
  torch.manual_seed(5)
  perm = train_idx[torch.randperm(10)]
  assert torch.equal(sampler.select_images(None, None), perm[:4]) and torch.equal(sampler.select_images(), perm[4:8])
  restored = cfg.from_state_dict(sampler.state_dict(), train_idx)
  assert torch.equal(restored.next, perm[8:])
  torch.manual_seed(6)
  batch = sampler.select_images()                                   # two left: a new permutation
  torch.manual_seed(6)
  assert torch.equal(batch, train_idx[torch.randperm(10)][:4]) and sampler.next.shape[0] == 6


def test_state_dict_round_trips():
  vc = _clustering(seed=6, metric="euclidean")
  back = vis.ViewClustering.from_state_dict(vc.state_dict())
  assert back.metric == "euclidean" and torch.equal(back.cluster_visibility, vc.cluster_visibility)
  assert torch.equal(back.point_clusters.point_labels, vc.point_clusters.point_labels)
  assert torch.equal(back.point_clusters.centroids, vc.point_clusters.centroids)
  assert torch.equal(back.view_similarity, vc.view_similarity)
  pc = vis.PointClusters.from_state_dict(vc.point_clusters.state_dict())
  assert pc.num_clusters == vc.point_clusters.num_clusters


def test_cpu_tensors_are_refused_by_the_native_calls():
  batch = camera_batch(vis, ring_cameras(3))
  with pytest.raises(ValueError):
    vis.point_visibility(batch, torch.zeros(10, 3))
  clusters = vis.PointClusters(torch.zeros(10, dtype=torch.int64), torch.zeros(1, 3))
  with pytest.raises(ValueError):
    clusters.view_features(torch.arange(3), torch.ones(3))
  with pytest.raises(ValueError):
    vis.CameraBatch.from_params([])
  with pytest.raises(ValueError):
    vis.CameraBatch(torch.zeros(0, 4, 4), torch.zeros(0, 4), torch.zeros(0, 2, dtype=torch.int64), torch.zeros(0, 2))
