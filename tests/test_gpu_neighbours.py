"""The neighbour searches on the MI355X (splat_trainer_amd.neighbours): kNN and assignment bit-identical to the host shim
(the same header), estimate_scale and k-means against torch restatements of the reference's pykeops formulations,
determinism, the in-place contract of kmeans_iter, empty clusters, the reference's initial rows and every ValueError."""
import numpy as np
import pytest
import torch

import hostmath
import splat_trainer_amd as sta
from neighbours_oracle import (assign_torch, blobs, estimate_scale_torch, kmeans_iter_torch, shim_assign, shim_knn)

pytestmark = pytest.mark.gpu


def _cloud(n, seed, device="cuda"):
  g = torch.Generator().manual_seed(seed)
  return (torch.randn(n, 3, generator=g) * torch.tensor([1.0, 2.0, 0.5]) + 3.0).to(device)


def _rows(n):
  """Rows the shim recomputes: all for small clouds, the first and last 1536 otherwise (the tail wave included)."""
  return [(0, n)] if n <= 4096 else [(0, 1536), (n - 1536, n)]


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("n", ["k+1", 1000, 65537])
def test_knn_bit_identical_to_host(built_libs, n, k):
  lib = hostmath.load(built_libs)
  n = k + 1 if n == "k+1" else n
  p = _cloud(n, 10 + k)
  d, j = sta.knn(p, k)
  s = sta.estimate_scale(p, num_neighbors=k)
  torch.cuda.synchronize()
  assert d.shape == (n, k) and d.dtype == torch.float32 and j.shape == (n, k) and j.dtype == torch.int64
  pn = p.cpu().numpy()
  for a, b in _rows(n):
    hd, hj, hs = shim_knn(lib, pn, k, rows=(a, b))
    assert np.array_equal(d[a:b].cpu().numpy().view(np.uint32), hd.view(np.uint32)), (a, b)
    assert np.array_equal(j[a:b].cpu().numpy(), hj), (a, b)
    assert np.array_equal(s[a:b].cpu().numpy().view(np.uint32), hs.view(np.uint32)), (a, b)


def test_knn_duplicates_and_lattice_ties(built_libs):
  lib = hostmath.load(built_libs)
  g = torch.stack(torch.meshgrid(torch.arange(20), torch.arange(12), torch.arange(9), indexing="ij"), -1).reshape(-1, 3)
  p = g[torch.randperm(len(g), generator=torch.Generator().manual_seed(0))].float()
  p = torch.cat([p, p[:100]])                                  # duplicates: distance 0
  for k in (3, 16):
    d, j = sta.knn(p.cuda(), k)
    hd, hj, _ = shim_knn(lib, p.numpy(), k)
    assert np.array_equal(d.cpu().numpy(), hd) and np.array_equal(j.cpu().numpy(), hj)
    assert (d[:100, 0] == 0).all() and (j[:100, 0] == torch.arange(len(g), len(g) + 100, device="cuda")).all()


def test_assign_bit_identical_to_host(built_libs):
  lib = hostmath.load(built_libs)
  for n, K, seed in [(1, 1, 0), (1000, 7, 1), (65537, 256, 2), (200_000, 100, 3)]:
    x, c = _cloud(n, seed), _cloud(K, 100 + seed)
    labels = sta.assign_clusters(x, c)
    assert labels.dtype == torch.int64 and labels.shape == (n,)
    assert np.array_equal(labels.cpu().numpy(), shim_assign(lib, x.cpu().numpy(), c.cpu().numpy())), (n, K)
  x = torch.tensor([[float("nan"), 0, 0], [0, 0, 0]], device="cuda")
  c = torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 1, 0]], device="cuda")
  assert sta.assign_clusters(x, c).tolist() == [0, 0]


def test_estimate_scale_matches_reference_restatement():
  p = _cloud(20_000, 4)
  for k in (3, 5):
    got = sta.estimate_scale(p, num_neighbors=k)
    want = estimate_scale_torch(p.double(), k)
    assert ((got.double() - want).abs() / want).max().item() < 1e-6

  class Cloud:                                                  # the reference passes a PointCloud
    points = p
  assert torch.equal(sta.estimate_scale(Cloud()), sta.estimate_scale(p, 3))


def test_kmeans_iter_matches_reference_loop():
  x, centres, _ = blobs(150_000, 200, seed=1)
  x = x.cuda()
  init = x[torch.randperm(200, generator=torch.Generator().manual_seed(2)).cuda()]   # one point of every blob
  labels, c = sta.kmeans_iter(x, init.clone(), iters=15)
  ref_labels, ref_c = kmeans_iter_torch(x, init.clone(), 15)
  assert torch.equal(labels, ref_labels)
  assert torch.isfinite(ref_c).all()
  assert ((c - ref_c).abs().max() / ref_c.abs().max()).item() < 1e-5


def test_kmeans_iter_is_bit_reproducible_and_in_place():
  x = _cloud(100_003, 5)
  init = x[:256].clone()
  c1 = init.clone()
  l1, r1 = sta.kmeans_iter(x, c1, iters=7)
  assert r1 is c1 and r1.data_ptr() == c1.data_ptr()
  c2 = init.clone()
  l2, r2 = sta.kmeans_iter(x, c2, iters=7)
  assert torch.equal(l1, l2) and torch.equal(c1.view(torch.int32), c2.view(torch.int32))
  # the labels come from the last assignment, made before the last update
  c6 = init.clone()
  sta.kmeans_iter(x, c6, iters=6)
  assert torch.equal(l1, sta.assign_clusters(x, c6))


def test_kmeans_iter_non_contiguous_centroids_updated_in_place():
  x = _cloud(5000, 6)
  buf = torch.zeros(8, 6, device="cuda")
  view = buf[:, ::2]
  view.copy_(x[:8])
  want_l, want_c = sta.kmeans_iter(x, x[:8].clone(), iters=3)
  l, c = sta.kmeans_iter(x, view, iters=3)
  assert c is view and torch.equal(view, want_c) and torch.equal(l, want_l)


def test_empty_cluster_keeps_its_centroid():
  x = _cloud(4000, 7)
  far = torch.tensor([[1e4, 1e4, 1e4]], device="cuda")
  c = torch.cat([x[:5], far])
  labels, out = sta.kmeans_iter(x, c, iters=1)
  assert torch.equal(out[5], far[0]) and not (labels == 5).any()
  for j in range(5):                                            # the others are the means of their points
    want = x[labels == j].double().mean(0)
    assert ((out[j].double() - want).abs().max() / want.abs().max()).item() < 1e-5


def test_kmeans_picks_the_reference_rows():
  x = _cloud(3000, 8)
  torch.manual_seed(123)
  labels, c = sta.kmeans(x, k=12, iters=1)
  torch.manual_seed(123)
  init = x[torch.randperm(x.shape[0])[:12].cuda()]
  want_l, want_c = sta.kmeans_iter(x, init.clone(), iters=1)
  assert torch.equal(labels, want_l) and torch.equal(c, want_c)
  assert torch.equal(labels, sta.assign_clusters(x, init))


def test_value_errors():
  p = _cloud(100, 9)
  cpu = p.cpu()
  bad = [lambda: sta.knn(cpu, 3), lambda: sta.knn(p.double(), 3), lambda: sta.knn(p[:, :2], 3),
         lambda: sta.knn(p.reshape(-1), 3), lambda: sta.knn(p, 0), lambda: sta.knn(p, 17), lambda: sta.knn(p[:5], 5),
         lambda: sta.knn(p, 2.0), lambda: sta.knn([[1.0, 2.0, 3.0]] * 4, 1),
         lambda: sta.estimate_scale(cpu), lambda: sta.estimate_scale(p, num_neighbors=0),
         lambda: sta.assign_clusters(cpu, p[:4]), lambda: sta.assign_clusters(p, cpu[:4]),
         lambda: sta.assign_clusters(p, p[:4].half()), lambda: sta.assign_clusters(p, p[:0]),
         lambda: sta.assign_clusters(p, p[:4, :2]), lambda: sta.assign_clusters(p[:0], p[:4]),
         lambda: sta.kmeans_iter(p, p[:4].clone(), iters=0), lambda: sta.kmeans_iter(p, p[:4].clone(), iters=2.5),
         lambda: sta.kmeans_iter(p, cpu[:4].clone()), lambda: sta.kmeans_iter(p.double(), p[:4].clone()),
         lambda: sta.kmeans(p, k=0), lambda: sta.kmeans(p, k=101), lambda: sta.kmeans(cpu, k=3)]
  for i, f in enumerate(bad):
    with pytest.raises(ValueError):
      f()
      pytest.fail(f"case {i} did not raise")
  # non-contiguous points are copied, not refused
  q = torch.zeros(100, 6, device="cuda")[:, ::2]
  q.copy_(p)
  assert torch.equal(sta.knn(q, 3)[1], sta.knn(p, 3)[1])
