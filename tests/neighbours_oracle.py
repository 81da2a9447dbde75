"""Checkers for the neighbour searches (splat_trainer_amd.neighbours): the host shim's brute force (the same header as
the kernels), an fp64 numpy brute force, and torch restatements of the reference's pykeops formulations
(gaussians/loading.py estimate_scale, visibility/cluster.py kmeans_iter), chunked so that no N x N or N x K matrix of
the whole problem is held at once."""
import numpy as np
import torch


def shim_knn(lib, points: np.ndarray, k: int, rows=None):
  """(dist2, idx, scale) of the host shim for rows [i0, i1) (default: all)."""
  p = np.ascontiguousarray(points, np.float32)
  N = p.shape[0]
  i0, i1 = rows if rows is not None else (0, N)
  d = np.zeros((i1 - i0, k), np.float32)
  j = np.zeros((i1 - i0, k), np.int64)
  s = np.zeros(i1 - i0, np.float32)
  assert lib.hm_knn(p, N, k, i0, i1, d, j, s) == 0
  return d, j, s


def shim_assign(lib, x: np.ndarray, c: np.ndarray):
  x = np.ascontiguousarray(x, np.float32)
  c = np.ascontiguousarray(c, np.float32)
  labels = np.zeros(x.shape[0], np.int64)
  lib.hm_assign_clusters(x, x.shape[0], c, c.shape[0], labels)
  return labels


def dist2_fp64(q: np.ndarray, c: np.ndarray) -> np.ndarray:
  q, c = q.astype(np.float64), c.astype(np.float64)
  return ((q[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def knn_fp64(points: np.ndarray, k: int, chunk: int = 512):
  """Exact fp64 k nearest (self excluded), ordered by (distance, index)."""
  N = points.shape[0]
  D, J = np.zeros((N, k)), np.zeros((N, k), np.int64)
  for a in range(0, N, chunk):
    d = dist2_fp64(points[a:a + chunk], points)
    d[np.arange(d.shape[0]), np.arange(a, a + d.shape[0])] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    J[a:a + chunk] = order
    D[a:a + chunk] = np.take_along_axis(d, order, 1)
  return D, J


def estimate_scale_torch(points: torch.Tensor, num_neighbors: int, chunk: int = 4096) -> torch.Tensor:
  """The reference's estimate_scale: Kmin(k + 1) of the squared distances (self included, at 0), the first dropped,
  sqrt, mean -- over query chunks."""
  out = []
  for a in range(0, points.shape[0], chunk):
    d = ((points[a:a + chunk, None, :] - points[None, :, :]) ** 2).sum(-1)
    kmin = torch.topk(d, num_neighbors + 1, dim=1, largest=False, sorted=True).values
    out.append(kmin[:, 1:].sqrt().mean(dim=1))
  return torch.cat(out)


def assign_torch(x: torch.Tensor, c: torch.Tensor, chunk: int = 65536) -> torch.Tensor:
  return torch.cat([((x[a:a + chunk, None, :] - c[None]) ** 2).sum(-1).argmin(dim=1)
                    for a in range(0, x.shape[0], chunk)])


def kmeans_iter_torch(x: torch.Tensor, centroids: torch.Tensor, iters: int):
  """The reference's Lloyd loop: assign, zero, scatter_add the points, divide by the counts (in place)."""
  K, D = centroids.shape
  for _ in range(iters):
    labels = assign_torch(x, centroids)
    centroids.zero_()
    centroids.scatter_add_(0, labels[:, None].repeat(1, D), x)
    counts = torch.bincount(labels, minlength=K).type_as(centroids).view(K, 1)
    centroids /= counts
  return labels, centroids


def blobs(n: int, k: int, seed: int, spread: float = 0.02, box: float = 10.0):
  """n points around k well-separated centres (a jittered grid of pitch >= box / ceil(k^(1/3)))."""
  g = torch.Generator().manual_seed(seed)
  side = int(np.ceil(k ** (1 / 3)))
  cells = torch.randperm(side ** 3, generator=g)[:k]
  centres = torch.stack([cells % side, (cells // side) % side, cells // (side * side)], 1).float() * (box / side)
  labels = torch.randint(0, k, (n,), generator=g)
  labels[:k] = torch.arange(k)                        # every blob has a point
  return centres[labels] + spread * torch.randn(n, 3, generator=g), centres, labels
