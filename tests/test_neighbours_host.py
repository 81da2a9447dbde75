"""CPU checks of the neighbour maths (csrc/gsr_neighbours.h, the source the HIP kernels compile) through the host shim:
kNN and nearest-centroid assignment against an fp64 numpy brute force -- distances within fp32 rounding, indices equal
except between distances that fp32 cannot tell apart, equal distances in index order, duplicates at distance 0, the
assignment's lowest-index tie-break and the label of an all-NaN point."""
import numpy as np
import pytest

import hostmath
from neighbours_oracle import dist2_fp64, knn_fp64, shim_assign, shim_knn

EPS = 4e-7          # relative: a few fp32 roundings of a squared distance


def _cloud(n, seed):
  rng = np.random.default_rng(seed)
  return (rng.standard_normal((n, 3)) * np.array([1.0, 2.0, 0.5]) + 3.0).astype(np.float32)


@pytest.mark.parametrize("n,k,seed", [(2, 1, 0), (17, 16, 1), (1000, 5, 2), (4096, 3, 3), (777, 16, 4)])
def test_knn_matches_fp64(built_libs, n, k, seed):
  lib = hostmath.load(built_libs)
  p = _cloud(n, seed)
  d, j, s = shim_knn(lib, p, k)
  D, J = knn_fp64(p, k)
  own = np.take_along_axis(dist2_fp64(p, p), j, 1)                      # fp64 distance of each chosen pair
  assert (j != np.arange(n)[:, None]).all()
  assert np.all(np.abs(d - own) <= EPS * own + 1e-30)
  assert np.all(np.abs(own - D) <= EPS * D + 1e-30)                      # the chosen ones are the nearest
  assert np.all(np.diff(d, axis=1) >= 0)
  # indices equal wherever the true distances are apart by more than fp32 rounding
  gap_lo = np.abs(D - np.concatenate([np.full((n, 1), -np.inf), D[:, :-1]], 1))
  gap_hi = np.abs(np.concatenate([D[:, 1:], np.full((n, 1), np.inf)], 1) - D)
  clear = (gap_lo > 2 * EPS * D) & (gap_hi > 2 * EPS * D)
  assert (j[clear] == J[clear]).all()
  assert np.allclose(s, np.sqrt(D).mean(1), rtol=1e-6, atol=0)


def test_knn_exact_ties_in_index_order(built_libs):
  """Integer lattice: every distance is exact in fp32, so the lists equal the fp64 (distance, index) order bit for bit."""
  lib = hostmath.load(built_libs)
  g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
  p = g[np.random.default_rng(0).permutation(len(g))].astype(np.float32)
  for k in (1, 6, 16):
    d, j, _ = shim_knn(lib, p, k)
    D, J = knn_fp64(p, k)
    assert (d == D).all() and (j == J).all(), k


def test_knn_duplicates_at_distance_zero(built_libs):
  lib = hostmath.load(built_libs)
  p = _cloud(50, 5)
  p = np.concatenate([p, p[:10], p[:3]])                 # 10 points twice, 3 of them three times
  d, j, s = shim_knn(lib, p, 2)
  for i in range(3):
    assert d[i, 0] == 0 and d[i, 1] == 0 and list(j[i]) == [50 + i, 60 + i]
    assert s[i] == 0
  for i in range(3, 10):
    assert d[i, 0] == 0 and j[i, 0] == 50 + i and d[i, 1] > 0
  assert d[60, 0] == 0 and list(j[60]) == [0, 50]


def test_knn_rows_of_a_range(built_libs):
  lib = hostmath.load(built_libs)
  p = _cloud(300, 6)
  d, j, s = shim_knn(lib, p, 4)
  d2, j2, s2 = shim_knn(lib, p, 4, rows=(100, 177))
  assert (d2 == d[100:177]).all() and (j2 == j[100:177]).all() and (s2 == s[100:177]).all()


def test_assign_matches_fp64(built_libs):
  lib = hostmath.load(built_libs)
  x, c = _cloud(4096, 7), _cloud(100, 8)
  labels = shim_assign(lib, x, c)
  D = dist2_fp64(x, c)
  best = D.min(1)
  assert np.all(np.abs(D[np.arange(len(x)), labels] - best) <= EPS * best + 1e-30)
  second = np.sort(D, 1)[:, 1]
  clear = second - best > 2 * EPS * best
  assert (labels[clear] == D.argmin(1)[clear]).all()


def test_assign_ties_go_to_the_lowest_index(built_libs):
  lib = hostmath.load(built_libs)
  c = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 2]], np.float32)
  x = np.array([[0, 0, 0], [0, 2, 0], [0, 0, 1], [5, 5, 5]], np.float32)
  # origin: 0,1,2,3 at 1 -> 0;  (0,2,0): 1 and 3 at 1 -> 1;  (0,0,1): 4 at 1 and 0..3 at 2 -> 4
  assert list(shim_assign(lib, x, c)[:3]) == [0, 1, 4]
  assert list(shim_assign(lib, x[:2], c[[4, 1, 3, 0]])) == [1, 1]     # origin: 1, 2, 3 at 1; (0,2,0): 1 and 2


def test_assign_all_nan_point_gets_label_zero(built_libs):
  lib = hostmath.load(built_libs)
  c = _cloud(9, 9)
  x = np.array([[np.nan, 0, 0], [0, np.nan, np.nan], [1, 2, 3]], np.float32)
  labels = shim_assign(lib, x, c)
  assert labels[0] == 0 and labels[1] == 0
  assert labels[2] == int(dist2_fp64(x[2:], c).argmin())
  c[0] = np.nan                                           # a NaN centroid never wins
  assert shim_assign(lib, np.array([[c[1, 0], c[1, 1], c[1, 2]]], np.float32), c)[0] == 1
