"""Oracles for splat_trainer_amd.sh_fit (the direct least-squares SH export fit).  The reference fits by Adam steps, so
there is no golden file from it: the oracle is this build's own, as for the 3-D filter.

* the fp64 ORACLE: the real SH basis rebuilt from its polynomial definitions in fp64 (checked against
  tests/golden/rsh_deg0_4.npz by test_sh_fit_host.py), the normal equations G = sum w Y Y^T, b_c = sum w Y (y_c - 0.5),
  W = sum w per point, ``np.linalg.solve`` of (G + ridge W Y0^2 diag(0, 1, ..., 1)) s_c = b_c, and the objective J_p;
* the RESTATEMENT: the same algorithm with the direction and the basis in float32, operation by operation as
  csrc/gsr_sh_fit.h has them, everything after them fp64, the result rounded to float32;
* the scenes the checks use and the wrappers of the host shim.

How two solutions are compared.  With many views (V = 64) the coefficients are well conditioned and are compared
directly.  With few views they are ill conditioned by construction and the objective is compared instead: s* being
the oracle's minimiser, J_p(s) - J_p(s*) = sum_c d_c^T A d_c with d = s - s* and A the ridge matrix -- evaluated in that
form, which does not cancel -- relative to J_p(s*) + 2^-24 J_p(0).  The second term is a floor: J_p(s*) is 0 to rounding
for a point seen by one view (the unpenalised constant term fits one colour exactly), and the colours and weights that
define J_p are float32 numbers, so its data term J_p(0) = sum w (y - 0.5)^2 is not given more finely than one part in
2^24.
"""
import math
from typing import NamedTuple

import numpy as np

F = np.float32
RADIUS = 4.0
NOISE = 0.02
KEEP = 0.7
# chosen by ridge_experiment() from (1e-3, 1e-2, 1e-1): see test_sh_fit_host.py and profiles/r18_sh_fit.txt
DEFAULT_RIDGE = 1e-1
MIN_RIDGE = 1e-6
# measured for the restatement against the oracle (test_sh_fit_host.py prints them): the largest |coefficient
# difference| on the V = 64 scenes at ridge 1e-6 and the default, degrees 0..3, and the largest relative excess of J on
# the V in {1, 2, 4, 8} scenes at the default ridge
RESTATEMENT_COEF, RESTATEMENT_J, MARGIN = 7.4e-8, 2.0e-7, 4.0
FLOOR = 2.0 ** -24


# ---- the basis -----------------------------------------------------------------------------------------------------------

def basis_fp64(d, K):
  """Y (..., K) of unit directions d (..., 3), from the polynomial definitions (k = n (n + 1) + m)."""
  d = np.asarray(d, dtype=np.float64)
  x, y, z = d[..., 0], d[..., 1], d[..., 2]
  pi = math.pi
  Y = [np.full(x.shape, 0.5 * math.sqrt(1.0 / pi))]
  if K > 1:
    c1 = math.sqrt(3.0 / (4.0 * pi))
    Y += [-c1 * y, c1 * z, -c1 * x]
  if K > 4:
    a, b, c = 0.5 * math.sqrt(15.0 / pi), 0.25 * math.sqrt(5.0 / pi), 0.25 * math.sqrt(15.0 / pi)
    Y += [a * x * y, -a * y * z, b * (2 * z * z - x * x - y * y), -a * x * z, c * (x * x - y * y)]
  if K > 9:
    a, b = 0.25 * math.sqrt(35.0 / (2.0 * pi)), 0.5 * math.sqrt(105.0 / pi)
    c, e, f = 0.25 * math.sqrt(21.0 / (2.0 * pi)), 0.25 * math.sqrt(7.0 / pi), 0.25 * math.sqrt(105.0 / pi)
    Y += [-a * y * (3 * x * x - y * y), b * x * y * z, -c * y * (4 * z * z - x * x - y * y),
          e * z * (2 * z * z - 3 * x * x - 3 * y * y), -c * x * (4 * z * z - x * x - y * y), f * z * (x * x - y * y),
          -a * x * (x * x - 3 * y * y)]
  return np.stack(Y[:K], axis=-1)


Y0 = 0.5 * math.sqrt(1.0 / math.pi)


def basis_f32(x, y, z, K):
  """gsr_sh_basis<K> (csrc/gsr_math.h) in numpy float32: the same products and sums, each rounded on its own."""
  x, y, z = (np.asarray(t, dtype=F) for t in (x, y, z))
  c = lambda v: F(v)
  Y = [np.full(x.shape, c(0.28209479177387814), dtype=F)]
  if K > 1:
    Y += [-c(0.4886025119029199) * y, c(0.4886025119029199) * z, -c(0.4886025119029199) * x]
  if K > 4:
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    Y += [c(1.0925484305920792) * xy, -c(1.0925484305920792) * yz, c(0.31539156525252005) * (c(2) * zz - xx - yy),
          -c(1.0925484305920792) * xz, c(0.5462742152960396) * (xx - yy)]
    if K > 9:
      Y += [-c(0.5900435899266435) * y * (c(3) * xx - yy), c(2.890611442640554) * xy * z,
            -c(0.4570457994644658) * y * (c(4) * zz - xx - yy),
            c(0.3731763325901154) * z * (c(2) * zz - c(3) * xx - c(3) * yy),
            -c(0.4570457994644658) * x * (c(4) * zz - xx - yy), c(1.445305721320277) * z * (xx - yy),
            -c(0.5900435899266435) * x * (xx - c(3) * yy)]
  out = np.stack(Y[:K], axis=-1)
  assert out.dtype == F
  return out


def view_basis_fp64(points, camera, K):
  v = np.asarray(points, dtype=np.float64) - np.asarray(camera, dtype=np.float64)
  return basis_fp64(v / np.linalg.norm(v, axis=-1, keepdims=True), K)


def view_basis_f32(points, camera, K):
  """gsr_shf_operands: v = p - c, inv = 1 / sqrt((vx vx + vy vy) + vz vz), the basis at v inv -- all float32."""
  p, c = np.asarray(points, dtype=F), np.asarray(camera, dtype=F)
  vx, vy, vz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
  inv = F(1) / np.sqrt((vx * vx + vy * vy) + vz * vz)
  return basis_f32(vx * inv, vy * inv, vz * inv, K)


# ---- scenes ------------------------------------------------------------------------------------------------------------------

class Scene(NamedTuple):
  positions: np.ndarray      # (N, 3) float32, in the unit ball
  cameras: np.ndarray        # (V, 3) float32, on the sphere of radius RADIUS
  views: list                # per camera (idx (M,) int64 ascending and distinct, colours (M, 3) float32, weights (M,) float32)
  truth: np.ndarray          # (N, 3, truth K) fp64: the coefficients the colours were made from
  unseen: np.ndarray         # the points left out of every view


def unit_vectors(rng, n):
  v = rng.standard_normal((n, 3))
  return v / np.linalg.norm(v, axis=1, keepdims=True)


def sphere_views(V, seed, N=257, truth_degree=3, noise=NOISE, scale=0.05, keep=KEEP):
  """V cameras on the sphere of radius 4 around N points in the unit ball; every view keeps each point with probability
  ``keep`` and min(3, N // 16) points are in no view; weights in [0.1, 1]; colours 0.5 + truth . Y + N(0, noise), clipped to
  [0, 1], from random coefficients of ``truth_degree``."""
  rng = np.random.default_rng(seed)
  positions = (unit_vectors(rng, N) * rng.uniform(0, 1, (N, 1)) ** (1 / 3)).astype(F)
  cameras = (unit_vectors(rng, V) * RADIUS).astype(F)
  Kt = (truth_degree + 1) ** 2
  truth = rng.standard_normal((N, 3, Kt)) * scale
  unseen = rng.permutation(N)[:min(3, N // 16)]
  allowed = np.ones(N, dtype=bool)
  allowed[unseen] = False
  views = []
  for v in range(V):
    idx = np.nonzero(allowed & (rng.uniform(size=N) < keep))[0].astype(np.int64)
    Y = view_basis_fp64(positions[idx], cameras[v], Kt)
    colours = 0.5 + np.einsum("mck,mk->mc", truth[idx], Y) + noise * rng.standard_normal((len(idx), 3))
    assert noise > 0 or len(idx) == 0 or (colours.min() >= 0 and colours.max() <= 1)
    weights = rng.uniform(0.1, 1.0, len(idx))
    views.append((idx, np.clip(colours, 0, 1).astype(F), weights.astype(F)))
  return Scene(positions, cameras, views, truth, np.sort(unseen))


SIZES = (1, 63, 64, 65, 257, 1000, 4099)       # lane-group, wave and block tails; a last wave that is not full
FEW_VIEWS = (1, 2, 4, 8)


def coefficient_scene(N, degree):
  """The V = 64 scene of (N, degree): colours exactly representable at the fitted degree, no noise."""
  return sphere_views(64, 64 * 100003 + 17 * N + degree, N=N, truth_degree=degree, noise=0.0)


def few_view_scene(V, N, degree):
  """Noisy degree-3 colours seen from V cameras."""
  return sphere_views(V, V * 100003 + 17 * N + degree, N=N, truth_degree=3, noise=NOISE)


# ---- normal equations, solution, objective --------------------------------------------------------------------------------------

class Equations(NamedTuple):
  G: np.ndarray              # (N, K, K)
  b: np.ndarray              # (N, 3, K)
  W: np.ndarray              # (N,)
  J0: np.ndarray             # (N,) sum w (y - 0.5)^2 over the channels: J_p(0)


def normal_equations(scene: Scene, K, view_basis=view_basis_fp64) -> Equations:
  N = len(scene.positions)
  G, b, W, J0 = np.zeros((N, K, K)), np.zeros((N, 3, K)), np.zeros(N), np.zeros(N)
  for camera, (idx, colours, weights) in zip(scene.cameras, scene.views):
    Y = view_basis(scene.positions[idx], camera, K).astype(np.float64)
    w, r = weights.astype(np.float64), colours.astype(np.float64) - 0.5
    G[idx] += w[:, None, None] * Y[:, :, None] * Y[:, None, :]
    b[idx] += w[:, None, None] * r[:, :, None] * Y[:, None, :]
    W[idx] += w
    J0[idx] += w * (r * r).sum(1)
  return Equations(G, b, W, J0)


def ridge_matrix(eq: Equations, ridge, y0=Y0):
  """G + float32(ridge) W Y0^2 diag(0, 1, ..., 1): (N, K, K)."""
  K = eq.G.shape[1]
  D = np.diag(np.r_[0.0, np.ones(K - 1)])
  return eq.G + (float(F(ridge)) * eq.W * y0 * y0)[:, None, None] * D


def solve(eq: Equations, ridge, y0=Y0):
  """(N, 3, K) fp64; zeros where W == 0."""
  s = np.zeros_like(eq.b)
  seen = eq.W > 0
  s[seen] = np.linalg.solve(ridge_matrix(eq, ridge, y0)[seen], eq.b[seen].transpose(0, 2, 1)).transpose(0, 2, 1)
  return s


def fit_fp64(scene: Scene, K, ridge):
  eq = normal_equations(scene, K)
  return solve(eq, ridge), eq


def fit_restated(scene: Scene, K, ridge):
  """What the kernels compute, to their rounding: float32 direction, basis and Y0, fp64 from there, float32 out."""
  eq = normal_equations(scene, K, view_basis_f32)
  return solve(eq, ridge, y0=float(F(0.28209479177387814))).astype(F)


def objective(scene: Scene, s, ridge):
  """J_p(s) (N,), summed over the channels, view by view in fp64."""
  s = np.asarray(s, dtype=np.float64)
  K = s.shape[2]
  J, W = np.zeros(len(s)), np.zeros(len(s))
  for camera, (idx, colours, weights) in zip(scene.cameras, scene.views):
    Y = view_basis_fp64(scene.positions[idx], camera, K)
    res = np.einsum("mck,mk->mc", s[idx], Y) - (colours.astype(np.float64) - 0.5)
    J[idx] += weights.astype(np.float64) * (res * res).sum(1)
    W[idx] += weights.astype(np.float64)
  return J + float(F(ridge)) * W * Y0 * Y0 * (s[:, :, 1:] ** 2).sum((1, 2))


def relative_excess(scene: Scene, eq: Equations, s_star, s, ridge):
  """(J_p(s) - J_p(s*)) / (J_p(s*) + 2^-24 J_p(0)) per point (0 where the point is unseen), the numerator as the quadratic
  form of s - s*."""
  d = np.asarray(s, dtype=np.float64) - s_star
  num = np.einsum("nci,nij,ncj->n", d, ridge_matrix(eq, ridge), d)
  den = objective(scene, s_star, ridge) + FLOOR * eq.J0
  return np.where(eq.W > 0, num / np.where(den > 0, den, 1.0), 0.0)


def relative_gap(scene: Scene, eq: Equations, s, s_other, ridge):
  """(J_p(s) - J_p(s_other)) / (J_p(s_other) + 2^-24 J_p(0)): how far s is ABOVE some other coefficients (negative: below)."""
  Ja, Jb = objective(scene, s, ridge), objective(scene, s_other, ridge)
  den = Jb + FLOOR * eq.J0
  return np.where(eq.W > 0, (Ja - Jb) / np.where(den > 0, den, 1.0), 0.0)


# ---- the ridge experiment -----------------------------------------------------------------------------------------------------

def ridge_experiment(ridges=(1e-3, 1e-2, 1e-1), view_counts=(4, 8, 16, 32), N=512, seed=11):
  """{ridge: [held-out colour RMSE per view count]}: degree-3 truth, fitted at degree 2 from noisy views, scored on 64
  held-out directions."""
  held = unit_vectors(np.random.default_rng(seed + 1), 64)
  table = {r: [] for r in ridges}
  for V in view_counts:
    scene = sphere_views(V, seed + V, N=N, truth_degree=3, noise=NOISE)
    eq = normal_equations(scene, 9)
    want = np.einsum("nck,hk->nhc", scene.truth, basis_fp64(held, 16))
    for r in ridges:
      got = np.einsum("nck,hk->nhc", solve(eq, r), basis_fp64(held, 9))
      seen = eq.W > 0
      table[r].append(float(np.sqrt(np.mean((got[seen] - want[seen]) ** 2))))
  return table


# ---- the host shim --------------------------------------------------------------------------------------------------------------

def row_doubles(K):
  return K * (K + 1) // 2 + 3 * K + 1


def shim_fit(shim, scene: Scene, K, ridge):
  """(sh (N, 3, K) float32, weight (N,) float32, acc (N, R) fp64) through hm_sh_fit_accumulate / hm_sh_fit_solve."""
  N = len(scene.positions)
  acc = np.zeros((N, row_doubles(K)))
  pos = np.ascontiguousarray(scene.positions, dtype=F)
  for camera, (idx, colours, weights) in zip(scene.cameras, scene.views):
    if len(idx) == 0:
      continue
    cam = np.ascontiguousarray(camera, dtype=F)
    shim.hm_sh_fit_accumulate(pos, N, np.ascontiguousarray(idx), len(idx), np.ascontiguousarray(colours),
                              np.ascontiguousarray(weights), cam, K, acc)
  sh, weight = np.empty((N, 3, K), dtype=F), np.empty(N, dtype=F)
  shim.hm_sh_fit_solve(acc, N, K, ridge, sh, weight)
  return sh, weight, acc


def weight_fp64(scene: Scene):
  """sum of the float32 weights per point in fp64, in view order."""
  W = np.zeros(len(scene.positions))
  for idx, _, weights in scene.views:
    W[idx] += weights.astype(np.float64)
  return W
