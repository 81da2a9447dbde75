"""Oracles for splat_trainer_amd.filter3d (Mip-Splatting's 3-D smoothing filter).  The reference has no such filter, so
there is no golden file from it: the oracle is this build's own, as for the rasteriser.

* the fp64 definitions in their PLAIN form -- sigma' = sqrt(sigma^2 + c), opacity' = opacity prod sigma / sigma' through
  sigmoid and logit -- and their gradients by torch autograd on that form;
* the float32 RESTATEMENT of the stable form the kernels implement (csrc/gsr_filter3d.h), operation by operation in numpy
  float32, and the naive float32 form ``logit(sigmoid(a) coef)`` that must not be used;
* the fp64 lower / upper bounds of the sampling rate: the maximum of f / d over the cameras that pass every inequality
  of the sampling test with slack above E (L) and above -E (U), E twice the modelled float32 rounding of both sides;
* the scenes the checks use and the wrappers of the host shim.
"""

import numpy as np
import torch

import visibility_oracle as vo

U24 = 2.0 ** -24
STRENGTH = 0.2
# measured for the restatement against the plain fp64 form on 2 M random rows (ls in [-8, 8], a in [-12, 12], c in
# [1e-14, 1e2]): outputs within 5.6e-7 of max(1, |value|), the two derivatives of a' within 5.7e-7 relative
RESTATEMENT_OUT, RESTATEMENT_GRAD, MARGIN = 5.6e-7, 5.7e-7, 4.0


# ---- smoothing: plain fp64 ---------------------------------------------------------------------------------------------

def variance_fp64(rate, strength=STRENGTH):
  """c = float32(strength) / rate^2 in fp64 on the float32 rates; 0 where the rate is not > 0."""
  r = np.asarray(rate, dtype=np.float64)
  s = float(np.float32(strength))
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.where(r > 0, s / (r * r), 0.0)


def smooth_plain(ls: torch.Tensor, a: torch.Tensor, c: torch.Tensor):
  """The definition, in the dtype of its arguments (fp64 here): ls (N, 3), a (N,), c (N,) -> ls' (N, 3), a' (N,)."""
  var = torch.exp(2 * ls)
  new_var = var + c[:, None]
  coef = torch.sqrt(var / new_var).prod(dim=1)
  return 0.5 * torch.log(new_var), torch.logit(torch.sigmoid(a) * coef)


def smooth_fp64(ls, a, c):
  out_ls, out_a = smooth_plain(*(torch.as_tensor(np.asarray(t, dtype=np.float64)) for t in (ls, a, c)))
  return out_ls.numpy(), out_a.numpy()


def partials_fp64(ls, a, c):
  """Autograd on the plain form: d ls'_j / d ls_j (N, 3), d a' / d a (N,), d a' / d ls_j (N, 3) and ``floor`` (N,), the
  size below which the last is the oracle's own rounding.  (Rows are independent and ls'_j depends on ls_j alone, so the
  gradients of the two sums are these partials.)  The plain form reaches d a' / d ls_j = (u_j / (1 + u_j)) / (1 - q) as
  (1 - var / (var + c)) / (1 - q), exact to 2^-52 / (1 - q) only; ``floor`` = 2^-26 / (1 - q) keeps that error 2^-26
  of the scale an entry is compared on (error_on)."""
  ls_t = torch.as_tensor(np.asarray(ls, dtype=np.float64)).requires_grad_(True)
  a_t = torch.as_tensor(np.asarray(a, dtype=np.float64)).requires_grad_(True)
  out_ls, out_a = smooth_plain(ls_t, a_t, torch.as_tensor(np.asarray(c, dtype=np.float64)))
  dls_dls, = torch.autograd.grad(out_ls.sum(), ls_t, retain_graph=True)
  da_da, da_dls = torch.autograd.grad(out_a.sum(), (a_t, ls_t))
  one_minus_q = torch.sigmoid(-a_t.detach()) / da_da                    # d a' / d a = sigmoid(-a) / (1 - q)
  return dls_dls.numpy(), da_da.numpy(), da_dls.numpy(), (2.0 ** -26 / one_minus_q).numpy()


def backward_fp64(ls, a, c, g_ls, g_a):
  """(d_ls, d_a, scale_ls): the vector-Jacobian product of the plain form, and per entry of d_ls the scale a rounding
  error of it is relative to: the sum of the magnitudes of its two terms (they can cancel), the second not below
  |g_a| floor."""
  dls_dls, da_da, da_dls, floor = partials_fp64(ls, a, c)
  g_ls, g_a = np.asarray(g_ls, dtype=np.float64), np.asarray(g_a, dtype=np.float64)
  t1, t2 = g_ls * dls_dls, g_a[:, None] * da_dls
  return t1 + t2, g_a * da_da, np.abs(t1) + np.maximum(np.abs(t2), np.abs(g_a * floor)[:, None])


# ---- smoothing: the float32 restatement of csrc/gsr_filter3d.h --------------------------------------------------------

F = np.float32


def variance_f32(rate, strength=STRENGTH):
  r = np.asarray(rate, dtype=F)
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.where(r > 0, F(strength) / (r * r), F(0)).astype(F)


def _terms_f32(ls, a, c):
  ls, a, c = np.asarray(ls, dtype=F), np.asarray(a, dtype=F), np.asarray(c, dtype=F)
  u = c[:, None] * np.exp(F(-2) * ls)
  l = np.log1p(u)
  lc = F(-0.5) * ((l[:, 0] + l[:, 1]) + l[:, 2])
  e = np.exp(-np.abs(a))
  r = F(1) / (F(1) + e)
  big, small = r, e * r
  sp, sn = np.where(a >= 0, big, small), np.where(a >= 0, small, big)
  log_sp = np.minimum(a, F(0)) - np.log1p(e)
  D = sn + sp * -np.expm1(lc)
  assert all(t.dtype == F for t in (u, l, lc, sp, sn, log_sp, D))
  return u, l, lc, sp, sn, log_sp, D


def smooth_f32(ls, a, c):
  """Rows with c == 0 are copied, as the kernels do."""
  ls, a, c = np.asarray(ls, dtype=F), np.asarray(a, dtype=F), np.asarray(c, dtype=F)
  u, l, lc, sp, sn, log_sp, D = _terms_f32(ls, a, c)
  out_ls = ls + F(0.5) * l
  out_a = (log_sp + lc) - np.log(D)
  keep = c == 0
  return np.where(keep[:, None], ls, out_ls).astype(F), np.where(keep, a, out_a).astype(F)


def partials_f32(ls, a, c):
  u, l, lc, sp, sn, log_sp, D = _terms_f32(ls, a, c)
  k = F(1) + u
  return F(1) / k, sn / D, (u / k) / D[:, None]


def backward_f32(ls, a, c, g_ls, g_a):
  g_ls, g_a, c = np.asarray(g_ls, dtype=F), np.asarray(g_a, dtype=F), np.asarray(c, dtype=F)
  u, l, lc, sp, sn, log_sp, D = _terms_f32(ls, a, c)
  k = F(1) + u
  d_ls = g_ls / k + g_a[:, None] * ((u / k) / D[:, None])
  d_a = g_a * (sn / D)
  keep = c == 0
  return np.where(keep[:, None], g_ls, d_ls).astype(F), np.where(keep, g_a, d_a).astype(F)


def naive_f32(ls, a, c):
  """a' as logit(sigmoid(a) coef) in float32: 1 - q cancels for q near 1."""
  ls, a, c = np.asarray(ls, dtype=F), np.asarray(a, dtype=F), np.asarray(c, dtype=F)
  var = np.exp(F(2) * ls)
  coef = np.sqrt(var / (var + c[:, None])).prod(axis=1, dtype=F)
  q = (F(1) / (F(1) + np.exp(-a))) * coef
  with np.errstate(divide="ignore", invalid="ignore"):
    return np.log(q / (F(1) - q))


def out_error(got, want):
  """max |got - want| / max(1, |want|)."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if want.size else 0.0


def error_on(got, want, scale=None):
  """max |got - want| / scale, scale = |want| by default; an entry with scale 0 must be exact."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  scale = np.abs(want) if scale is None else np.broadcast_to(np.asarray(scale, dtype=np.float64), want.shape)
  err = np.abs(got - want)
  ok = scale > 0
  assert np.all(err[~ok] == 0), "an entry the oracle has as exactly 0 is not 0"
  return float(np.max(err[ok] / scale[ok])) if ok.any() else 0.0


def partial_errors(got, want):
  """Errors of (d ls' / d ls, d a' / d a, d a' / d ls) against partials_fp64's four: relative, the last on
  max(|want|, floor)."""
  dls_dls, da_da, da_dls, floor = want
  return (error_on(got[0], dls_dls), error_on(got[1], da_da),
          error_on(got[2], da_dls, np.maximum(np.abs(da_dls), floor[:, None])))


def random_rows(n, seed, corners=True):
  """(ls (n, 3), a (n,), rate (n,)) float32 over the ranges above -- the rate chosen so that c = 0.2 / rate^2 is
  log-uniform in [1e-14, 1e2] -- with, when ``corners``, the first rows replaced by: c = 0 (rate 0); u >> 1 (ls = -8,
  c = 1e2); a = +-12; ls = +-8 (the scene's clamp); and all of these combined."""
  rng = np.random.default_rng(seed)
  ls = rng.uniform(-8, 8, (n, 3))
  a = rng.uniform(-12, 12, n)
  c = 10.0 ** rng.uniform(-14, 2, n)
  if corners:
    rows = []
    for c_ in (0.0, 1e-14, 1e2):
      for a_ in (-12.0, 12.0, 0.3):
        for ls_ in ((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0), (-8.0, 8.0, 0.5)):
          rows.append((ls_, a_, c_))
    rows = rows[:n] if n < 8 else rows[:max(8, min(len(rows), n // 2))]
    for i, (ls_, a_, c_) in enumerate(rows[:n]):
      ls[i], a[i], c[i] = ls_, a_, c_
  with np.errstate(divide="ignore"):
    rate = np.where(c > 0, np.sqrt(float(F(STRENGTH)) / np.where(c > 0, c, 1.0)), 0.0)
  return ls.astype(F), a.astype(F), rate.astype(F)


# ---- sampling rate: fp64 bounds ------------------------------------------------------------------------------------------

def rate_bounds_fp64(points, records, focal, margin):
  """Per point, from the float32 points, records (V, 16), focal (V,) and float32(margin), all taken to fp64:
  ``L``, ``U`` (N,) as in the module docstring and ``eps_L``, ``eps_U`` = 2^-22 + E_d / d of the pair that gives the bound;
  ``band`` = the number of (camera, point) pairs that pass with slack above -E but not above E.

  E per inequality lhs - rhs > 0 (>= for the two lower image bounds): a row h_r is three nested fmaf, three roundings of
  at most 2^-24 of the sum of the magnitudes of its terms s_r; a right-hand side k d has the rounding of the factor k
  (-m w or fmaf(m, w, w)), the rounding of the product and the row's error times |k|: at most 5 2^-24 |k| s_2.  Twice the
  two: E = 2^-24 (6 s_r + 10 |k| s_2); for d against near and far, which are exact, E_d = 2^-24 6 s_2."""
  p = np.asarray(points, dtype=np.float64)
  m = float(F(margin))
  N = p.shape[0]
  L, U = np.zeros(N), np.zeros(N)
  eps_L, eps_U = np.full(N, 2.0 ** -22), np.full(N, 2.0 ** -22)
  band = 0
  for c in range(records.shape[0]):
    r = records[c].astype(np.float64)
    M = r[:12].reshape(3, 4)
    w, h, near, far = r[12:]
    f = float(focal[c])
    terms = M[:, None, :3] * p[None, :, :]
    hr = terms.sum(-1) + M[:, 3:4]
    sr = np.abs(terms).sum(-1) + np.abs(M[:, 3:4])
    (h0, h1, d), (s0, s1, s2) = hr, sr
    slack_E = []
    for hv, sv, size in ((h0, s0, w), (h1, s1, h)):
      lo, hi = -m * size, size + m * size
      slack_E.append((hv - lo * d, U24 * (6 * sv + 10 * abs(lo) * s2)))
      slack_E.append((hi * d - hv, U24 * (6 * sv + 10 * abs(hi) * s2)))
    E_d = U24 * 6 * s2
    slack_E += [(d - near, E_d), (far - d, E_d)]
    with np.errstate(invalid="ignore", divide="ignore"):
      strict = np.all([s > E for s, E in slack_E], axis=0)
      loose = np.all([s > -E for s, E in slack_E], axis=0) & (d > 0)
      q = f / d
      e = 2.0 ** -22 + E_d / d
    band += int((loose & ~strict).sum())
    up = strict & (q > L)
    L[up], eps_L[up] = q[up], e[up]
    up = loose & (q > U)
    U[up], eps_U[up] = q[up], e[up]
  return dict(L=L, U=U, eps_L=eps_L, eps_U=eps_U, band=band)


def inside_sandwich(rate, b):
  """Per point: L (1 - eps_L) <= rate <= U (1 + eps_U)."""
  rate = np.asarray(rate, dtype=np.float64)
  return (rate >= b["L"] * (1 - b["eps_L"])) & (rate <= b["U"] * (1 + b["eps_U"]))


# ---- scenes ----------------------------------------------------------------------------------------------------------------

SIZE = (160, 120)


def ring_cameras(V, seed=0, far=9.0):
  """visibility_oracle.ring_cameras at 160 x 120 with fx != fy (fy = fx times a factor in [0.8, 1.25], so that
  max(fx, fy) is fx for some cameras and fy for others) and a far plane that cuts the far side of the cloud."""
  ctw, intr, sizes, ranges = vo.ring_cameras(V, radius=6.0, seed=seed, size=SIZE, focal=(100.0, 175.0), near=0.1, far=far)
  rng = np.random.default_rng(seed + 1000)
  intr = intr.copy()
  intr[:, 1] = (intr[:, 1] * rng.uniform(0.8, 1.25, V)).astype(F)
  return ctw, intr, sizes, ranges


def ring_points(n, seed=0):
  """A cloud wide enough that, with 64 cameras on the ring, 10-30 % of it is sampled by no camera and part of it lies
  behind cameras."""
  return vo.ring_points(n, seed=seed, sigma=(3.0, 3.9, 3.0))


def far_from_every_bound(n, seed=0):
  """Points for the ring cameras on which no comparison is close: half in a ball of radius 0.3 about the origin (near the
  image centre of every camera, at depth about 6 between near 0.1 and far 9), half 40 to 60 units above the ring
  (outside every image by many image heights)."""
  rng = np.random.default_rng(seed)
  p = rng.uniform(-0.3, 0.3, (n, 3))
  p[n // 2:, 1] += rng.uniform(40, 60, n - n // 2) * rng.choice([-1.0, 1.0], n - n // 2)
  return p.astype(F)


def focal_of(intr):
  return np.maximum(intr[:, 0], intr[:, 1]).astype(F)


# ---- host shim -----------------------------------------------------------------------------------------------------------

def shim_sampling_rate(lib, points, records, focal, margin):
  points, records, focal = (np.ascontiguousarray(t, dtype=F) for t in (points, records, focal))
  rate = np.empty(points.shape[0], dtype=F)
  lib.hm_sampling_rate(points, points.shape[0], records, focal, records.shape[0], float(margin), rate)
  return rate


def shim_forward(lib, ls, a, rate, strength=STRENGTH):
  ls, a, rate = (np.ascontiguousarray(t, dtype=F) for t in (ls, a, rate))
  out_ls, out_a = np.empty_like(ls), np.empty_like(a)
  lib.hm_filter3d_forward(ls, a, rate, a.shape[0], float(strength), out_ls, out_a)
  return out_ls, out_a


def shim_backward(lib, ls, a, rate, g_ls, g_a, strength=STRENGTH):
  ls, a, rate, g_ls, g_a = (np.ascontiguousarray(t, dtype=F) for t in (ls, a, rate, g_ls, g_a))
  d_ls, d_a = np.empty_like(ls), np.empty_like(a)
  lib.hm_filter3d_backward(ls, a, rate, a.shape[0], float(strength), g_ls, g_a, d_ls, d_a)
  return d_ls, d_a
