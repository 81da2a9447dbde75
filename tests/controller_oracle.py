"""Oracles for splat_trainer_amd.controller's native noise step (csrc/gsr_controller.h, csrc/controller.hip).

* Philox4x32-10 in plain integer arithmetic (numpy uint64, vectorised);
* the fp64 DEFINITION of the draw -- u = ((w >> 8) + 0.5) 2^-24 per word, Box-Muller on the pairs (0, 1) and (2, 3) --
  and of the row update: level = soft_lt(sigmoid(a), threshold / 2, margin) noise_level, offset =
  R(q / |q|) (max(exp(ls), eps) * (xi level));
* the float32 RESTATEMENT of the kernel's formula, operation by operation in numpy float32 (a fused multiply-add as the
  float32 rounding of the fp64 product and sum);
* the wrappers of the host shim;
* a scene of plain tensors that records its ``split_and_prune`` calls, a logger that records, random statistics.
"""
from types import SimpleNamespace

import numpy as np
import torch

F = np.float32
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
THRESHOLD, GATE_MARGIN, SCALE_EPS = 0.1, 16.0, 1e-4

# Measured for the restatement against the fp64 definition on 2.2 M random rows (SAMPLES below; ls in [-8, 8], a in [-12, 12], random
# unnormalised quaternions with components in [-1, 1], noise_level 100, threshold 0.1, margin 16; rows with
# s_row = level_64 max_j sigma_j < 2^-100 excluded): max |offset_f32 - offset_f64|_inf / s_row = 3.885e-05 (`python
# tests/controller_oracle.py` prints it; the excluded rows' offsets stay below 2.2e-30 = 2^-98.5).  Nearly all of it is
# the gate: its argument -(o - h) margin / h reaches -88 before the float32 gate leaves the normal range, an ulp of such
# an argument is 7.6e-6, and the gate's relative error is the argument's absolute one; times |xi| up to 5.
RESTATEMENT = 3.9e-5
MARGIN = 4.0            # what the project gives device intrinsics over the host's libm (filter3d_oracle.py)


# ---- Philox --------------------------------------------------------------------------------------------------------------

def philox4x32(counter, key):
  """counter (..., 4), key (..., 2) of integers below 2^32 -> (..., 4) uint32."""
  counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
  c0, c1, c2, c3 = (counter[..., j].copy() for j in range(4))
  k0, k1 = key[..., 0].copy(), key[..., 1].copy()
  for _ in range(10):
    p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
    k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
  return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(index, seed, step):
  """The four words of the rows ``index`` (any integers below 2^64, broadcast against seed and step): (..., 4) uint32."""
  index, seed, step = np.broadcast_arrays(*(np.asarray(t, dtype=np.uint64) for t in (index, seed, step)))
  lo, hi = (lambda t: t & MASK), (lambda t: t >> np.uint64(32))
  return philox4x32(np.stack([lo(index), hi(index), lo(step), hi(step)], axis=-1), np.stack([lo(seed), hi(seed)], axis=-1))


# ---- fp64 definition -----------------------------------------------------------------------------------------------------

def uniforms_fp64(w):
  return ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals_fp64(w):
  """(..., 4) words -> (..., 4) normals; xi is [..., :3]."""
  u = uniforms_fp64(w)
  r01, r23 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
  t01, t23 = 2.0 * np.pi * u[..., 1], 2.0 * np.pi * u[..., 3]
  return np.stack([r01 * np.cos(t01), r01 * np.sin(t01), r23 * np.cos(t23), r23 * np.sin(t23)], axis=-1)


def _sigmoid64(x):
  e = np.exp(-np.abs(x))
  return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def soft_lt_fp64(o, h, margin):
  """soft_lt(o, h, margin) = 1 - sigmoid((o - h) margin / h) of util/misc.py:21-37, as one sigmoid."""
  return _sigmoid64(-(np.asarray(o, dtype=np.float64) - h) * margin / h)


def gate_fp64(a, threshold=THRESHOLD, margin=GATE_MARGIN):
  """soft_lt(sigmoid(a), threshold / 2, margin) on float32 inputs."""
  return soft_lt_fp64(_sigmoid64(np.asarray(a, dtype=F).astype(np.float64)), 0.5 * float(F(threshold)), float(F(margin)))


def rotmat_fp64(q):
  """Rotation matrices (..., 3, 3) of quaternions (..., 4) xyzw, normalised here."""
  q = np.asarray(q, dtype=np.float64)
  x, y, z, w = np.moveaxis(q / np.linalg.norm(q, axis=-1, keepdims=True), -1, 0)
  return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                   np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                   np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def offsets_fp64(ls, q, a, index, seed, step, noise_level, threshold=THRESHOLD, margin=GATE_MARGIN, eps=SCALE_EPS):
  """(offset (N, 3), s_row (N,)) of the float32 rows, every row taken as eligible."""
  sigma = np.maximum(np.exp(np.asarray(ls, dtype=F).astype(np.float64)), float(F(eps)))
  level = gate_fp64(a, threshold, margin) * float(F(noise_level))
  xi = normals_fp64(words(index, seed, step))[..., :3]
  v = sigma * (xi * level[:, None])
  return np.einsum("nij,nj->ni", rotmat_fp64(np.asarray(q, dtype=F)), v), level * sigma.max(axis=1)


# ---- float32 restatement of csrc/gsr_controller.h -------------------------------------------------------------------------

def _fma(a, b, c):
  return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, dtype=F).astype(np.float64)).astype(F)


def normals_f32(w):
  w = np.asarray(w, dtype=np.uint32)
  k = w >> np.uint32(8)
  out = []
  for p in (0, 2):
    ka, kb = k[..., p], k[..., p + 1]
    lo = np.log(((ka & np.uint32(0x7FFFFF)).astype(F) + F(0.5)) * F(2.0 ** -24))
    hi = np.log1p(-(((np.uint32(0x1000000) - (ka | np.uint32(0x800000))).astype(F) - F(0.5)) * F(2.0 ** -24)))
    r = np.sqrt(F(-2) * np.where(ka < 0x800000, lo, hi))
    frac = ((kb & np.uint32(0x3FFFFF)).astype(F) + F(0.5)) * F(2.0 ** -24)
    theta = _fma(frac, np.full_like(frac, F(6.2831855)), frac * F(-1.7484555e-7))
    ct, st = np.cos(theta), np.sin(theta)
    quad = kb >> np.uint32(22)
    cq, sq = np.where(quad & 1, -st, ct), np.where(quad & 1, ct, st)
    c, s = np.where(quad & 2, -cq, cq), np.where(quad & 2, -sq, sq)
    out += [r * c, r * s]
  out = np.stack(out, axis=-1)
  assert out.dtype == F
  return out


def _sigmoid32(x):
  e = np.exp(-np.abs(x))
  r = F(1) / (F(1) + e)
  return np.where(x >= 0, r, e * r).astype(F)


def level_f32(a, noise_level, threshold=THRESHOLD, margin=GATE_MARGIN):
  o, h = _sigmoid32(np.asarray(a, dtype=F)), F(0.5) * F(threshold)
  with np.errstate(under="ignore"):
    return _sigmoid32(-(((o - h) * F(margin)) / h)) * F(noise_level)


def offsets_f32(ls, q, a, index, seed, step, noise_level, threshold=THRESHOLD, margin=GATE_MARGIN, eps=SCALE_EPS):
  """(offset (N, 3) float32, written (N,) bool): a row with level max sigma == 0 in float32 has no offset."""
  ls, q = np.asarray(ls, dtype=F), np.asarray(q, dtype=F)
  with np.errstate(under="ignore"):
    sigma = np.maximum(np.exp(ls), F(eps))
    level = level_f32(a, noise_level, threshold, margin)
    written = level * sigma.max(axis=1) != 0
    xi = normals_f32(words(index, seed, step))[..., :3]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    norm = np.sqrt(_fma(x, x, _fma(y, y, _fma(z, z, w * w))))
    inv = F(1) / np.maximum(norm, F(1e-12))
    x, y, z, w = x * inv, y * inv, z * inv, w * inv
    one, two = np.ones_like(x), F(2)
    R = [[_fma(-two * one, _fma(y, y, z * z), one), two * _fma(x, y, -(w * z)), two * _fma(x, z, w * y)],
         [two * _fma(x, y, w * z), _fma(-two * one, _fma(x, x, z * z), one), two * _fma(y, z, -(w * x))],
         [two * _fma(x, z, -(w * y)), two * _fma(y, z, w * x), _fma(-two * one, _fma(x, x, y * y), one)]]
    v = sigma * (xi * level[:, None])
    off = np.stack([_fma(R[j][0], v[:, 0], _fma(R[j][1], v[:, 1], R[j][2] * v[:, 2])) for j in range(3)], axis=1)
  assert off.dtype == F
  return np.where(written[:, None], off, F(0)), written


def random_rows(n, seed):
  """(ls (n, 3), q (n, 4), a (n,)) float32: ls in [-8, 8], a in [-12, 12], unnormalised quaternions.  Half of the logits
  are drawn where the gate is not negligible (opacity below the threshold); the first rows are the corners."""
  rng = np.random.default_rng(seed)
  ls = rng.uniform(-8, 8, (n, 3))
  a = rng.uniform(-12, 12, n)
  low = rng.random(n) < 0.5
  a[low] = rng.uniform(-12, -1.5, int(low.sum()))
  q = rng.uniform(-1, 1, (n, 4))
  corners = [((-8, -8, -8), -12, (0, 0, 0, 1)), ((8, 8, 8), -12, (1, 0, 0, 0)), ((-8, 8, 0.5), 12, (0.5, 0.5, 0.5, 0.5)),
             ((-12, -12, -12), -3, (0, 0, 0, 2)), ((0, 0, 0), -2.2, (0.3, -0.2, 0.1, 1e-3)), ((1, 2, 3), 0, (0, 1, 0, 1))]
  for i, (ls_, a_, q_) in enumerate(corners[:n]):
    ls[i], a[i], q[i] = ls_, a_, q_
  return ls.astype(F), q.astype(F), a.astype(F)


def row_error(got, want, s_row):
  """max over the rows with s_row >= 2^-100 of |got - want|_inf / s_row, and the largest |got|_inf among the others."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  big = s_row >= 2.0 ** -100
  err = np.abs(got - want).max(axis=1)
  worst = float(np.max(err[big] / s_row[big])) if big.any() else 0.0
  small = float(np.abs(got[~big]).max()) if (~big).any() else 0.0
  return worst, small


# ---- host shim -----------------------------------------------------------------------------------------------------------

def shim_philox(lib, counter, key):
  counter, key = np.ascontiguousarray(counter, dtype=np.uint32), np.ascontiguousarray(key, dtype=np.uint32)
  out = np.empty(4, dtype=np.uint32)
  lib.hm_philox4x32(counter, key, out)
  return out


def shim_draws(lib, first, n, seed, step):
  w, z = np.empty((n, 4), dtype=np.uint32), np.empty((n, 3), dtype=F)
  lib.hm_mcmc_draws(int(first), n, int(seed), int(step), w, z)
  return w, z


def shim_level(lib, a, noise_level, threshold=THRESHOLD, margin=GATE_MARGIN):
  a = np.ascontiguousarray(a, dtype=F)
  out = np.empty_like(a)
  lib.hm_mcmc_level(a, a.shape[0], float(threshold), float(margin), float(noise_level), out)
  return out


def shim_noise(lib, position, ls, q, a, views, min_views, noise_level, seed, step, threshold=THRESHOLD,
               margin=GATE_MARGIN, eps=SCALE_EPS):
  position = np.array(position, dtype=F, order="C")
  ls, q, a = (np.ascontiguousarray(t, dtype=F) for t in (ls, q, a))
  views = np.ascontiguousarray(views, dtype=np.int16)
  lib.hm_mcmc_noise(position, ls, q, a, views, a.shape[0], int(min_views), float(threshold),
                    float(margin), float(noise_level), float(eps), int(seed), int(step))
  return position


# ---- controller logic: a scene of plain tensors -------------------------------------------------------------------------------

class FakeScene:
  """A scene of plain CPU tensors: what a controller needs, with ``split_and_prune`` recorded."""

  def __init__(self, n, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    self.points = SimpleNamespace(position=torch.randn(n, 3, generator=g), log_scaling=torch.randn(n, 3, generator=g),
                                  rotation=torch.randn(n, 4, generator=g), alpha_logit=torch.randn(n, 1, generator=g) * 3)
    for k, v in vars(self.points).items():
      setattr(self.points, k, v.to(device))
    self.calls = []

  @property
  def num_points(self):
    return self.points.position.shape[0]

  @property
  def device(self):
    return self.points.position.device

  def split_and_prune(self, keep_mask, split_idx, **kw):
    self.calls.append(dict(keep_mask=keep_mask.clone(), split_idx=split_idx.clone(), kw=kw))
    for k, v in vars(self.points).items():
      setattr(self.points, k, torch.cat([v[keep_mask], v[split_idx].repeat_interleave(2, dim=0)]))


class FakeLogger:
  def __init__(self):
    self.values, self.histograms = [], []

  def log_values(self, name, values):
    self.values.append((name, dict(values)))

  def log_histogram(self, name, t):
    self.histograms.append(name)


def fill_state(state, seed: int):
  """Random statistics (drawn on the CPU, whatever the state's device)."""
  g = torch.Generator().manual_seed(seed)
  n = state.prune_cost.shape[0]
  state.prune_cost.copy_(torch.rand(n, generator=g))
  state.split_score.copy_(torch.rand(n, generator=g))
  state.max_scale_px.copy_(torch.rand(n, generator=g) * 250)
  state.points_in_view.copy_(torch.randint(0, 12, (n,), generator=g).to(torch.int16))
  state.visibility.copy_(torch.rand(n, generator=g))
  return state


def measure_restatement(n, rows_seed, first, seed, step, noise_level=100.0):
  """(restatement error, largest |offset| among the rows below 2^-100, rows above) of ``n`` random rows."""
  ls, q, a = random_rows(n, seed=rows_seed)
  idx = np.arange(n, dtype=np.uint64) + np.uint64(first)
  want, s_row = offsets_fp64(ls, q, a, idx, seed, step, noise_level)
  got, _ = offsets_f32(ls, q, a, idx, seed, step, noise_level)
  return row_error(got, want, s_row) + (int((s_row >= 2.0 ** -100).sum()),)


# the samples RESTATEMENT is the maximum over: 8 x 250 000 rows and the 200 000 rows tests/test_controller_host.py checks
SAMPLES = [(250_000, 100 + c, c * 250_000, 7, 3) for c in range(8)] + [(200_000, 1, 0, 17, 23)]

if __name__ == "__main__":
  worst = 0.0
  for sample in SAMPLES:
    e, small, above = measure_restatement(*sample)
    worst = max(worst, e)
    print(f"rows {sample}: {above} rows above 2^-100, restatement {e:.3e}, largest |offset| below {small:.3e}")
  print(f"RESTATEMENT over {sum(s[0] for s in SAMPLES)} rows: {worst:.3e}")
