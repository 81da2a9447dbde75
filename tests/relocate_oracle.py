"""Oracles for the MCMC relocation move (csrc/gsr_relocate.h, csrc/relocate.hip).

* the weighted draw in Python integers: the Philox words of ``controller_oracle`` (pinned there to the published
  vectors) at the tagged counter, ``t = (r S) >> 64`` and the smallest ``i`` with ``P_i > t``;
* the opacity weight and the opacity / scale correction in mpmath at 60 digits, the correction in the DOUBLE-sum form of
  Eq. 9 of Kheradmand et al. 2024 (the kernel uses the collapsed single sum);
* float32 ulps of an oracle value; the wrappers of the host shim.
"""
import mpmath
import numpy as np

import controller_oracle as co

mpmath.mp.dps = 60
BLOCK = 256                      # rows per block of the prefix (GSR_RELOC_BLOCK)
MAX_COPIES = 51
F = np.float32
_M32 = 0xFFFFFFFF


# ---- the draw ------------------------------------------------------------------------------------------------------------
def draw_words(k, seed, step, domain):
  """(len(k), 4) uint32: the words of the draws ``k`` at (seed, step) in ``domain``."""
  k = np.asarray(k, dtype=np.uint64).reshape(-1)
  seed, step, domain = int(seed), int(step), int(domain)
  counter = np.empty((k.shape[0], 4), dtype=np.uint64)
  counter[:, 0], counter[:, 1] = k & np.uint64(_M32), k >> np.uint64(32)
  counter[:, 2], counter[:, 3] = step & _M32, ((step >> 32) & 0x00FFFFFF) | (domain << 24)
  key = np.array([seed & _M32, seed >> 32], dtype=np.uint64)
  return co.philox4x32(counter, np.broadcast_to(key, (k.shape[0], 2)))


def targets(n, seed, step, domain, S):
  """[t_0 .. t_{n-1}] as Python ints."""
  w = draw_words(np.arange(n, dtype=np.uint64), seed, step, domain)
  return [(((int(a) << 32) | int(b)) * int(S)) >> 64 for a, b in zip(w[:, 0], w[:, 1])]


def draws(weights, n, seed, step, domain):
  """(sources (n,) int32, counts (N,) int32, S): the definition, entry by entry."""
  weights = np.asarray(weights, dtype=np.uint32)
  N = weights.shape[0]
  P = np.cumsum(weights.astype(np.uint64), dtype=np.uint64)
  S = int(P[-1]) if N else 0
  if S == 0:
    return np.full(n, -1, dtype=np.int32), np.zeros(N, dtype=np.int32), 0
  t = np.array(targets(n, seed, step, domain, S), dtype=np.uint64)
  sources = np.searchsorted(P, t, side="right").astype(np.int32)          # the smallest i with P_i > t
  assert n == 0 or (sources.max() < N and np.all(weights[sources] > 0))
  return sources, np.bincount(sources, minlength=N).astype(np.int32), S


# ---- weight and correction, 60 digits ----------------------------------------------------------------------------------------
def _sigmoid(a):
  return 1 / (1 + mpmath.exp(-mpmath.mpf(float(a))))


def weight(a, alive=True):
  """max(1, floor(2^24 sigmoid(a))) of a float32 logit, 0 for a dead row."""
  return max(1, int(mpmath.floor(_sigmoid(F(a)) * 2 ** 24))) if alive else 0


def corrected_opacity(a, copies):
  """(o', n) of a source with ``copies`` >= 1 copies."""
  n = min(int(copies) + 1, MAX_COPIES)
  return 1 - (1 - _sigmoid(F(a))) ** (mpmath.mpf(1) / n), n


def denominator_double_sum(op, n):
  """Eq. 9: sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1)."""
  return mpmath.fsum(mpmath.binomial(i - 1, k) * (-1) ** k * op ** (k + 1) / mpmath.sqrt(k + 1)
                     for i in range(1, n + 1) for k in range(i))


def denominator_single_sum(op, n):
  """The same by sum_i C(i-1, k) = C(n, k+1)."""
  return mpmath.fsum(mpmath.binomial(n, k + 1) * (-1) ** k * op ** (k + 1) / mpmath.sqrt(k + 1) for k in range(n))


def rescale(a, copies, log_scaling, o_floor):
  """(new logit, [new log-scales]) as mpf, of a float32 row with ``copies`` >= 1; o_floor is taken as a float32."""
  op, n = corrected_opacity(a, copies)
  coeff = _sigmoid(F(a)) / denominator_double_sum(op, n)
  p = min(max(op, mpmath.mpf(float(F(o_floor)))), 1 - mpmath.mpf(2) ** -24)
  return mpmath.log(p / (1 - p)), [mpmath.mpf(float(F(v))) + mpmath.log(coeff) for v in log_scaling]


def ulps(got, want):
  """|got - want| in float32 ulps of ``want`` (an mpf)."""
  unit = float(np.spacing(np.abs(F(float(want)))))
  return float(abs(mpmath.mpf(float(got)) - want) / unit)


# ---- host shim -----------------------------------------------------------------------------------------------------------
def shim_words(lib, k, seed, step, domain):
  out = np.empty(4, dtype=np.uint32)
  lib.hm_reloc_words(int(k), int(seed), int(step), int(domain), out)
  return out


def shim_draws(lib, weights, n, seed, step, domain):
  weights = np.ascontiguousarray(weights, dtype=np.uint32)
  N = weights.shape[0]
  sources, counts = np.full(max(n, 1), -7, dtype=np.int32), np.full(max(N, 1), -7, dtype=np.int32)
  total, ws = np.full(1, 99, dtype=np.uint64), np.empty(max((N + BLOCK - 1) // BLOCK, 1), dtype=np.uint64)
  rc = lib.hm_weighted_draws(weights if N else None, N, n, int(seed), int(step), int(domain), sources, counts, total, ws,
                             ws.nbytes)
  assert rc == 0, rc
  return sources[:n], counts[:N], int(total[0])


def shim_weights(lib, a, alive=None):
  a = np.ascontiguousarray(a, dtype=F)
  out = np.empty(a.shape[0], dtype=np.uint32)
  assert lib.hm_relocate_weights(a, None if alive is None else np.ascontiguousarray(alive, dtype=np.uint8), a.shape[0], out) == 0
  return out


def shim_rescale(lib, a, log_scaling, counts, o_floor):
  a, ls = np.array(a, dtype=F, order="C"), np.array(log_scaling, dtype=F, order="C")
  assert lib.hm_relocate_rescale(a, ls, np.ascontiguousarray(counts, dtype=np.int32), a.shape[0], float(o_floor)) == 0
  return a, ls


# ---- the cases both suites run ---------------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 257, 1025, 4099]
DRAWS = [0, 1, 64, 1000]
SEED, STEP = 2 ** 63 + 77, 2 ** 40 + 5          # both words of the key and of the step are in use


def weight_patterns(N):
  """{name: weights (N,) uint32}."""
  rng = np.random.default_rng(N)
  out = {"equal": np.full(N, 5, dtype=np.uint32), "binary": rng.integers(0, 2, N).astype(np.uint32),
         "random": rng.integers(0, 2 ** 24 + 1, N).astype(np.uint32)}
  out["binary"][rng.integers(0, N)] = 1                                    # never all zero
  for name, at in (("first", 0), ("middle", N // 2), ("last", N - 1)):
    out[name] = np.zeros(N, dtype=np.uint32)
    out[name][at] = 3
  runs = rng.integers(1, 2 ** 24 + 1, N).astype(np.uint32)                 # zeros across the boundaries of the 256-row blocks
  for b in range(BLOCK, N + BLOCK, BLOCK):
    runs[max(b - 40, 0):b + 300 * ((b // BLOCK) % 2) + 7] = 0
  if not runs.any():
    runs[N - 1] = 9
  out["zero_runs"] = runs
  if N == 4099:
    out["full"] = np.full(N, 2 ** 24, dtype=np.uint32)                     # S = 4099 * 2^24 > 2^32
  return out


LOGITS = np.concatenate([np.linspace(-12.0, 16.0, 29), [-6.0, -2.0, 0.0, 2.0, 4.6, 8.0]]).astype(F)
COUNTS = [0, 1, 2, 7, 50, 51, 1000]
LOG_SCALES = np.array([-5.0, 0.75, 3.0], dtype=F)
O_FLOOR = 0.1
ULP_BOUND = 2.0


def rescale_grid():
  """(a (R,), ls (R, 3), counts (R,)): every logit of the grid with every count."""
  a = np.repeat(LOGITS, len(COUNTS))
  counts = np.tile(np.array(COUNTS, dtype=np.int32), len(LOGITS))
  return a, np.tile(LOG_SCALES, (a.shape[0], 1)), counts


_GRID_ORACLE = {}


def rescale_grid_oracle():
  """[(logit, [ls_0, ls_1, ls_2]) as mpf, or None for a count of 0] per row of rescale_grid(); computed once."""
  if not _GRID_ORACLE:
    a, ls, counts = rescale_grid()
    memo = {}
    rows = []
    for x, c in zip(a, counts):
      key = (float(x), min(int(c), MAX_COPIES - 1))
      if c > 0 and key not in memo:
        memo[key] = rescale(x, c, LOG_SCALES, O_FLOOR)
      rows.append(memo[key] if c > 0 else None)
    _GRID_ORACLE["rows"] = rows
  return _GRID_ORACLE["rows"]


def worst_ulps(a_new, ls_new):
  """(worst logit ulps, worst log-scale ulps) of a rescaled grid against the oracle."""
  worst_a = worst_ls = 0.0
  for r, want in enumerate(rescale_grid_oracle()):
    if want is None:
      continue
    worst_a = max(worst_a, ulps(a_new[r], want[0]))
    worst_ls = max([worst_ls] + [ulps(ls_new[r, j], want[1][j]) for j in range(3)])
  return worst_a, worst_ls
