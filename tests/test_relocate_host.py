"""The MCMC relocation without a GPU (csrc/gsr_relocate.h compiled for the host, the shim): the weighted draw against the
Python-integer oracle on every entry, the rule's distribution, the opacity weights within 1 of the exact value, and the
opacity / scale correction within 2 float32 ulps of the 60-digit oracle (tests/relocate_oracle.py).

The correction's bound: the fp64 evaluation's own error in log(coeff) -- measured below on this file's grid and printed --
is 2.5e-13, under a hundredth of a float32 ulp of the smallest log-scale the grid produces, so the final float32 rounding
(half an ulp) dominates and 2 ulps is the bound."""
import math

import mpmath
import numpy as np
import pytest

import controller_oracle as co
import hostmath
import relocate_oracle as ro
import splat_trainer_amd as sta
from splat_trainer_amd import controller as ctl


def _note(line: str):
  print(line)


@pytest.fixture(scope="module")
def shim(built_libs):
  return hostmath.load(built_libs)


# ---------------------------------------------------------------------------------------------------------------- words
def test_words_at_a_published_vector(shim):
  """The third Random123 known-answer vector of philox4x32-10 read as a tagged counter: draw 0x85a308d3243f6a88 at step
  0x70734413198a2e in domain 3, seed 0x299f31d0a4093822."""
  k, step, domain, seed = 0x85A308D3243F6A88, 0x0070734413198A2E, 3, 0x299F31D0A4093822
  want = "d16cfe09 94fdcceb 5001e420 24126ea1"
  assert " ".join(f"{int(x):08x}" for x in ro.draw_words([k], seed, step, domain)[0]) == want
  assert " ".join(f"{int(x):08x}" for x in ro.shim_words(shim, k, seed, step, domain)) == want


def test_domains_give_different_words_and_domain_0_is_the_noise_stream(shim):
  k = np.arange(64, dtype=np.uint64) + np.uint64(2 ** 32 - 32)
  by_domain = [ro.draw_words(k, ro.SEED, ro.STEP, d) for d in (0, 1, 2)]
  assert np.array_equal(by_domain[0], co.words(k, ro.SEED, ro.STEP))          # the noise step's words: tag 0
  for a in range(3):
    for b in range(a + 1, 3):
      assert not np.any(np.all(by_domain[a] == by_domain[b], axis=1))
  for d in (0, 1, 2):
    for i in (0, 31, 32, 63):
      assert np.array_equal(ro.shim_words(shim, int(k[i]), ro.SEED, ro.STEP, d), by_domain[d][i])
  # only the low 24 bits of the step's high word reach the counter
  assert np.array_equal(ro.draw_words(k, 1, 5 + (1 << 56), 1), ro.draw_words(k, 1, 5, 1))


# ---------------------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("N", ro.SIZES)
def test_draws_equal_the_integer_oracle(shim, N):
  for name, weights in ro.weight_patterns(N).items():
    want_sources, want_counts, want_S = ro.draws(weights, 1000, ro.SEED, ro.STEP, 1)
    for n in ro.DRAWS:
      sources, counts, S = ro.shim_draws(shim, weights, n, ro.SEED, ro.STEP, 1)
      assert S == want_S == int(weights.astype(np.uint64).sum()), (name, n)
      assert np.array_equal(sources, want_sources[:n]), (name, n)              # n = 1000 begins with n = 64: not a function of n
      assert np.array_equal(counts, np.bincount(sources, minlength=N)), (name, n)
      assert np.all(weights[sources] > 0)
    assert np.array_equal(counts, want_counts), name
  assert want_S > 2 ** 32 or N != 4099                                         # "full", the last pattern at 4099


def test_draws_depend_on_domain_step_and_seed(shim):
  weights = ro.weight_patterns(1025)["random"]
  base = ro.shim_draws(shim, weights, 1000, ro.SEED, ro.STEP, 1)[0]
  for other in ((ro.SEED, ro.STEP, 2), (ro.SEED, ro.STEP + 1, 1), (ro.SEED + 1, ro.STEP, 1)):
    got = ro.shim_draws(shim, weights, 1000, other[0], other[1], other[2])[0]
    assert np.array_equal(got, ro.draws(weights, 1000, *other)[0])
    assert (got != base).mean() > 0.9


@pytest.mark.parametrize("N", [0, 1, 300])
def test_a_total_of_zero_draws_nothing(shim, N):
  sources, counts, S = ro.shim_draws(shim, np.zeros(N, dtype=np.uint32), 64, ro.SEED, ro.STEP, 1)
  assert S == 0 and np.all(sources == -1) and sources.shape == (64,) and not counts.any() and counts.shape == (N,)
  want = ro.draws(np.zeros(N, dtype=np.uint32), 64, ro.SEED, ro.STEP, 1)
  assert np.array_equal(sources, want[0]) and np.array_equal(counts, want[1])


def test_distribution_of_200000_draws_over_16_weights(shim):
  """Every frequency within 5 standard deviations of w_i / S: sigma_i = sqrt(n p_i (1 - p_i))."""
  weights = np.array([1, 2, 5, 17, 64, 255, 1000, 4096, 2 ** 14, 2 ** 16, 2 ** 18, 2 ** 20, 2 ** 22, 2 ** 23, 2 ** 24 - 1, 2 ** 24],
                     dtype=np.uint32)
  n = 200_000
  sources, counts, S = ro.shim_draws(shim, weights, n, 12345, 678, 1)
  assert np.array_equal(sources, ro.draws(weights, n, 12345, 678, 1)[0])
  p = weights.astype(np.float64) / S
  z = (counts - n * p) / np.sqrt(n * p * (1 - p))
  _note("distribution: z = " + " ".join(f"{v:+.2f}" for v in z))
  assert np.all(np.abs(z) <= 5.0)


# -------------------------------------------------------------------------------------------------------------- weights
def test_weights_are_within_1_of_the_exact_value(shim):
  a = np.concatenate([np.linspace(-30.0, 30.0, 1201), [-16.635532, -16.6355, 16.6, 17.0, -0.0, 1e-30]]).astype(np.float32)
  alive = np.ones(a.shape[0], dtype=bool)
  alive[::7] = False
  got = ro.shim_weights(shim, a, alive)
  want = np.array([ro.weight(x, l) for x, l in zip(a, alive)], dtype=np.int64)
  worst = int(np.abs(got.astype(np.int64) - want).max())
  _note(f"weights, {a.shape[0]} logits in [-30, 30]: max |w - oracle| = {worst}; range {got[alive].min()} .. {got.max()}")
  assert worst <= 1
  assert np.all(got[alive] >= 1) and np.all(got[~alive] == 0) and got.max() <= 2 ** 24
  assert np.array_equal(ro.shim_weights(shim, a), np.where(alive, got, ro.shim_weights(shim, a)))      # NULL: all alive
  assert np.all(ro.shim_weights(shim, a) >= 1)
  assert ro.shim_weights(shim, np.array([np.nan], dtype=np.float32))[0] == 1


# -------------------------------------------------------------------------------------------------------------- rescale
def test_the_single_sum_equals_the_double_sum():
  """sum_i C(i-1, k) = C(n, k+1): the collapsed form the kernel uses against Eq. 9 as printed, at 60 digits."""
  worst = mpmath.mpf(0)
  for a in (-12.0, -2.0, 0.0, 4.6, 16.0):
    for copies in (1, 2, 7, 50):
      op, n = ro.corrected_opacity(a, copies)
      d2, d1 = ro.denominator_double_sum(op, n), ro.denominator_single_sum(op, n)
      worst = max(worst, abs(d1 - d2) / abs(d2))
  _note(f"single against double sum: max relative difference {float(worst):.2e}")
  assert worst < mpmath.mpf(10) ** -40


def test_fp64_error_of_the_correction_on_the_grid(shim):
  """The measurement the bound rests on: |log(coeff)_fp64 - oracle| over the grid, its ends included."""
  a, ls, counts = ro.rescale_grid()
  live = counts > 0
  a_out, log_coeff = np.empty(int(live.sum()), dtype=np.float32), np.empty(int(live.sum()), dtype=np.float64)
  shim.hm_reloc_rescale_rows(np.ascontiguousarray(a[live]), np.ascontiguousarray(counts[live]), int(live.sum()),
                             ro.O_FLOOR, a_out, log_coeff)
  worst, at = 0.0, None
  for x, c, got, want in zip(a[live], counts[live], log_coeff, [w for w in ro.rescale_grid_oracle() if w is not None]):
    err = float(abs(mpmath.mpf(float(got)) - (want[1][0] - mpmath.mpf(float(ro.LOG_SCALES[0])))))
    if err > worst:
      worst, at = err, (float(x), int(c))
  smallest = min(float(abs(v)) for w in ro.rescale_grid_oracle() if w is not None for v in w[1])
  _note(f"fp64 log(coeff) on the grid: max abs error {worst:.3e} at (logit, count) = {at}; smallest |new log-scale| {smallest:.3e}")
  # the fp64 error is under a hundredth of a float32 ulp of the smallest log-scale the grid produces: the float32
  # rounding, half an ulp, dominates
  assert worst < 0.01 * float(np.spacing(np.float32(smallest)))


def test_rescale_stays_within_2_ulps_of_the_oracle(shim):
  a, ls, counts = ro.rescale_grid()
  a_new, ls_new = ro.shim_rescale(shim, a, ls, counts, ro.O_FLOOR)
  worst_a, worst_ls = ro.worst_ulps(a_new, ls_new)
  _note(f"rescale, {int((counts > 0).sum())} rows: logit {worst_a:.3f} ulps, log-scales {worst_ls:.3f} ulps (bound {ro.ULP_BOUND})")
  assert np.isfinite(a_new).all() and np.isfinite(ls_new).all()
  assert worst_a <= ro.ULP_BOUND and worst_ls <= ro.ULP_BOUND
  # a count of 0 leaves the row's bits alone
  idle = counts == 0
  assert np.array_equal(a_new[idle].view(np.uint32), a[idle].view(np.uint32))
  assert np.array_equal(ls_new[idle].view(np.uint32), ls[idle].view(np.uint32))
  # the cap: a count of 1000 is a count of 50
  assert np.array_equal(a_new[counts == 1000].view(np.uint32), a_new[counts == 50].view(np.uint32))
  assert np.array_equal(ls_new[counts == 1000].view(np.uint32), ls_new[counts == 50].view(np.uint32))
  assert not np.array_equal(a_new[counts == 7], a_new[counts == 50])
  # the clamp: no new opacity below the floor
  assert np.all(a_new[~idle] >= np.float32(math.log(ro.O_FLOOR / (1 - ro.O_FLOOR))) - np.float32(1e-6))


def test_rescaled_copies_compose_to_the_source_opacity():
  """What the correction is for, at 60 digits: 1 - (1 - o')^n = o."""
  for a in (-2.0, 0.405, 4.6):
    for copies in (1, 4, 50):
      op, n = ro.corrected_opacity(a, copies)
      o = 1 / (1 + mpmath.exp(-mpmath.mpf(float(np.float32(a)))))
      assert abs(1 - (1 - op) ** n - o) < mpmath.mpf(10) ** -50


# ----------------------------------------------------------------------------------------------------------- row moves
def test_shim_row_move(shim, built_libs):
  rng = np.random.default_rng(3)
  N, n = 50, 12
  cols = [rng.normal(size=(N, w)).astype(np.float32) for w in (1, 3, 4, 8)] + [rng.normal(size=(N, 2)).astype(np.float32)]
  before = [c.copy() for c in cols]
  dst = rng.permutation(25)[:n].astype(np.int32)
  src = (25 + rng.integers(0, 25, n)).astype(np.int32)
  dst[3], src[5] = -1, N                                                       # both skipped
  table = np.zeros(len(cols), dtype=np.dtype([("data", np.uint64), ("width", np.int32), ("zero", np.int32)]))
  for i, c in enumerate(cols):
    table[i] = (c.ctypes.data, c.shape[1], int(i == len(cols) - 1))
  assert table.itemsize == 16
  assert shim.hm_relocate_rows(dst, src, n, N, table, len(cols)) == 0
  moved = [k for k in range(n) if k not in (3, 5)]
  for c, b in zip(cols[:-1], before[:-1]):
    want = b.copy()
    want[dst[moved]] = b[src[moved]]
    assert np.array_equal(c.view(np.uint32), want.view(np.uint32))
  want = before[-1].copy()
  want[dst[moved]] = 0
  want[src[moved]] = 0
  assert np.array_equal(cols[-1], want)


# ------------------------------------------------------------------------------------------------------------- the rest
def test_growth_rule_at_hand_computed_values():
  assert ctl.growth_target(300, 10_000, 0.05) == 315 and ctl.growth_target(315, 10_000, 0.05) == 331
  assert ctl.growth_target(300, 310, 0.05) == 310 and ctl.growth_target(300, 200, 0.05) == 300
  assert ctl.growth_target(1, 10, 0.05) == 2 and ctl.growth_target(0, 10, 0.05) == 0 and ctl.growth_target(7, 10, 0.0) == 7


def test_config_fields_and_exports():
  c = sta.MCMCConfig()
  assert c.relocate is False and c.grow_rate == 0.05
  for name in ("weighted_draws", "relocate_points", "grow_points", "relocate_weights", "relocate_rescale", "relocate_rows",
               "growth_target"):
    assert name in sta.__all__ and hasattr(sta, name), name
  assert (ctl.RELOCATE_DOMAIN, ctl.GROW_DOMAIN) == (1, 2)


def test_no_cpu_fallback():
  import torch
  with pytest.raises(sta.GsplatHipError, match="no CPU fallback"):
    sta.weighted_draws(torch.ones(8, dtype=torch.int32), 4, 0, 0, 1)
  with pytest.raises(sta.GsplatHipError, match="no CPU fallback"):
    sta.relocate_weights(torch.zeros(8, 1))
  with pytest.raises(sta.GsplatHipError, match="no CPU fallback"):
    sta.relocate_rescale(torch.zeros(8, 1), torch.zeros(8, 3), torch.zeros(8, dtype=torch.int32), 0.1)
