"""The controllers without a GPU: the generator of the MCMC noise pinned to published Philox4x32-10 vectors (oracle and
csrc/gsr_controller.h compiled for the host, the shim), the gate against the reference's soft_lt, the shim's row update
against the fp64 definition, the statistics of the normals, and the logic of the three controllers on a small fake scene
that records its ``split_and_prune`` calls.

`python tests/controller_oracle.py` prints the restatement figure (profiles/r20_controllers.txt)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controller_oracle as co  # noqa: E402
import hostmath  # noqa: E402
from controller_oracle import FakeLogger, FakeScene, fill_state as _fill  # noqa: E402
import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import _lib, controller as ctl  # noqa: E402
from splat_trainer_amd.controller_math import PointState, find_split_prune_indexes, take_n  # noqa: E402

BOUND = co.MARGIN * co.RESTATEMENT


def _note(line: str):
  print(line)


@pytest.fixture(scope="module")
def shim(built_libs):
  return hostmath.load(built_libs)


# ------------------------------------------------------------------------------------------------------------ generator
KNOWN = [([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _hex(w):
  return " ".join(f"{int(x):08x}" for x in w)


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(shim, counter, key, want):
  """The Random123 known-answer vectors of philox4x32-10."""
  assert _hex(co.philox4x32(counter, key)) == want
  assert _hex(co.shim_philox(shim, counter, key)) == want


def test_shim_words_equal_the_oracle_across_the_carries(shim):
  """4 099 (point, step, seed) triples: runs of consecutive points that cross 2^32 (the index's high word changes inside
  the run), steps on both sides of 2^32, seeds with both halves set."""
  runs = [(0, 1000, 0, 0), (2 ** 32 - 500, 1000, 2 ** 32 - 1, 1), (2 ** 32 - 7, 1000, 2 ** 32, 2 ** 63 + 12345),
          (2 ** 33 - 50, 1000, 2 ** 32 + 1, 2 ** 64 - 1), (2 ** 31 - 50, 99, 2 ** 40 + 3, 0xDEADBEEFCAFEF00D)]
  total = 0
  for first, n, step, seed in runs:
    got, _ = co.shim_draws(shim, first, n, seed, step)
    want = co.words(np.arange(n, dtype=np.uint64) + np.uint64(first), seed, step)
    assert np.array_equal(got, want), (first, step, seed)
    total += n
  assert total == 4099
  # the index, the step and the seed each reach the words
  base = co.words(np.arange(64), 5, 9)
  for other in (co.words(np.arange(64) + 2 ** 32, 5, 9), co.words(np.arange(64), 5, 9 + 2 ** 32),
                co.words(np.arange(64), 5 + 2 ** 32, 9), co.words(np.arange(64), 6, 9), co.words(np.arange(64), 5, 10)):
    assert not np.any(np.all(other == base, axis=1))


def test_uniforms_are_never_0_or_1():
  u = co.uniforms_fp64(np.array([0, 0xFF, 0x100, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32))
  assert u.min() == 2.0 ** -25 and u.max() == 1.0 - 2.0 ** -25
  z = co.normals_fp64(np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0, 0x40000000, 0, 0xC0000000]], dtype=np.uint32))
  assert np.abs(z).max() <= np.sqrt(50 * np.log(2)) < 5.9
  # the float32 form keeps both ends: the smallest and the largest uniform give the radius of the definition
  z32 = co.normals_f32(np.array([[0, 0, 0xFFFFFFFF, 0]], dtype=np.uint32))
  want = co.normals_fp64(np.array([[0, 0, 0xFFFFFFFF, 0]], dtype=np.uint32))
  assert np.abs(z32 - want).max() <= co.MARGIN * 2.0 ** -22
  assert abs(float(z32[0, 2])) > 2e-4                   # sqrt(2 * 2^-25): a uniform rounded to 1 would give 0


def test_shim_normals_follow_the_definition(shim):
  w, z = co.shim_draws(shim, 0, 65_536, seed=3, step=11)
  err = float(np.abs(z - co.normals_fp64(w)[:, :3]).max())
  _note(f"shim normals against fp64, 65536 rows: max abs error {err:.3e} (bound {co.MARGIN * 2.0 ** -22:.3e})")
  assert err <= co.MARGIN * 2.0 ** -22


def test_normals_have_the_moments_of_the_sample_size():
  """65 536 rows of oracle normals: each bound is five standard errors of the statistic at that n."""
  n = 65_536
  xi = co.normals_fp64(co.words(np.arange(n), 1, 2))[:, :3]
  mean, var = xi.mean(axis=0), xi.var(axis=0)
  corr = np.corrcoef(xi.T)
  off = np.abs(corr[np.triu_indices(3, 1)])
  _note(f"normals n={n}: |mean| {np.abs(mean).max():.2e} (<= {5 / np.sqrt(n):.2e})  |var - 1| {np.abs(var - 1).max():.2e} "
        f"(<= {5 * np.sqrt(2 / n):.2e})  |corr| {off.max():.2e} (<= {5 / np.sqrt(n):.2e})")
  assert np.all(np.abs(mean) <= 5 / np.sqrt(n))
  assert np.all(np.abs(var - 1) <= 5 * np.sqrt(2 / n))
  assert np.all(off <= 5 / np.sqrt(n))


# ----------------------------------------------------------------------------------------------------------------- gate
def test_gate_equals_the_golden_soft_lt(shim, golden_dir):
  """The gate of the definition (the oracle's, fp64) equals the reference's soft_lt(o, 0.05, margin=16) on the fixture's
  opacities within MARGIN 2^-24 relative for every gate above 2^-100 -- against the reference's own 1 - sigmoid form
  where that form resolves the gate (above 2^-24: its absolute error is 2^-53), against its mirrored one-sigmoid form
  soft_gt(2 h - o, h) everywhere.

  The float32 gate of csrc/gsr_controller.h is held to the bound float32 allows: its relative error is the absolute
  error of its argument x = -(o - h) margin / h, so with u = 2^-24 and three roundings in sigmoid(a)
  it is within u (5 + 2 |x| + 3 o margin / h) -- 2 |x| u for the subtraction and the division, 3 o u margin / h for the
  opacity's own rounding carried through, 5 u for the last sigmoid -- times MARGIN for the libm."""
  with open(os.path.join(golden_dir, "controller_vectors.json")) as f:
    v = json.load(f)
  o, h, margin = np.array(v["opacity"]), v["threshold"], v["margin"]
  ref, mirrored = np.array(v["soft_lt"]), np.array(v["soft_gt_mirrored"])
  gate = co.soft_lt_fp64(o, h, margin)
  above = mirrored > 2.0 ** -100
  resolved = ref > v["resolved_above"]
  assert above.sum() > 80 and resolved.sum() > 40 and (above & ~resolved).sum() > 20
  rel = lambda got, want: np.abs(got - want) / want
  e_ref, e_mir = float(rel(gate[resolved], ref[resolved]).max()), float(rel(gate[above], mirrored[above]).max())
  _note(f"gate (fp64 definition) against soft_lt: {e_ref:.2e} on {int(resolved.sum())} resolved gates, against the mirrored "
        f"form {e_mir:.2e} on {int(above.sum())} gates above 2^-100 (bound {co.MARGIN * 2.0 ** -24:.2e})")
  assert e_ref <= co.MARGIN * 2.0 ** -24 and e_mir <= co.MARGIN * 2.0 ** -24
  assert np.all(ref[~above] == 0.0)                     # what 1 - sigmoid does below 1e-16: the form not to copy

  # float32: the shim on the fixture's logits at threshold 0.1 (h = float32(0.1) / 2, as the oracle's own h)
  logit = np.array(v["logit"], dtype=np.float32)
  got = co.shim_level(shim, logit, 1.0, threshold=0.1, margin=margin).astype(np.float64)
  want = co.gate_fp64(logit, 0.1, margin)
  h32 = 0.5 * float(np.float32(0.1))
  x = np.abs((o - h32) * margin / h32)
  bound = co.MARGIN * 2.0 ** -24 * (5 + 2 * x + 3 * o * margin / h32)
  big = want > 2.0 ** -100
  worst = float((rel(got[big], want[big]) / bound[big]).max())
  _note(f"gate (float32, host): largest error / bound {worst:.3f}; largest relative error {float(rel(got[big], want[big]).max()):.2e}")
  assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------- row update
ROWS = 200_000


@pytest.fixture(scope="module")
def rows():
  assert co.SAMPLES[-1] == (ROWS, 1, 0, 17, 23)           # one of the samples the recorded figure is the maximum over
  ls, q, a = co.random_rows(ROWS, seed=1)
  idx = np.arange(ROWS, dtype=np.uint64)
  want, s_row = co.offsets_fp64(ls, q, a, idx, 17, 23, 100.0)
  return dict(ls=ls, q=q, a=a, idx=idx, want=want, s_row=s_row)


def test_restatement_stays_inside_its_recorded_error(rows):
  got, written = co.offsets_f32(rows["ls"], rows["q"], rows["a"], rows["idx"], 17, 23, 100.0)
  worst, small = co.row_error(got, rows["want"], rows["s_row"])
  _note(f"restatement, {ROWS} rows: {worst:.3e} of s_row (recorded {co.RESTATEMENT:.1e}); rows below 2^-100: |offset| <= {small:.2e}; "
        f"{int(written.sum())} rows written")
  assert worst <= co.RESTATEMENT
  assert small <= 2.0 ** -97


def test_shim_row_update_stays_inside_the_bound(shim, rows):
  zero = np.zeros((ROWS, 3), dtype=np.float32)
  views = np.full(ROWS, 9, dtype=np.int16)
  got = co.shim_noise(shim, zero, rows["ls"], rows["q"], rows["a"], views, 5, 100.0, 17, 23)
  worst, small = co.row_error(got, rows["want"], rows["s_row"])
  _note(f"shim row update, {ROWS} rows: {worst:.3e} of s_row (bound {BOUND:.2e}); rows below 2^-100: |offset| <= {small:.2e}")
  assert worst <= BOUND
  assert small <= 2.0 ** -97
  assert np.abs(got).max() > 1.0                        # the rows do move


def test_shim_skips_rows_with_too_few_views(shim, rows):
  n = 4099
  rng = np.random.default_rng(4)
  p0 = rng.normal(size=(n, 3)).astype(np.float32)
  views = rng.integers(0, 12, n).astype(np.int16)
  ls, q, a = rows["ls"][:n], rows["q"][:n], rows["a"][:n]
  got = co.shim_noise(shim, p0, ls, q, a, views, 5, 100.0, 17, 23)
  skipped = views <= 5
  assert skipped.sum() > 1000 and (~skipped).sum() > 1000
  assert np.array_equal(got[skipped].view(np.uint32), p0[skipped].view(np.uint32))
  moved = np.any(got != p0, axis=1)
  assert not moved[skipped].any() and moved[~skipped].mean() > 0.3
  # a shorter prefix gives the same rows: nothing depends on N
  assert np.array_equal(co.shim_noise(shim, p0[:1000], ls[:1000], q[:1000], a[:1000], views[:1000], 5, 100.0, 17, 23),
                        got[:1000])


# ---------------------------------------------------------------------------------------------------------- controllers
def test_progress_and_schedules():
  assert sta.Progress(250, 1000).t == 0.25 and sta.Progress(1500, 1000).t == 1.0 and float(sta.Progress(0, 10)) == 0.0
  assert ctl.eval_schedule(7, 0.3) == 7 and ctl.eval_schedule(lambda t: 100 * (1 - t), sta.Progress(250, 1000)) == 75.0
  assert ctl.smoothstep(0.5, 1000, 2000) == 1500 and ctl.smoothstep(-1, 3, 5) == 3 and ctl.smoothstep(2, 3, 5) == 5


def test_target_schedule_at_hand_computed_values():
  scene = FakeScene(1000)
  c = sta.TargetConfig().make_controller(scene, 2000, sta.Progress(0, 1000))
  assert (c.config.prune_rate, c.config.target_count_t, c.config.min_views, c.config.max_scale_px, c.config.min_split_px,
          c.config.densify_prune_interval) == (0.04, 0.8, 5, 200, 0.0, 100)
  assert c.start_points == 1000 and c.next_densify == 100
  # target step 800; t = 0.25: 3/16 - 2/64 = 0.15625; t = 0.5: 0.5
  assert c.target_points(sta.Progress(0, 1000)) == 1000
  assert c.target_points(sta.Progress(200, 1000)) == 1156
  assert c.target_points(sta.Progress(400, 1000)) == 1500
  assert c.target_points(sta.Progress(800, 1000)) == 2000 and c.target_points(sta.Progress(999, 1000)) == 2000
  assert c.find_next_densify(sta.Progress(700, 1000)) == 800          # 800 + 100 < 1000
  assert c.find_next_densify(sta.Progress(800, 1000)) is None         # 900 + 100 is not
  varying = sta.TargetConfig(densify_prune_interval=lambda t: 50 if t < 0.5 else 200).make_controller(
      scene, 2000, sta.Progress(0, 1000))
  assert varying.next_densify == 50 and varying.find_next_densify(sta.Progress(500, 1000)) == 700


def test_target_round_equals_find_split_prune_indexes():
  scene, logger = FakeScene(1000), FakeLogger()
  config = sta.TargetConfig(prune_rate=0.025, min_split_px=20.0)
  c = config.make_controller(scene, 1500, sta.Progress(0, 1000), logger)
  _fill(c.points, 3)
  before = PointState(**{k: v.clone() for k, v in vars(c.points).items()})
  c.step(sta.Progress(99, 1000))
  assert not scene.calls and torch.equal(c.points.prune_cost, before.prune_cost)      # not yet due: nothing happens
  progress = sta.Progress(100, 1000)
  split, prune = find_split_prune_indexes(before, progress.t, c.target_points(progress), prune_rate=0.025, min_views=5,
                                          max_scale_px=200, min_split_px=20.0)
  assert split.any() and prune.any() and not (split & prune).any()
  c.step(progress, log_details=True)
  assert len(scene.calls) == 1 and not scene.calls[0]["kw"]           # no generator given: none passed on
  assert torch.equal(scene.calls[0]["keep_mask"], ~(split | prune))
  assert torch.equal(scene.calls[0]["split_idx"], split.nonzero().squeeze(1))
  n = 1000 - int(split.sum()) - int(prune.sum()) + 2 * int(split.sum())
  assert scene.num_points == n and c.points.prune_cost.shape[0] == n
  assert all(not getattr(c.points, k).any() for k in vars(before))    # a fresh zero state after a round
  assert c.points.points_in_view.dtype == torch.int16 and c.next_densify == 200
  name, metrics = logger.values[0]
  assert name == "densify" and metrics["n"] == 1000 and metrics["prune"] == int(prune.sum())
  assert metrics["split"] == int(split.sum()) and set(metrics) == {"n", "prune", "split", "max_prune_score",
                                                                    "min_split_score", "unseen"}
  assert metrics["max_prune_score"] == before.prune_cost[prune].max().item()
  assert metrics["min_split_score"] == before.split_score[split].min().item()
  assert "step/prune_cost" in logger.histograms and "densify/points_in_view" in logger.histograms
  g = torch.Generator().manual_seed(1)
  _fill(c.points, 4)
  c.step(sta.Progress(200, 1000), generator=g)
  assert scene.calls[1]["kw"] == {"generator": g}


def _mcmc_masks_literal(state, alpha_logit, config):
  """mcmc_controller.py:76-87 written out, with a stable sort and the stated deviation."""
  opacity = torch.sigmoid(alpha_logit).squeeze(1)
  prune_mask = (state.max_scale_px > config.max_scale_px) | (opacity < config.opacity_threshold)
  n = prune_mask.sum().item()
  too_small = state.max_scale_px < config.min_split_px
  split_score = torch.where(prune_mask | too_small, 0, state.split_score)
  idx = torch.argsort(split_score, descending=True, stable=True)[:n]
  split_mask = torch.zeros_like(split_score, dtype=torch.bool)
  split_mask[idx] = True
  return split_mask & ~prune_mask, prune_mask, split_mask & prune_mask


@pytest.mark.parametrize("case", ["ties", "overlap"])
def test_mcmc_prune_branch_against_a_literal_restatement(case):
  """"ties": the selection boundary falls inside a run of equal scores.  "overlap": more rows are pruned than have a
  positive score left, so the literal form picks pruned rows among the zeros and the count falls by that overlap."""
  n = 600
  scene = FakeScene(n, seed=5)
  config = sta.MCMCConfig(prune_interval=20, min_split_px=10.0, max_scale_px=240.0)
  assert (sta.MCMCConfig().opacity_threshold, sta.MCMCConfig().prune_interval, sta.MCMCConfig().min_views,
          sta.MCMCConfig().max_scale_px, sta.MCMCConfig().min_split_px, sta.MCMCConfig().noise_level,
          sta.MCMCConfig().seed) == (0.1, 50, 5, 200, 0.0, 100.0, 0)
  assert not hasattr(config, "max_prune_rate")
  c = config.make_controller(scene, 1000, sta.Progress(0, 100))
  _fill(c.points, 6)
  with torch.no_grad():
    scene.points.alpha_logit[:20] = -6.0                               # nearly transparent among the top-scored
    if case == "overlap":
      scene.points.alpha_logit[:400] -= 3.0                            # most rows nearly transparent: n is large
    c.points.split_score[torch.arange(0, n, 2)] = 0.5                  # ties in the score, half of the rows
    c.points.split_score[:40] = 5.0                                    # rows that are both pruned and top-scored
  opacity = torch.sigmoid(scene.points.alpha_logit)
  assert (opacity - config.opacity_threshold).abs().min() > 1e-5       # no opacity on the threshold
  before = PointState(**{k: v.clone() for k, v in vars(c.points).items()})
  split, prune, overlap = _mcmc_masks_literal(before, scene.points.alpha_logit.clone(), config)
  n_prune, n_split, n_overlap = int(prune.sum()), int(split.sum()), int(overlap.sum())
  assert n_split > 0 and n_split == n_prune - n_overlap and prune[:20].all() and not split[:20].any()
  if case == "overlap":
    assert n_overlap > 0
  else:
    # the tie value is on the boundary of the selection: among equal scores the lowest indexes are taken
    tied = (before.split_score == 0.5) & ~prune & ~(before.max_scale_px < 10.0)
    assert (split & tied).any() and (~split & tied).any()
    assert tied.nonzero()[split[tied]].max() < tied.nonzero()[~split[tied]].min()
  c.step(sta.Progress(40, 100))
  call = scene.calls[0]
  assert torch.equal(call["keep_mask"], ~(split | prune)) and torch.equal(call["split_idx"], split.nonzero().squeeze(1))
  kept = int((~(split | prune)).sum())
  assert scene.num_points == kept + 2 * n_split == n + n_split - n_prune == n - n_overlap
  # the state is carried: kept rows in order, children zero, dtypes kept
  for k, v in vars(before).items():
    now = getattr(c.points, k)
    assert now.dtype == v.dtype and torch.equal(now[:kept], v[~(split | prune)]) and not now[kept:].any(), k
    assert now.shape[0] == scene.num_points
  assert c.points.points_in_view.dtype == torch.int16 and c.num_points == scene.num_points


def test_mcmc_noise_branch_has_no_cpu_fallback():
  scene = FakeScene(50)
  c = sta.MCMCConfig().make_controller(scene, 100, sta.Progress(0, 100))
  with pytest.raises(sta.GsplatHipError, match="no CPU fallback"):
    c.step(sta.Progress(1, 100))
  assert not scene.calls


def test_disabled_resets_its_state_and_leaves_the_scene():
  scene, logger = FakeScene(100), FakeLogger()
  c = sta.DisabledConfig().make_controller(scene, 200, sta.Progress(0, 100), logger)
  _fill(c.points, 7)
  c.step(sta.Progress(1, 100), log_details=True)
  assert not scene.calls and scene.num_points == 100 and "step/visibility" in logger.histograms
  assert all(not v.any() for v in vars(c.points).values()) and c.points.prune_cost.shape[0] == 100
  assert c.state_dict() == {}
  again = sta.DisabledConfig().from_state_dict({}, scene, 200, sta.Progress(0, 100), None)
  assert isinstance(again, sta.DisabledController) and isinstance(again, sta.Controller)


def test_state_dicts_round_trip():
  scene = FakeScene(300)
  progress = sta.Progress(150, 1000)
  for config in (sta.TargetConfig(), sta.MCMCConfig()):
    assert isinstance(config, sta.ControllerConfig)
    c = config.make_controller(scene, 900, progress)
    _fill(c.points, 8)
    state = c.state_dict()
    if isinstance(config, sta.TargetConfig):
      c.start_points = 123
      state = c.state_dict()
      assert set(state) == {"points", "start_points"} and state["start_points"] == 123
    else:
      assert set(state) == {"points"}
    saved = {k: v.clone() for k, v in state["points"].items()}
    c.points.prune_cost.zero_()                                      # the dict holds copies
    assert torch.equal(state["points"]["prune_cost"], saved["prune_cost"])
    back = config.from_state_dict(state, scene, 900, progress)
    assert type(back) is type(c)
    for k, v in saved.items():
      assert torch.equal(getattr(back.points, k), v) and getattr(back.points, k).dtype == v.dtype, k
    if isinstance(config, sta.TargetConfig):
      assert back.start_points == 123 and back.next_densify == 250
  with pytest.raises(ValueError):
    sta.MCMCConfig().from_state_dict(dict(points=point_rows(299)), scene, 900, progress)


def point_rows(n):
  return ctl.point_state_dict(PointState.new_zeros(n, "cpu"))


def test_densify_and_prune_returns_the_carried_state():
  scene = FakeScene(10)
  state = _fill(PointState.new_zeros(10, "cpu"), 9)
  split = torch.tensor([0, 1, 0, 0, 0, 0, 1, 0, 0, 0], dtype=torch.bool)
  prune = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.bool)
  out = sta.densify_and_prune(state, scene, split, prune)
  keep = ~(split | prune)
  assert scene.num_points == 10 and out.prune_cost.shape[0] == 10     # 6 kept + 2 x 2 children
  for k, v in vars(state).items():
    assert torch.equal(getattr(out, k)[:6], v[keep]) and not getattr(out, k)[6:].any()
  assert take_n(torch.tensor([1.0, 3.0, 3.0, 2.0]), 2, descending=True).tolist() == [False, True, True, False]


# -------------------------------------------------------------------------------------------------------------- binding
def test_binding_gains_the_two_entries_and_keeps_the_abi():
  assert _lib.ABI_VERSION == 38
  noise, draws = _lib.FUNCTIONS["gsr_mcmc_noise"], _lib.FUNCTIONS["gsr_mcmc_draws"]
  assert noise == ("int", ["float*", "const float*", "const float*", "const float*", "const int16_t*", "int64_t",
                           "int32_t", "float", "float", "float", "float", "uint64_t", "uint64_t", "void*"])
  assert draws == ("int", ["int64_t", "uint64_t", "uint64_t", "uint32_t*", "float*", "void*"])
  assert _lib.PROTOTYPES["gsr_mcmc_noise"][1][11] is C.c_uint64
  for name in ("Progress", "ControllerConfig", "Controller", "DisabledConfig", "DisabledController", "TargetConfig",
               "TargetController", "MCMCConfig", "MCMCController", "densify_and_prune", "mcmc_noise"):
    assert name in sta.__all__ and hasattr(sta, name)
