"""The controllers on the GPU (splat_trainer_amd.controller, csrc/controller.hip): the generator against the integer oracle
bit for bit, the noise step against the fp64 definition (tests/controller_oracle.py) inside MARGIN x the float32
restatement's own error, the rows it must not touch, its independence of N, of the launch shape and of earlier calls, an
``MCMCController`` beside a small ``MLPScene`` through two prune rounds, and a ``TargetController`` round against the CPU
masks of the same state.

N covers 0, 1, a few rows (3 / 4 / 5), the 64-row slot of a wave (63 / 64 / 65), the wave's 256 rows (257), the 1024-row
block (1000 / 1023 / 1024 / 1025) and several blocks with a tail (4099).  One set of 4099 rows and one fp64 reference serve
every N: a smaller N takes the prefix."""
import numpy as np
import pytest
import torch

import controller_oracle as co
import splat_trainer_amd as sta
from controller_oracle import FakeScene, fill_state
from splat_trainer_amd import controller as ctl, synthetic
from splat_trainer_amd.controller_math import PointState, find_split_prune_indexes

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 257, 1000, 1023, 1024, 1025, 4099]
FULL = 4099
SEED, STEP = 2 ** 63 + 77, 2 ** 32 + 5              # both words of the key and of the step counter are in use
NOISE, MIN_VIEWS = 100.0, 5
BOUND = co.MARGIN * co.RESTATEMENT


def _note(line: str):
  """Every figure is printed before it is asserted (run with -s to keep them)."""
  print(line)


@pytest.fixture(scope="module")
def rows():
  """4099 rows on the host with their fp64 offsets; never modified."""
  ls, q, a = co.random_rows(FULL, seed=11)
  # four rows whose levels are non-zero but tiny: rows 10 and 11 underflow against their sigma
  a[8:12] = np.float32(-0.547)                # gate about 1e-44, seven units of the smallest float32
  ls[8:10], ls[10:12] = 2.0, -8.0
  rng = np.random.default_rng(12)
  position = rng.normal(scale=3.0, size=(FULL, 3)).astype(np.float32)
  views = rng.integers(0, 12, FULL).astype(np.int16)
  want, s_row = co.offsets_fp64(ls, q, a, np.arange(FULL, dtype=np.uint64), SEED, STEP, NOISE)
  return dict(ls=ls, q=q, a=a, position=position, views=views, want=want, s_row=s_row)


def _run(rows, n, position=None, views=None, seed=SEED, step=STEP):
  """The noise step on the first n rows -> new positions (n, 3) as numpy."""
  dev = lambda t: torch.from_numpy(np.ascontiguousarray(t[:n])).cuda()
  p = dev(np.zeros((FULL, 3), dtype=np.float32) if position is None else position)
  v = dev(np.full(FULL, MIN_VIEWS + 1, dtype=np.int16) if views is None else views)
  out = sta.mcmc_noise(p, dev(rows["ls"]), dev(rows["q"]), dev(rows["a"])[:, None], v, min_views=MIN_VIEWS,
                       opacity_threshold=co.THRESHOLD, noise_level=NOISE, seed=seed, step=step)
  assert out is p
  return p.cpu().numpy()


@pytest.fixture(scope="module")
def full(rows):
  """The step on all 4099 rows from their real positions with their real view counts."""
  return _run(rows, FULL, rows["position"], rows["views"])


# ---------------------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("n", SIZES)
def test_draws_equal_the_oracle(n):
  words, normals = ctl.mcmc_draws(n, SEED, STEP)
  assert tuple(words.shape) == (n, 4) and tuple(normals.shape) == (n, 3)
  if n == 0:
    return
  w = words.cpu().numpy().view(np.uint32)
  want = co.words(np.arange(n, dtype=np.uint64), SEED, STEP)
  assert np.array_equal(w, want)
  err = float(np.abs(normals.cpu().numpy().astype(np.float64) - co.normals_fp64(want)[:, :3]).max())
  _note(f"draws N={n}: words bit-equal; normals max abs error {err:.3e} (bound {co.MARGIN * 2.0 ** -22:.3e})")
  assert err <= co.MARGIN * 2.0 ** -22


# ------------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("n", SIZES)
def test_update_from_zero_stays_inside_the_bound(rows, n):
  got = _run(rows, n)
  assert got.shape == (n, 3)
  if n == 0:
    return
  worst, small = co.row_error(got, rows["want"][:n], rows["s_row"][:n])
  moved = int(np.any(got != 0, axis=1).sum())
  _note(f"noise N={n}: {worst:.3e} of s_row (bound {BOUND:.2e}); rows below 2^-100: |offset| <= {small:.2e}; {moved} rows moved")
  assert np.isfinite(got).all()
  assert worst <= BOUND
  assert small <= 2.0 ** -97
  if n >= 63:
    assert moved > n // 4


def test_update_from_real_positions(rows, full):
  eligible = rows["views"] > MIN_VIEWS
  p0 = rows["position"].astype(np.float64)
  err = np.abs(full.astype(np.float64) - (p0 + rows["want"]))
  ulp = np.spacing((np.abs(rows["position"]) + np.abs(rows["want"]).astype(np.float32)).astype(np.float32)).astype(np.float64)
  big = eligible & (rows["s_row"] >= 2.0 ** -100)
  slack = err[big] - ulp[big]
  worst = float((slack.max(axis=1) / rows["s_row"][big]).max())
  _note(f"real start, {int(big.sum())} rows: (error - 1 ulp) {worst:.3e} of s_row (bound {BOUND:.2e})")
  assert worst <= BOUND
  small = eligible & ~big
  assert np.all(err[small] <= 2.0 ** -97 + ulp[small])


def test_skipped_rows_keep_their_bits(rows, full):
  skipped = rows["views"] <= MIN_VIEWS
  assert 1000 < skipped.sum() < FULL - 1000
  assert np.array_equal(full[skipped].view(np.uint32), rows["position"][skipped].view(np.uint32))
  moved = np.any(full != rows["position"], axis=1)
  assert moved[~skipped].mean() > 0.3 and not moved[skipped].any()
  # an opaque row -- s_row far below the smallest float32 (2^-149) -- has no offset in float32 and stays as well
  opaque = ~skipped & (rows["s_row"] < 2.0 ** -160)
  assert opaque.sum() > 100 and not moved[opaque].any()
  # rows 10 and 11: a level of a few units of 2^-149 times a sigma of 3e-4 is below half a unit
  assert not _run(rows, 12)[10:12].any()


@pytest.mark.parametrize("n", SIZES[:-1])
def test_a_row_does_not_depend_on_n(rows, full, n):
  got = _run(rows, n, rows["position"], rows["views"])
  assert np.array_equal(got.view(np.uint32), full[:n].view(np.uint32))


def test_repeatable_and_sensitive_to_step_and_seed(rows, full):
  again = _run(rows, FULL, rows["position"], rows["views"])
  assert np.array_equal(again.view(np.uint32), full.view(np.uint32))
  moved = np.any(full != rows["position"], axis=1)
  for name, other in (("step", _run(rows, FULL, rows["position"], rows["views"], step=STEP + 1)),
                      ("seed", _run(rows, FULL, rows["position"], rows["views"], seed=SEED + 1))):
    changed = np.any(other != full, axis=1)
    share = changed[moved].mean()
    _note(f"another {name}: {share:.4f} of the {int(moved.sum())} perturbed rows change")
    assert share > 0.99


def test_noise_step_has_no_host_wait(rows):
  """Neither the native call nor the controller's noise branch around it synchronises (torch raises on a synchronising
  call in this mode)."""
  dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda()
  scene = FakeScene(FULL, device="cuda")
  scene.points.log_scaling, scene.points.rotation = dev(rows["ls"]), dev(rows["q"])
  scene.points.alpha_logit, scene.points.position = dev(rows["a"])[:, None].contiguous(), dev(rows["position"])
  controller = sta.MCMCConfig(noise_level=NOISE, seed=SEED).make_controller(scene, FULL, sta.Progress(0, 2 ** 33))
  controller.points.points_in_view.copy_(dev(rows["views"]))
  torch.cuda.synchronize()
  previous = torch.cuda.get_sync_debug_mode()
  torch.cuda.set_sync_debug_mode("error")
  try:
    controller.step(sta.Progress(STEP, 2 ** 33))
  finally:
    torch.cuda.set_sync_debug_mode(previous)
  # the controller's step is the native call at (config.seed, progress.step) on the scene's own tensor
  want = _run(rows, FULL, rows["position"], rows["views"])
  assert np.array_equal(scene.points.position.cpu().numpy().view(np.uint32), want.view(np.uint32))
  assert not scene.calls


def test_misuse_is_refused(rows):
  p = torch.zeros(8, 3, device="cuda")
  args = (torch.zeros(8, 3, device="cuda"), torch.zeros(8, 4, device="cuda"), torch.zeros(8, 1, device="cuda"),
          torch.zeros(8, dtype=torch.int16, device="cuda"))
  kw = dict(min_views=5, opacity_threshold=0.1, noise_level=1.0, seed=0, step=0)
  with pytest.raises(ValueError):
    sta.mcmc_noise(p, *args[:3], args[3].to(torch.int32), **kw)
  with pytest.raises(ValueError):
    sta.mcmc_noise(torch.zeros(3, 8, device="cuda").t(), *args, **kw)          # not contiguous: cannot be updated in place
  with pytest.raises(ValueError):
    sta.mcmc_noise(p, *args, **dict(kw, seed=-1))
  with pytest.raises(sta.GsplatHipError, match="no CPU fallback"):
    sta.mcmc_noise(p.cpu(), *(t.cpu() for t in args), **kw)


# -------------------------------------------------------------------------------------------------------- training loop
PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))


def _literal_masks(state, alpha_logit, config):
  """mcmc_controller.py:76-87 with a stable sort: (split without the pruned rows, prune, overlap)."""
  opacity = torch.sigmoid(alpha_logit).squeeze(1)
  prune = (state.max_scale_px > config.max_scale_px) | (opacity < config.opacity_threshold)
  n = int(prune.sum())
  score = torch.where(prune | (state.max_scale_px < config.min_split_px), 0, state.split_score)
  split = torch.zeros_like(prune)
  split[torch.argsort(score, descending=True, stable=True)[:n]] = True
  return split & ~prune, prune, split & prune


def test_mcmc_controller_beside_an_mlp_scene():
  g, cams = synthetic.scene_b(2000, 64, 64, sh_degree=0, seed=9, num_cameras=4)
  cams = [c.to("cuda") for c in cams]
  gen = torch.Generator().manual_seed(5)
  g.alpha_logit[torch.randperm(2000, generator=gen)[:600]] = -3.0 - torch.rand(600, 1, generator=gen)   # nearly transparent
  scene_config = sta.MLPSceneConfig(parameters=PARAMETERS, reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
                                    color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=3), image_features=8,
                                    point_features=8)
  torch.manual_seed(3)
  scene = scene_config.from_color_gaussians(g, 4, "cuda", seed=3)
  targets = [torch.rand(64, 64, 3, generator=gen).cuda() for _ in cams]
  total = 45
  config = sta.MCMCConfig(prune_interval=20, min_views=2, noise_level=lambda t: 0.5 * (1.0 - t), seed=9)
  controller = config.make_controller(scene, 4000, sta.Progress(0, total))
  split_gen = torch.Generator(device="cuda").manual_seed(1)
  rounds, noise_steps, moved_total = 0, 0, 0
  for step in range(total):
    progress = sta.Progress(step, total)
    i = step % 4
    r = scene.render(cams[i], image_idx=i, compute_visibility=True, compute_point_heuristic=True)
    loss = sta.reference_loss(r.image, targets[i], ssim_levels=2) + scene.reg_loss(r)   # (64 px: two levels)
    loss.backward()
    scene.add_rendering(i, r)
    controller.add_rendering(i, r, progress)
    scene.step()
    before = scene.points.position.detach().clone()
    state = PointState(**{k: v.clone() for k, v in vars(controller.points).items()})
    n = scene.num_points
    if step % 20 == 0:
      split, prune, overlap = _literal_masks(state, scene.points.alpha_logit.detach(), config)
      keep = ~(split | prune)
      controller.step(progress, generator=split_gen)
      rounds += 1
      assert scene.num_points == n - int(overlap.sum()) == int(keep.sum()) + 2 * int(split.sum())
      kept = int(keep.sum())
      assert torch.equal(scene.points.position.detach()[:kept], before[keep])        # a prune step adds no noise
      for k, v in vars(state).items():                                                # the state is carried
        now = getattr(controller.points, k)
        assert now.shape[0] == scene.num_points and now.dtype == v.dtype
        assert torch.equal(now[:kept], v[keep]) and not now[kept:].any(), k
    else:
      controller.step(progress)
      noise_steps += 1
      assert scene.num_points == n
      moved = (scene.points.position.detach() != before).any(dim=1)
      # (a level that is far below the smallest float32 in fp64 is zero on the device whatever its libm rounds)
      level = co.gate_fp64(scene.points.alpha_logit.detach().cpu().numpy().reshape(-1)) * config.noise_level(progress.t)
      eligible = (state.points_in_view > config.min_views) & torch.from_numpy(level > 2.0 ** -160).cuda()
      assert not (moved & ~eligible).any()
      moved_total += int(moved.sum())
      for k, v in vars(state).items():
        assert torch.equal(getattr(controller.points, k), v)
  torch.cuda.synchronize()
  _note(f"mcmc loop: {rounds} prune rounds, {noise_steps} noise steps, {moved_total} row moves, {scene.num_points} points")
  assert rounds == 3 and noise_steps == 42 and moved_total > 0
  assert controller.points.points_in_view.max().item() > 20                           # carried across the rounds
  for k in ("position", "log_scaling", "rotation", "alpha_logit", "feature"):
    assert torch.isfinite(getattr(scene.points, k)).all(), k
  back = config.from_state_dict(controller.state_dict(), scene, 4000, sta.Progress(total, total))
  assert torch.equal(back.points.points_in_view, controller.points.points_in_view)


# --------------------------------------------------------------------------------------------------------------- target
def test_target_round_equals_the_cpu_masks():
  n = 4099
  config = sta.TargetConfig(prune_rate=0.025, min_split_px=20.0)
  scene = FakeScene(n, seed=2, device="cuda")
  controller = config.make_controller(scene, 6000, sta.Progress(0, 1000))
  fill_state(controller.points, 13)
  with torch.no_grad():
    controller.points.split_score[::3] = 0.5                         # ties, on both sides of the selection
  cpu = PointState(**{k: v.cpu() for k, v in vars(controller.points).items()})
  progress = sta.Progress(100, 1000)
  split, prune = find_split_prune_indexes(cpu, progress.t, controller.target_points(progress), prune_rate=0.025,
                                          min_views=5, max_scale_px=200, min_split_px=20.0)
  assert split.sum() > 100 and prune.sum() > 100
  controller.step(progress)
  assert len(scene.calls) == 1
  assert torch.equal(scene.calls[0]["keep_mask"].cpu(), ~(split | prune))
  assert torch.equal(scene.calls[0]["split_idx"].cpu(), split.nonzero().squeeze(1))
  assert scene.num_points == n + int(split.sum()) - int(prune.sum()) == controller.points.prune_cost.shape[0]
  assert controller.points.prune_cost.is_cuda and not controller.points.visibility.any()
