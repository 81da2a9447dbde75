"""The MCMC relocation on the GPU (splat_trainer_amd.controller, csrc/relocate.hip): the weighted draw against the
Python-integer oracle on every entry (tests/relocate_oracle.py), the weights and the correction inside the bounds of
tests/test_relocate_host.py, ``relocate_points`` and ``grow_points`` on a 300-row ``ParameterClass`` row by row and bit
for bit, what the correction is for -- coincident copies composite to the source's opacity -- and an
``MCMCController(relocate=True)`` beside a small ``MLPScene``.

N covers a single row, the 64-lane wave (63 / 64 / 65), the 256-row block of the prefix (257), several blocks with a tail
(1025, 4099) and more blocks than one round of the 64-way block search resolves (70001: 274 blocks)."""
import numpy as np
import pytest
import torch

import relocate_oracle as ro
import splat_trainer_amd as sta
from controller_oracle import fill_state
from splat_trainer_amd import controller as ctl, synthetic
from splat_trainer_amd.controller_math import PointState
from splat_trainer_amd.optim import ParameterClass

pytestmark = pytest.mark.gpu

PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))


def _note(line: str):
  print(line)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
  return t.detach().cpu().contiguous().view(-1).view(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- draws
def _device_draws(weights, n, seed, step, domain):
  sources, counts, total = sta.weighted_draws(_dev(weights.view(np.int32)), n, seed, step, domain)
  assert sources.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(sources.shape) == (n,)
  return sources.cpu().numpy(), counts.cpu().numpy(), int(total.item())


@pytest.mark.parametrize("N", ro.SIZES + [70001])
def test_draws_equal_the_integer_oracle(N):
  for name, weights in ro.weight_patterns(N).items():
    want_sources, want_counts, want_S = ro.draws(weights, 1000, ro.SEED, ro.STEP, 1)
    for n in ro.DRAWS:
      sources, counts, S = _device_draws(weights, n, ro.SEED, ro.STEP, 1)
      assert S == want_S, (name, n)
      assert np.array_equal(sources, want_sources[:n]), (name, n)
      assert np.array_equal(counts, np.bincount(sources, minlength=N)), (name, n)
    assert np.array_equal(counts, want_counts), name
    again = _device_draws(weights, 1000, ro.SEED, ro.STEP, 1)                  # two runs are bit-identical
    assert np.array_equal(again[0], sources) and np.array_equal(again[1], counts) and again[2] == S


def test_draws_depend_on_domain_step_and_seed_and_take_uint32():
  weights = ro.weight_patterns(1025)["random"]
  base = _device_draws(weights, 1000, ro.SEED, ro.STEP, 1)[0]
  for other in ((ro.SEED, ro.STEP, 2), (ro.SEED, ro.STEP + 1, 1), (ro.SEED + 1, ro.STEP, 1)):
    got = _device_draws(weights, 1000, *other)[0]
    assert np.array_equal(got, ro.draws(weights, 1000, *other)[0])
    assert (got != base).mean() > 0.9
  heavy = np.full(300, 2 ** 32 - 1, dtype=np.uint32)                           # weights above 2^31, as int32 bit patterns
  heavy[::3] = 7
  got = _device_draws(heavy, 1000, 5, 6, 1)
  want = ro.draws(heavy, 1000, 5, 6, 1)
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("N", [0, 1, 300])
def test_a_total_of_zero_draws_nothing(N):
  sources, counts, S = _device_draws(np.zeros(N, dtype=np.uint32), 64, ro.SEED, ro.STEP, 1)
  assert S == 0 and np.all(sources == -1) and not counts.any() and counts.shape == (N,)


def test_draw_has_no_host_wait():
  weights = _dev(ro.weight_patterns(4099)["random"].view(np.int32))
  a = torch.zeros(4099, 1, device="cuda")
  sta.weighted_draws(weights, 64, 1, 2, 1)                                     # (workspace sizes are cached by no one: warm up the allocator)
  torch.cuda.synchronize()
  previous = torch.cuda.get_sync_debug_mode()
  torch.cuda.set_sync_debug_mode("error")
  try:
    w = sta.relocate_weights(a)
    _, counts, _ = sta.weighted_draws(w, 64, 1, 2, 1)
    sta.relocate_rescale(a, torch.zeros(4099, 3, device="cuda"), counts, 0.1)
  finally:
    torch.cuda.set_sync_debug_mode(previous)


# ------------------------------------------------------------------------------------------------- weights and rescale
def test_weights_are_within_1_of_the_exact_value():
  a = np.concatenate([np.linspace(-30.0, 30.0, 1201), [-16.635532, -16.6355, 16.6, 17.0, -0.0, 1e-30]]).astype(np.float32)
  alive = np.ones(a.shape[0], dtype=bool)
  alive[::7] = False
  got = sta.relocate_weights(_dev(a)[:, None], _dev(alive)).cpu().numpy().astype(np.int64)
  want = np.array([ro.weight(x, l) for x, l in zip(a, alive)], dtype=np.int64)
  worst = int(np.abs(got - want).max())
  _note(f"device weights, {a.shape[0]} logits in [-30, 30]: max |w - oracle| = {worst}")
  assert worst <= 1
  assert np.all(got[alive] >= 1) and np.all(got[~alive] == 0) and got.max() <= 2 ** 24
  assert np.all(sta.relocate_weights(_dev(a)).cpu().numpy() >= 1)              # no mask: every row is alive


def test_rescale_stays_within_2_ulps_of_the_oracle():
  a, ls, counts = ro.rescale_grid()
  a_dev, ls_dev = _dev(a)[:, None].contiguous(), _dev(ls)
  sta.relocate_rescale(a_dev, ls_dev, _dev(counts), ro.O_FLOOR)
  a_new, ls_new = a_dev.cpu().numpy().reshape(-1), ls_dev.cpu().numpy()
  worst_a, worst_ls = ro.worst_ulps(a_new, ls_new)
  _note(f"device rescale, {int((counts > 0).sum())} rows: logit {worst_a:.3f} ulps, log-scales {worst_ls:.3f} ulps (bound {ro.ULP_BOUND})")
  assert np.isfinite(a_new).all() and np.isfinite(ls_new).all()
  assert worst_a <= ro.ULP_BOUND and worst_ls <= ro.ULP_BOUND
  idle = counts == 0
  assert np.array_equal(a_new[idle].view(np.uint32), a[idle].view(np.uint32))
  assert np.array_equal(ls_new[idle].view(np.uint32), ls[idle].view(np.uint32))
  assert np.array_equal(a_new[counts == 1000].view(np.uint32), a_new[counts == 50].view(np.uint32))
  assert np.array_equal(ls_new[counts == 1000].view(np.uint32), ls_new[counts == 50].view(np.uint32))


def test_rescale_of_sparse_rows_in_several_waves():
  """4099 rows of which every 19th has a count: the rows dealt to the lanes are the rows the loop over all rows picks."""
  rng = np.random.default_rng(8)
  n = 4099
  a, ls = rng.uniform(-6, 8, n).astype(np.float32), rng.uniform(-6, 2, (n, 3)).astype(np.float32)
  counts = np.zeros(n, dtype=np.int32)
  counts[::19] = rng.integers(1, 9, counts[::19].shape[0])
  counts[[1, 63, 64, 255, 256, 4098]] = 3
  a_dev, ls_dev = _dev(a), _dev(ls)
  sta.relocate_rescale(a_dev, ls_dev, _dev(counts), 0.05)
  a_new, ls_new = a_dev.cpu().numpy(), ls_dev.cpu().numpy()
  idle = counts == 0
  assert np.array_equal(a_new[idle].view(np.uint32), a[idle].view(np.uint32))
  assert np.array_equal(ls_new[idle].view(np.uint32), ls[idle].view(np.uint32))
  worst = 0.0
  for r in np.flatnonzero(~idle)[::7]:
    want_a, want_ls = ro.rescale(a[r], counts[r], ls[r], 0.05)
    worst = max([worst, ro.ulps(a_new[r], want_a)] + [ro.ulps(ls_new[r, j], want_ls[j]) for j in range(3)])
  _note(f"sparse rescale: {worst:.3f} ulps")
  assert worst <= ro.ULP_BOUND and np.all(a_new[~idle] != a[~idle])


# ------------------------------------------------------------------------------------------- relocate_points, grow_points
def _points(n, seed):
  g = torch.Generator().manual_seed(seed)
  tensors = dict(position=torch.randn(n, 3, generator=g), log_scaling=torch.randn(n, 3, generator=g) - 2,
                 rotation=torch.randn(n, 4, generator=g), alpha_logit=torch.randn(n, 1, generator=g) * 3,
                 feature=torch.randn(n, 8, generator=g), visible=torch.rand(n, generator=g))
  points = ParameterClass({k: v.cuda() for k, v in tensors.items()}, PARAMETERS)
  state_columns = ctl._optimizer_columns(points)
  for t in state_columns:
    t.copy_(torch.rand(t.shape, generator=g) + 0.5)                            # no zero anywhere
  return points, fill_state(PointState.new_zeros(n, "cuda"), seed + 1), state_columns


def _snapshot(points, state, state_columns):
  return ({k: t.detach().clone() for k, t in points.tensors.items()}, [t.clone() for t in state_columns],
          {k: v.clone() for k, v in vars(state).items()})


def _check_corrected(before, after, rows, counts, o_floor):
  worst = 0.0
  for r in rows:
    want_a, want_ls = ro.rescale(before["alpha_logit"][r, 0].item(), int(counts[r]), before["log_scaling"][r].cpu().numpy(), o_floor)
    worst = max([worst, ro.ulps(after["alpha_logit"][r, 0].item(), want_a)] +
                [ro.ulps(after["log_scaling"][r, j].item(), want_ls[j]) for j in range(3)])
  assert worst <= ro.ULP_BOUND
  return worst


def test_relocate_points_row_by_row():
  n, n_dead, o_floor, seed, step = 300, 37, 0.1, 11, 2 ** 33 + 50
  points, state, state_columns = _points(n, 21)
  tensors0, opt0, state0 = _snapshot(points, state, state_columns)
  dead = torch.zeros(n, dtype=torch.bool)
  dead[torch.randperm(n, generator=torch.Generator().manual_seed(4))[:n_dead]] = True
  weights = sta.relocate_weights(points.alpha_logit, ~dead.cuda()).cpu().numpy().astype(np.uint32)
  sources, counts, _ = ro.draws(weights, n_dead, seed, step, ctl.RELOCATE_DOMAIN)
  assert not dead.numpy()[sources].any() and (counts > 1).any()               # live sources, one of them drawn twice

  assert sta.relocate_points(points, state, dead.cuda(), o_floor, seed, step) == n_dead
  assert points.num_points == n and all(t.shape[0] == n for t in points.tensors.values())
  dead_rows, src = dead.nonzero().squeeze(1), torch.from_numpy(sources.astype(np.int64))
  is_source = torch.from_numpy(counts > 0)
  untouched = ~(dead | is_source)
  for k, t in points.tensors.items():
    now, was = t.detach().cpu(), tensors0[k].cpu()
    assert torch.equal(_bits(now[dead_rows]), _bits(now[src])), k               # a dead row is its source's NEW row
    assert torch.equal(_bits(now[untouched]), _bits(was[untouched])), k
    if k not in ("alpha_logit", "log_scaling"):
      assert torch.equal(_bits(now[is_source]), _bits(was[is_source])), k       # a source keeps what is not corrected
  after = {k: t.detach().cpu() for k, t in points.tensors.items()}
  worst = _check_corrected({k: v.cpu() for k, v in tensors0.items()}, after, np.flatnonzero(counts), counts, o_floor)
  _note(f"relocate_points: {int(is_source.sum())} sources corrected within {worst:.3f} ulps")
  for now, was in zip(state_columns, opt0):
    now, was = now.cpu(), was.cpu()
    assert not now[dead].any() and not now[is_source].any()                     # fresh optimizer state for both
    assert torch.equal(now[untouched], was[untouched]) and now[untouched].all()
  for k, was in state0.items():
    now = getattr(state, k).cpu()
    assert not now[dead].any() and torch.equal(now[~dead], was.cpu()[~dead]), k    # the sources keep their statistics


def test_relocate_points_with_nothing_or_everything_dead():
  points, state, state_columns = _points(70, 5)
  tensors0, opt0, state0 = _snapshot(points, state, state_columns)
  assert sta.relocate_points(points, state, torch.zeros(70, dtype=torch.bool, device="cuda"), 0.1, 1, 2) == 0
  assert sta.relocate_points(points, state, torch.ones(70, dtype=torch.bool, device="cuda"), 0.1, 1, 2) == 70
  for k, t in points.tensors.items():                                            # no live row: every source is -1, no row moves
    assert torch.equal(_bits(t), _bits(tensors0[k])), k
  assert all(torch.equal(a, b) for a, b in zip(state_columns, opt0))
  assert not any(getattr(state, k).any() for k in state0)


def test_grow_points_appends_copies_of_the_new_source_rows():
  n, n_new, o_floor, seed, step = 300, 23, 0.1, 11, 2 ** 33 + 50
  points, state, state_columns = _points(n, 22)
  tensors0, opt0, state0 = _snapshot(points, state, state_columns)
  weights = sta.relocate_weights(points.alpha_logit).cpu().numpy().astype(np.uint32)
  sources, counts, _ = ro.draws(weights, n_new, seed, step, ctl.GROW_DOMAIN)
  relocated = ro.draws(weights, n_new, seed, step, ctl.RELOCATE_DOMAIN)[0]
  assert not np.array_equal(sources, relocated)                                # growth has a stream of its own
  grown, grown_state = sta.grow_points(points, state, n_new, o_floor, seed, step)
  assert grown.num_points == n + n_new == grown_state.prune_cost.shape[0]
  src = torch.from_numpy(sources.astype(np.int64))
  is_source = torch.from_numpy(counts > 0)
  for k, t in grown.tensors.items():
    now, was = t.detach().cpu(), tensors0[k].cpu()
    assert now.shape[0] == n + n_new and (k not in PARAMETERS or t.requires_grad)
    assert torch.equal(_bits(now[n:]), _bits(now[src])), k
    assert torch.equal(_bits(now[:n][~is_source]), _bits(was[~is_source])), k
  after = {k: t.detach().cpu() for k, t in grown.tensors.items()}
  _check_corrected({k: v.cpu() for k, v in tensors0.items()}, after, np.flatnonzero(counts), counts, o_floor)
  for now, was in zip(ctl._optimizer_columns(grown), opt0):
    assert torch.equal(now[:n], was) and not now[n:].any()                       # fresh state for the appended rows
  for k, was in state0.items():
    now = getattr(grown_state, k)
    assert now.dtype == was.dtype and torch.equal(now[:n], was) and not now[n:].any(), k
  same, same_state = sta.grow_points(grown, grown_state, 0, o_floor, seed, step)
  assert same is grown and same_state is grown_state


# --------------------------------------------------------------------------------------------- what the correction is for
@pytest.mark.parametrize("copies", [2, 5])
def test_coincident_copies_composite_to_the_source_opacity(copies):
  """One Gaussian of opacity 0.6 on a pixel centre against ``copies`` coincident ones of the corrected opacity: the
  transmittance behind them at that pixel is 0.4 = (1 - o')^copies, within 16 float32 ulps of 0.4 (about copies + 2
  roundings of values no larger than 1)."""
  cam = sta.CameraParams(torch.eye(4), torch.tensor([40., 40., 20., 15.]), (40, 30)).to("cuda")
  config = sta.RasterConfig()
  logit = torch.full((1, 1), float(np.log(0.6 / 0.4)), device="cuda")
  opacity_alone = float(torch.sigmoid(logit.double()).item())
  new_logit, scales = logit.clone(), torch.zeros(1, 3, device="cuda")
  sta.relocate_rescale(new_logit, scales, torch.tensor([copies - 1], dtype=torch.int32, device="cuda"), 0.005)
  opacity_each = float(torch.sigmoid(new_logit.double()).item())

  def transmittance(n, opacity):
    g2d = torch.zeros(n, 6, device="cuda")
    g2d[:, 0], g2d[:, 1], g2d[:, 2], g2d[:, 4], g2d[:, 5] = 20.5, 15.5, 0.05, 0.05, opacity
    depth = torch.arange(1, n + 1, device="cuda", dtype=torch.float32)[:, None]
    r = sta.render_projected(torch.arange(n, device="cuda"), g2d, torch.ones(n, 1, device="cuda"), depth, cam, config)
    return float(r.final_transmittance[15, 20].item())

  ulp = float(np.spacing(np.float32(0.4)))
  alone, together = transmittance(1, opacity_alone), transmittance(copies, opacity_each)
  _note(f"{copies} copies of opacity {opacity_each:.7f}: T = {together:.9f} ({abs(together - 0.4) / ulp:.2f} ulps of 0.4); "
        f"alone {alone:.9f} ({abs(alone - 0.4) / ulp:.2f} ulps)")
  assert abs(alone - 0.4) <= 16 * ulp and abs(together - 0.4) <= 16 * ulp
  assert float(scales[0, 0]) < 0 and torch.equal(scales[0, :1].expand(3), scales[0])     # the copies shrink, all axes alike


# ----------------------------------------------------------------------------------------------------------- controller
def _scene(n, seed):
  g, _ = synthetic.scene_b(n, 64, 64, sh_degree=0, seed=seed, num_cameras=1)
  gen = torch.Generator().manual_seed(seed)
  g.alpha_logit[torch.randperm(n, generator=gen)[:n // 5]] = -3.0 - torch.rand(n // 5, 1, generator=gen)   # nearly transparent
  config = sta.MLPSceneConfig(parameters=PARAMETERS, reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
                              color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=3), image_features=8,
                              point_features=8)
  torch.manual_seed(seed)
  return config.from_color_gaussians(g, 1, "cuda", seed=seed)


def _all_bits(scene, controller):
  columns = list(scene.points.tensors.values()) + ctl._optimizer_columns(scene.points) + list(vars(controller.points).values())
  return [t.detach().clone() for t in columns]


def test_controller_relocates_grows_to_the_target_and_restarts_bit_for_bit():
  n, target, total = 500, 540, 1000
  scene = _scene(n, 6)
  config = sta.MCMCConfig(prune_interval=20, relocate=True, grow_rate=0.05, seed=9, noise_level=0.5)
  controller = config.make_controller(scene, target, sta.Progress(0, total))
  counts = []
  for step in (0, 20, 40):
    fill_state(controller.points, 30 + step)
    with torch.no_grad():
      scene.points.alpha_logit[step:step + 50] = -4.0                            # dead rows for this round
    restart_scene = scene.clone()
    restart = config.from_state_dict(controller.state_dict(), restart_scene, target, sta.Progress(step, total))
    opacity = torch.sigmoid(scene.points.alpha_logit.detach()).reshape(-1)
    dead = (controller.points.max_scale_px > config.max_scale_px) | (opacity < config.opacity_threshold)
    before = scene.num_points
    controller.step(sta.Progress(step, total))
    restart.step(sta.Progress(step, total))
    want = min(target, -(-before * 21 // 20))                                    # ceil(1.05 N)
    assert scene.num_points == want == ctl.growth_target(before, target, 0.05) == controller.num_points
    assert controller.points.prune_cost.shape[0] == want == scene.points.alpha_logit.shape[0]
    assert int(dead.sum()) >= 50
    now = torch.sigmoid(scene.points.alpha_logit.detach()).reshape(-1)
    assert (now[:before][dead] >= config.opacity_threshold - 1e-6).all()         # no copy is dead on arrival
    assert not controller.points.points_in_view[:before][dead].any() and not controller.points.points_in_view[before:].any()
    for a, b in zip(_all_bits(scene, controller), _all_bits(restart_scene, restart)):
      assert a.shape == b.shape and torch.equal(_bits(a), _bits(b))              # the restarted run repeats the same bits
    counts.append(scene.num_points)
    for k, t in scene.points.tensors.items():
      assert torch.isfinite(t).all(), k
  assert counts == [525, 540, 540]
  controller.step(sta.Progress(41, total))                                       # every other step is the noise step, unchanged
  assert scene.num_points == 540
  loss = scene.points.position.sum() + scene.points.alpha_logit.sum()            # the grown tensors are leaves that take gradients
  loss.backward()
  assert scene.points.position.grad is not None and scene.points.position.grad.shape == (540, 3)


def test_relocate_off_runs_the_prune_branch():
  scene = _scene(300, 7)
  controller = sta.MCMCConfig(prune_interval=20).make_controller(scene, 600, sta.Progress(0, 100))
  fill_state(controller.points, 3)
  split, prune = controller.find_split_prune_masks()
  controller.step(sta.Progress(0, 100))
  assert scene.num_points == 300 - int(prune.sum()) + int(split.sum())
