"""The direct SH export fit on the GPU (splat_trainer_amd.sh_fit, csrc/sh_fit.hip) against tests/sh_fit_oracle.py: the
coefficients of well-sampled points against the fp64 oracle, the objective of sparsely sampled ones against the oracle's
minimum -- both bounded by four times the float32 restatement's own distance from the oracle, measured on the CPU on
these same scenes (test_sh_fit_host.py) -- the rows a view does not list, the weights, unseen points, determinism, the
argument checks, and ``MLPScene.to_sh_gaussians(method="lstsq")`` against ``method="adam"`` on the views both were given.
Every figure is printed before it is asserted (run with -s to keep them: profiles/r18_sh_fit.txt holds that output)."""
import functools

import numpy as np
import pytest
import torch

import sh_fit_oracle as so
import splat_trainer_amd as sta
from splat_trainer_amd import mlp_scene, sh_fit, synthetic

pytestmark = pytest.mark.gpu

BOUND_COEF, BOUND_J = so.MARGIN * so.RESTATEMENT_COEF, so.MARGIN * so.RESTATEMENT_J
CASES = [(N, degree) for N in so.SIZES for degree in range(4)]


def _note(line: str):
  print(line)


def _device_fit(scene: so.Scene, degree: int) -> sta.ShFit:
  fit = sta.ShFit(torch.from_numpy(scene.positions).cuda(), sh_degree=degree)
  for camera, (idx, colours, weights) in zip(scene.cameras, scene.views):
    fit.add_view(torch.from_numpy(idx).cuda(), torch.from_numpy(colours).cuda(), torch.from_numpy(weights).cuda(),
                 torch.from_numpy(camera).cuda())
  return fit


@functools.lru_cache(maxsize=None)
def _coefficient_case(N, degree):
  scene = so.coefficient_scene(N, degree)
  return scene, so.normal_equations(scene, (degree + 1) ** 2)


@pytest.mark.parametrize("N,degree", CASES)
def test_coefficients_of_well_sampled_points(N, degree):
  scene, eq = _coefficient_case(N, degree)
  fit = _device_fit(scene, degree)
  want_weight = so.weight_fp64(scene)
  assert fit.acc.shape == (N, so.row_doubles((degree + 1) ** 2)) and fit.acc.dtype == torch.float64
  assert fit.acc[:, -1].cpu().numpy().tobytes() == want_weight.tobytes()
  for ridge in (so.MIN_RIDGE, so.DEFAULT_RIDGE):
    sh, weight = fit.solve(ridge)
    assert sh.shape == (N, 3, (degree + 1) ** 2) and sh.dtype == torch.float32 and weight.shape == (N,)
    err = float(np.max(np.abs(sh.cpu().numpy() - so.solve(eq, ridge))))
    _note(f"coefficients N={N} degree={degree} ridge={ridge:g}: max |s - oracle| = {err:.2e} (bound {BOUND_COEF:.2e})")
    assert err <= BOUND_COEF
    assert weight.cpu().numpy().tobytes() == want_weight.astype(np.float32).tobytes()
    unseen = torch.from_numpy(scene.unseen).cuda()
    assert bool((sh[unseen] == 0).all()) and bool((weight[unseen] == 0).all())
    assert int((weight == 0).sum()) == len(scene.unseen)


@pytest.mark.parametrize("N,degree", CASES)
def test_objective_of_sparsely_sampled_points(N, degree):
  K = (degree + 1) ** 2
  for V in (1, 2, 8):
    scene = so.few_view_scene(V, N, degree)
    s, eq = so.fit_fp64(scene, K, so.DEFAULT_RIDGE)
    sh, weight = _device_fit(scene, degree).solve(so.DEFAULT_RIDGE)
    got = sh.cpu().numpy()
    excess = float(so.relative_excess(scene, eq, s, got, so.DEFAULT_RIDGE).max())
    _note(f"objective N={N} degree={degree} V={V}: {int((eq.W > 0).sum())} points seen, max relative excess of J = "
          f"{excess:.2e} (bound {BOUND_J:.2e})")
    assert np.isfinite(got).all()
    assert excess <= BOUND_J
    assert (got[eq.W == 0] == 0).all()
    assert weight.cpu().numpy().tobytes() == so.weight_fp64(scene).astype(np.float32).tobytes()


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_rows_outside_the_view_are_not_touched(degree):
  N = 1000
  scene = so.few_view_scene(2, N, degree)
  idx, colours, weights = scene.views[0]
  fit = sta.ShFit(torch.from_numpy(scene.positions).cuda(), sh_degree=degree)
  gen = torch.Generator().manual_seed(degree)
  sentinel = torch.randn(fit.acc.shape, generator=gen, dtype=torch.float64).view(torch.int64)     # every mantissa bit in use
  fit.acc.view(torch.int64).copy_(sentinel)
  fit.add_view(torch.from_numpy(idx).cuda(), torch.from_numpy(colours).cuda(), torch.from_numpy(weights).cuda(),
               torch.from_numpy(scene.cameras[0]).cuda())
  after = fit.acc.view(torch.int64).cpu()
  listed = torch.zeros(N, dtype=torch.bool)
  listed[torch.from_numpy(idx)] = True
  assert 0 < int(listed.sum()) < N
  assert torch.equal(after[~listed], sentinel[~listed])
  changed = (after[listed] != sentinel[listed]).float().mean().item()
  _note(f"untouched rows degree={degree}: {int((~listed).sum())} rows bit-identical; {changed:.3f} of the listed rows' words changed")
  assert changed > 0.9


def test_indexes_outside_the_points_are_skipped():
  scene = so.few_view_scene(2, 257, 2)
  idx, colours, weights = scene.views[0]
  bad = idx.copy()
  bad[0], bad[-1] = -1, 257
  pos, cam = torch.from_numpy(scene.positions).cuda(), torch.from_numpy(scene.cameras[0]).cuda()
  a, b = sta.ShFit(pos, 2), sta.ShFit(pos, 2)
  a.add_view(torch.from_numpy(bad).cuda(), torch.from_numpy(colours).cuda(), torch.from_numpy(weights).cuda(), cam)
  b.add_view(torch.from_numpy(idx[1:-1]).cuda(), torch.from_numpy(colours[1:-1]).cuda(),
             torch.from_numpy(weights[1:-1]).cuda(), cam)
  assert torch.equal(a.acc, b.acc)


def test_two_fits_of_the_same_views_are_bit_identical():
  scene = so.few_view_scene(8, 4099, 3)
  a, b = _device_fit(scene, 3), _device_fit(scene, 3)
  assert torch.equal(a.acc, b.acc)
  for x, y in zip(a.solve(so.DEFAULT_RIDGE), b.solve(so.DEFAULT_RIDGE)):
    assert torch.equal(x, y)
  again = a.solve(so.DEFAULT_RIDGE)                       # the solve leaves the accumulators alone
  assert torch.equal(again[0], b.solve(so.DEFAULT_RIDGE)[0]) and torch.equal(a.acc, b.acc)


def test_small_ridge_raises_and_an_empty_view_changes_nothing():
  scene = so.few_view_scene(2, 65, 1)
  fit = _device_fit(scene, 1)
  before = fit.acc.clone()
  for ridge in (0.0, 1e-7, -1.0, float("nan"), float("inf")):
    with pytest.raises(ValueError, match="ridge"):
      fit.solve(ridge)
    with pytest.raises(ValueError, match="ridge"):
      sta.fit_sh(None, None, [], [], fit.positions, ridge=ridge)
  empty = torch.empty(0, device="cuda")
  fit.add_view(torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, 3, device="cuda"), empty,
               torch.zeros(3, device="cuda"))
  assert torch.equal(fit.acc, before)
  nothing = sta.ShFit(fit.positions, 1)
  sh, weight = nothing.solve()
  assert bool((sh == 0).all()) and bool((weight == 0).all())
  with pytest.raises(TypeError, match="int64"):
    fit.add_view(torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, 3, device="cuda"),
                 torch.zeros(2, device="cuda"), torch.zeros(3, device="cuda"))
  with pytest.raises(ValueError, match="expected"):
    fit.add_view(torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(3, 3, device="cuda"),
                 torch.zeros(2, device="cuda"), torch.zeros(3, device="cuda"))
  with pytest.raises(sta.GsplatHipError, match="HIP device only"):
    fit.add_view(torch.zeros(2, dtype=torch.int64), torch.zeros(2, 3, device="cuda"), torch.zeros(2, device="cuda"),
                 torch.zeros(3, device="cuda"))
  assert torch.equal(fit.acc, before)


# -------------------------------------------------------------------------------------------------------------- scene
PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))


def _trained_scene():
  g, cams = synthetic.scene_b(400, 64, 48, sh_degree=0, seed=9, num_cameras=8)
  cams = [c.to("cuda") for c in cams]
  config = sta.MLPSceneConfig(parameters=PARAMETERS, reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
                              color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=3), image_features=8,
                              point_features=8)
  torch.manual_seed(5)                                   # the colour model's initial weights
  scene = config.from_color_gaussians(g, 8, "cuda", seed=5)
  with torch.no_grad():
    scene.color_table.weight.copy_(0.5 * torch.randn(scene.color_table.weight.shape, generator=torch.Generator().manual_seed(6)))
  for step in range(4):
    r = scene.render(cams[step], image_idx=step, compute_visibility=True)
    ((r.image - 0.3).pow(2).mean() + scene.reg_loss(r)).backward()
    scene.add_rendering(step, r)
    scene.step()
  return scene, cams


def test_scene_export_by_least_squares_is_optimal_on_its_views():
  scene, cams = _trained_scene()
  N, image_indexes = scene.num_points, list(range(8))
  positions = scene.points.position.detach()
  recorded = []

  def plain_colors(idx, cam, image_idx):
    with torch.no_grad():
      return scene.color_model.post_activation(scene.eval_colors(idx, cam, image_idx).total())

  def eval_colors(idx, cam, image_idx):
    colors = plain_colors(idx, cam, image_idx)
    recorded[-1] += (colors,)
    return colors

  def query_visibility(cam):
    idx, visibility = scene.query_visibility(cam)
    recorded.append((cam, idx, visibility))
    return idx, visibility

  half = [mlp_scene.resized_camera(c, 0.5) for c in cams]
  direct, weight = sta.fit_sh(eval_colors, query_visibility, half, image_indexes, positions, sh_degree=2)
  views = [v for v in recorded if len(v) == 4]
  assert len(recorded) == 8 and len(views) >= 6
  exported = scene.to_sh_gaussians(cams, image_indexes, sh_degree=2, method="lstsq")
  assert exported.feature.shape == (N, 3, 9) and bool(torch.isfinite(exported.feature).all())
  assert torch.equal(exported.feature, direct) and not exported.feature.requires_grad
  assert torch.equal(exported.position, positions)
  assert torch.equal(scene.evaluate_sh_features(cams, image_indexes, method="lstsq", ridge=sh_fit.DEFAULT_RIDGE), direct)

  adam = scene.to_sh_gaussians(cams, image_indexes, epochs=1, sh_degree=2, generator=torch.Generator().manual_seed(0))
  by_hand = mlp_scene.transfer_sh(plain_colors, scene.query_visibility, half,
                                  image_indexes, positions, epochs=1, sh_degree=2,
                                  generator=torch.Generator().manual_seed(0))
  assert torch.equal(adam.feature, by_hand)
  assert torch.equal(adam.feature, scene.to_sh_gaussians(cams, image_indexes, 1, 2, torch.Generator().manual_seed(0),
                                                         method="adam").feature)

  fitted = so.Scene(positions.cpu().numpy(), np.stack([v[0].camera_position.cpu().numpy() for v in views]),
                    [(v[1].cpu().numpy(), v[3].cpu().numpy(), v[2].cpu().numpy()) for v in views], None, None)
  for idx, _, _ in fitted.views:
    assert len(np.unique(idx)) == len(idx)
  eq = so.normal_equations(fitted, 9)
  seen = eq.W > 0
  assert weight.cpu().numpy().tobytes() == so.weight_fp64(fitted).astype(np.float32).tobytes()
  assert bool((direct[torch.from_numpy(~seen).cuda()] == 0).all())
  s, _ = so.fit_fp64(fitted, 9, so.DEFAULT_RIDGE)
  excess = float(so.relative_excess(fitted, eq, s, direct.cpu().numpy(), so.DEFAULT_RIDGE).max())
  gap = so.relative_gap(fitted, eq, direct.cpu().numpy(), adam.feature.cpu().numpy(), so.DEFAULT_RIDGE)
  J_l = so.objective(fitted, direct.cpu().numpy(), so.DEFAULT_RIDGE)[seen].sum()
  J_a = so.objective(fitted, adam.feature.cpu().numpy(), so.DEFAULT_RIDGE)[seen].sum()
  _note(f"scene: {int(seen.sum())} of {N} points seen in {len(views)} views; lstsq against the oracle's minimum: max relative "
        f"excess of J = {excess:.2e} (bound {BOUND_J:.2e}); lstsq against adam: max relative gap {gap[seen].max():.2e} "
        f"(at most {BOUND_J:.2e}), sum of J lstsq {J_l:.4e}  adam {J_a:.4e}")
  assert excess <= BOUND_J
  assert gap[seen].max() <= BOUND_J
