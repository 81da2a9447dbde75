"""``MLPScene`` and the native regulariser on the GPU (splat_trainer_amd.mlp_scene / reg, csrc/reg.hip): the regulariser
against its fp64 restatement (tests/mlp_scene_oracle.py) over visible and invisible rows, bit-reproducibility, the absence
of a host synchronisation, the scene's render + reg_loss flow against the colour-model oracle flow, the post-step
projection, a short training run with one densify round and a save / load, and the SH export."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import color_model_oracle as cmo
import mlp_scene_oracle as mso
import splat_trainer_amd as sta
from helpers import oracle, rel_err, small_scene
from splat_trainer_amd import ply_io, reg, synthetic
from splat_trainer_amd.controller_math import PointState, find_split_prune_indexes

pytestmark = pytest.mark.gpu

# Derived, not measured: each row is a handful of fp32 operations with exp and one division (a few ulp, about 1e-6
# relative), all summands are non-negative, and a tree reduction over M <= 1e5 rows adds at most about 17 ulp.
REG_TOL = 1e-5
WEIGHTS = dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5)
FLOW_TOL = 5e-2                                         # tests/test_gpu_color_model.py: set by the f16 MFMA colour model


def _note(line: str):
  """Every figure is printed before it is asserted (run with -s to keep them)."""
  print(line)


# ---------------------------------------------------------------------------------------------------- regulariser
def _stack_scene():
  """Rows of a projected small scene behind a stack of 40 nearly opaque splats that covers part of the image (as the
  saturating stack of tests/test_gpu_render.py:125-138): the stack's tail and the scene's splats behind it are culled
  rows that never reach a pixel.  -> g2d (M, 6), depth (M, 1), features (M, 3), camera, config; all on the CPU."""
  g, cam = small_scene(1500, 160, 120, sh_degree=0, seed=5, sigma_px=2.5)
  cfg = sta.RasterConfig(compute_visibility=True)
  with torch.no_grad():
    gd = sta.Gaussians3D(*(t.cuda() for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
    g2d_s, depth_s, _ = sta.project_to_image(gd, cam.to("cuda"), cfg)
  n = 40
  stack = torch.zeros(n, 6)
  stack[:, 0], stack[:, 1] = 60., 50.
  stack[:, 2], stack[:, 4] = 4e-3, 4e-3                # sigma ~ 16 px
  stack[:, 5] = 0.97
  depth = torch.cat([0.5 + 0.01 * torch.arange(n, dtype=torch.float32)[:, None], depth_s.cpu()])
  g2d = torch.cat([stack, g2d_s.cpu()])
  feats = torch.rand(g2d.shape[0], 3, generator=torch.Generator().manual_seed(2))
  return g2d, depth, feats, cam, cfg


def _reg_inputs(variant: str):
  g2d, depth, feats, cam, cfg = _stack_scene()
  M = g2d.shape[0]
  out = oracle.rasterize(g2d, depth, feats, cam.image_size, cfg)
  # on the ORACLE's visibility: both classes of rows exist, so the mask is exercised whatever the code under test does
  n_vis = int((out.visibility > 0).sum())
  assert 0 < n_vis < M, (n_vis, M)
  gen = torch.Generator().manual_seed(7)
  N = 3 * M
  idx = torch.randperm(N, generator=gen)[:M].sort().values.cuda()
  g2d = g2d.cuda().requires_grad_(True)
  depth = depth.cuda().requires_grad_(True)
  specular = (0.3 * torch.randn(M, 3, generator=gen)).cuda().requires_grad_(True)
  log_scaling = (-3 + 0.5 * torch.randn(N, 3, generator=gen)).cuda().requires_grad_(True)
  r = sta.render_projected(idx, g2d, feats.cuda(), depth, cam.to("cuda"), cfg)
  points = r.points
  assert rel_err(points.visibility, out.visibility) < 1e-4
  if variant != "no_specular":
    points = points.replace(attributes=sta.Colors(torch.zeros_like(specular), specular))
  if variant == "none_visible":
    points = points.replace(visibility=torch.zeros_like(points.visibility))
  return points, g2d, depth, specular, log_scaling


def _native_reg(points, leaves, weights, weighted):
  for t in leaves:
    t.grad = None
  loss, terms = sta.reg_loss(points, leaves[-1], weights, visibility_weighted=weighted, return_terms=True)
  loss.backward()
  torch.cuda.synchronize()
  g2d, depth, specular, log_scaling = leaves
  return dict(loss=loss.detach(), terms=terms, d_opacity=g2d.grad[:, 5].clone(), d_depths=depth.grad.clone(),
              d_specular=None if specular.grad is None else specular.grad.clone(),
              d_log_scaling=log_scaling.grad.clone())


def _oracle_reg(points, leaves, weights, weighted, with_specular):
  g2d, depth, specular, log_scaling = leaves
  o = g2d.detach()[:, 5].double().cpu().requires_grad_(True)
  d = depth.detach().double().cpu().requires_grad_(True)
  s = specular.detach().double().cpu().requires_grad_(True) if with_specular else None
  ls = log_scaling.detach().double().cpu().requires_grad_(True)
  loss, terms, count = mso.reg_loss(points.idx.cpu(), o, d, s, points.visibility.detach().double().cpu(), ls, weights, weighted)
  loss.backward()
  return dict(loss=loss.detach(), terms=torch.stack([terms[k].detach() for k in mso.TERMS]), count=count, d_opacity=o.grad,
              d_depths=d.grad, d_specular=None if s is None else s.grad, d_log_scaling=ls.grad)


@pytest.mark.parametrize("variant", ["weighted", "unweighted", "no_specular", "zero_weight", "none_visible"])
def test_regulariser_matches_the_fp64_restatement(variant):
  points, *leaves = _reg_inputs(variant)
  weights = dict(WEIGHTS, aspect=0.0) if variant == "zero_weight" else WEIGHTS
  weighted = variant != "unweighted"
  with_specular = variant != "no_specular"
  got = _native_reg(points, leaves, weights, weighted)
  want = _oracle_reg(points, leaves, weights, weighted, with_specular)
  assert int(got["terms"][4].item()) == want["count"]
  for t in got.values():
    if t is not None:
      assert torch.isfinite(t).all()
  if variant == "none_visible":
    assert want["count"] == 0 and got["loss"].item() == 0.0 and got["terms"].abs().max().item() == 0.0
    for k in ("d_opacity", "d_depths", "d_specular", "d_log_scaling"):
      assert got[k].abs().max().item() == 0.0, k
    return
  assert want["count"] > 0
  errs = dict(loss=rel_err(got["loss"], want["loss"]))
  for i, k in enumerate(mso.TERMS):
    if k == "specular" and not with_specular:
      assert got["terms"][i].item() == 0.0
      continue
    errs[k] = rel_err(got["terms"][i], want["terms"][i])
  for k in ("d_opacity", "d_depths", "d_specular", "d_log_scaling"):
    if want[k] is None:
      assert got[k] is None
      continue
    errs[k] = rel_err(got[k], want[k])
  _note(f"reg parity [{variant}] count {want['count']} of {points.idx.shape[0]}: " +
        "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
  for k, e in errs.items():
    assert e < REG_TOL, (variant, k, e)
  # masked rows get exact zeros, and rows of log_scaling that idx does not name are untouched
  masked = ~(points.visibility > 0)
  assert got["d_opacity"][masked].abs().max().item() == 0.0 and got["d_depths"][masked].abs().max().item() == 0.0
  rows = torch.ones(leaves[-1].shape[0], dtype=torch.bool, device="cuda")
  rows[points.idx[~masked]] = False
  assert got["d_log_scaling"][rows].abs().max().item() == 0.0
  if variant == "zero_weight":
    # the aspect term is still reported, only dropped from the loss
    assert got["terms"][2].item() > 0


def test_regulariser_without_rows():
  dev = "cuda"
  e = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
  opacity, depths, spec = e(0).requires_grad_(True), e(0, 1).requires_grad_(True), e(0, 3).requires_grad_(True)
  points = sta.RenderedPoints(idx=e(0, dt=torch.int64), depths=depths, opacity=opacity, screen_scale=e(0, 2),
                              visibility=e(0), prune_cost=e(0), split_score=e(0),
                              attributes=sta.Colors(torch.zeros_like(spec), spec))
  ls = torch.randn(10, 3, device=dev).requires_grad_(True)
  loss, terms = sta.reg_loss(points, ls, WEIGHTS, return_terms=True)
  loss.backward()
  assert loss.item() == 0.0 and terms.abs().max().item() == 0.0
  assert ls.grad.abs().max().item() == 0.0 and opacity.grad.shape == (0,) and depths.grad.shape == (0, 1)


def test_regulariser_is_bit_reproducible():
  points, *leaves = _reg_inputs("weighted")
  a = _native_reg(points, leaves, WEIGHTS, True)
  b = _native_reg(points, leaves, WEIGHTS, True)
  for k in a:
    assert torch.equal(a[k], b[k]), k


def _torch_form(points_visible, log_scaling_all):
  """tests/test_gpu_dropin_flow.py:38-46: the regulariser as a user writes it with torch today."""
  scale = torch.exp(log_scaling_all[points_visible.idx])
  norm_scale = scale.pow(2).sum(1) / points_visible.depths.pow(2).squeeze(-1)
  opacity_term = mso.saturate(points_visible.opacity, gain=4.0, k=2.0) * norm_scale
  aspect = scale.max(1).values / scale.min(1).values
  w = points_visible.visibility
  return 0.1 * (norm_scale * w).mean() + 1.0 * (opacity_term * w).mean() + 0.01 * (aspect * w).mean()


def test_regulariser_makes_no_host_sync():
  points, *leaves = _reg_inputs("weighted")
  points.visibility                                     # resolved before the guarded region
  torch.cuda.synchronize()
  previous = torch.cuda.get_sync_debug_mode()
  torch.cuda.set_sync_debug_mode("error")
  try:
    loss = sta.reg_loss(points, leaves[-1], WEIGHTS)
    loss.backward()
    # the torch form goes through points.visible, i.e. nonzero(): that is the synchronisation being removed
    with pytest.raises(RuntimeError):
      _torch_form(points.visible, leaves[-1])
  finally:
    torch.cuda.set_sync_debug_mode(previous)
  torch.cuda.synchronize()
  assert math.isfinite(loss.item())


# ------------------------------------------------------------------------------------------------------ scene flow
PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))
CM_L, CM_S = 1, 5


def _config(**over):
  kw = dict(parameters=PARAMETERS, reg_weight=WEIGHTS,
            color_model=sta.ColorModelConfig(hidden_layers=CM_L, sh_degree=CM_S, lr_diffuse=1e-2, lr_specular=1e-2),
            lr_glo_feature=0.1, image_features=32, point_features=16)
  kw.update(over)
  return sta.MLPSceneConfig(**kw)


def _scene(g, num_images, seed, config=None):
  torch.manual_seed(seed)                               # the colour model's initial weights
  scene = (config or _config()).from_color_gaussians(g, num_images, "cuda", seed=seed)
  with torch.no_grad():
    gen = torch.Generator().manual_seed(seed + 100)
    scene.color_table.weight.copy_(0.5 * torch.randn(scene.color_table.weight.shape, generator=gen))
  return scene


def test_scene_flow_matches_the_oracle_flow():
  """MLPScene.render + an image loss + MLPScene.reg_loss + backward against the flow of
  tests/test_gpu_color_model.py:286-310 run with the colour-model restatement and the regulariser's restatement."""
  g, cam = synthetic.scene_a(3000, 160, 120, sh_degree=0, seed=3, sigma_px=2.5)
  camc = cam.to("cuda")
  scene = _scene(g, 2, seed=5)
  r = scene.render(camc, image_idx=1, compute_visibility=True)
  assert isinstance(r.points.attributes, sta.Colors) and r.image.shape == (120, 160, 3)
  assert 0 < r.points.num_visible
  loss = (r.image - 0.3).pow(2).mean() + scene.reg_loss(r)
  loss.backward()
  torch.cuda.synchronize()
  pts = scene.points
  names = [k for k, _ in scene.color_model.named_parameters()]
  got = dict(position=pts.position.grad, log_scaling=pts.log_scaling.grad, rotation=pts.rotation.grad,
             alpha_logit=pts.alpha_logit.grad, point_features=pts.feature.grad, glo=scene.color_table.weight.grad[1:2],
             **{f"colour.{k}": p.grad for k, p in scene.color_model.named_parameters()})
  assert scene.color_table.weight.grad[0].abs().max().item() == 0.0

  # the oracle flow on clones of the same parameters
  leaf = lambda t: t.detach().clone().requires_grad_(True)
  gd = sta.Gaussians3D(position=leaf(pts.position), rotation=leaf(pts.rotation), log_scaling=leaf(pts.log_scaling),
                       alpha_logit=leaf(pts.alpha_logit), feature=leaf(pts.feature))
  glo = leaf(scene.color_table.weight[1:2])
  params = {k: leaf(v) for k, v in scene.color_model.state_dict().items()}
  cfg = sta.RasterConfig(compute_visibility=True)
  g2d, depth, idx = sta.project_to_image(gd, camc, cfg)
  d, s = cmo.forward(params, gd.feature[idx], gd.position[idx], camc.camera_position, glo, CM_L, CM_S)
  colours = sta.Colors(d, s)
  ro = sta.render_projected(idx, g2d, colours.total(), depth, camc, cfg)
  po = ro.points
  oreg, _, _ = mso.reg_loss(po.idx, po.opacity, po.depths, s, po.visibility, gd.log_scaling, WEIGHTS, True)
  oloss = (ro.image[..., :3].clamp(0, 1) - 0.3).pow(2).mean() + oreg
  oloss.backward()
  torch.cuda.synchronize()
  want = dict(position=gd.position.grad, log_scaling=gd.log_scaling.grad, rotation=gd.rotation.grad,
              alpha_logit=gd.alpha_logit.grad, point_features=gd.feature.grad, glo=glo.grad,
              **{f"colour.{k}": params[k].grad for k in names})
  assert abs(loss.item() - oloss.item()) < FLOW_TOL * abs(oloss.item())
  for k in want:
    e = rel_err(got[k], want[k])
    _note(f"scene flow {k}: {e:.2e}")
    assert e < FLOW_TOL, (k, e)

  # the regulariser alone reaches alpha_logit, and only through points.opacity
  scene.zero_grad()
  r2 = scene.render(camc, image_idx=1, compute_visibility=True)
  scene.reg_loss(r2).backward()
  assert pts.alpha_logit.grad.abs().max().item() > 0
  scene.zero_grad()
  r3 = scene.render(camc, image_idx=1, compute_visibility=True)
  sta.reg_loss(r3.points.replace(opacity=r3.points.opacity.detach()), pts.log_scaling, WEIGHTS).backward()
  assert pts.alpha_logit.grad is None or pts.alpha_logit.grad.abs().max().item() == 0.0


def test_render_uses_a_zero_glo_vector_outside_the_training_images():
  g, cam = synthetic.scene_a(2000, 128, 96, sh_degree=0, seed=4, sigma_px=2.5)
  camc = cam.to("cuda")
  scene = _scene(g, 3, seed=9)
  with torch.no_grad():
    none = scene.render(camc).image
    one = scene.render(camc, image_idx=1).image
    scene.set_training_images([0, 2])
    held_out = scene.render(camc, image_idx=1).image
  assert torch.equal(none, held_out) and not torch.equal(none, one)


def test_unsupported_colour_model_surfaces_its_error():
  g, _ = synthetic.scene_a(100, 64, 48, sh_degree=0, seed=4)
  with pytest.raises(ValueError, match="supported: hidden_features = 32"):
    _config(color_model=sta.ColorModelConfig(hidden_features=64)).from_color_gaussians(g, 2, "cuda", seed=0)


# -------------------------------------------------------------------------------------------------------- post-step
def _ulp(t: torch.Tensor) -> torch.Tensor:
  a = t.abs()
  return torch.nextafter(a, torch.full_like(a, math.inf)) - a


def test_post_step_projection(monkeypatch):
  g, cam = synthetic.scene_a(3000, 160, 120, sh_degree=0, seed=3, sigma_px=2.5)
  camc = cam.to("cuda")
  scene = _scene(g, 2, seed=5)
  pts = scene.points
  with torch.no_grad():
    pts.position[:100, 2] = -5.0                        # behind the camera: never culled in, never visible
    pts.log_scaling[:20] = -8.3                         # of those, rows that only the clamp moves
    pts.log_scaling[20:30, 0] = -9.0
    pts.rotation[:500] *= 3.0                           # not unit length
  r = scene.render(camc, image_idx=0, compute_visibility=True)
  ((r.image - 0.3).pow(2).mean() + scene.reg_loss(r)).backward()
  scene.add_rendering(0, r)
  seen = pts.visible > 0
  assert 0 < int(seen.sum()) < scene.num_points
  before = {k: pts.tensors[k].detach().clone() for k in ("position", "log_scaling", "alpha_logit", "feature")}
  captured = {}
  native = reg.scene_post_step

  def spy(rotation, log_scaling, *a, **kw):
    captured["rotation"], captured["log_scaling"] = rotation.clone(), log_scaling.clone()
    return native(rotation, log_scaling, *a, **kw)

  monkeypatch.setattr(reg, "scene_post_step", spy)
  scene.step()
  torch.cuda.synchronize()
  assert torch.equal(pts.log_scaling.detach(), captured["log_scaling"].clamp_(-8, 8))
  assert pts.log_scaling.min().item() == -8.0
  want = F.normalize(captured["rotation"], dim=1)
  diff = (pts.rotation.detach() - want).abs()
  assert bool((diff <= 2 * _ulp(want)).all()), (diff / _ulp(want)).max().item()
  assert (pts.rotation.detach().norm(dim=1) - 1).abs().max().item() < 1e-6
  assert pts.visible.abs().max().item() == 0.0
  for k in ("position", "log_scaling", "rotation", "alpha_logit", "feature"):
    grad = pts.tensors[k].grad
    assert grad is None or grad.abs().max().item() == 0.0, k
  for p in list(scene.color_model.parameters()) + [scene.color_table.weight]:
    assert p.grad is None or p.grad.abs().max().item() == 0.0
  unseen = ~seen
  assert bool(unseen[:100].all())
  for k in ("position", "alpha_logit", "feature"):
    assert torch.equal(pts.tensors[k].detach()[unseen], before[k][unseen]), k
  assert torch.equal(pts.log_scaling.detach()[unseen], before["log_scaling"][unseen].clamp(-8, 8))
  assert torch.equal(pts.log_scaling.detach()[30:100], before["log_scaling"][30:100])
  moved = (pts.position.detach()[seen] != before["position"][seen]).any(dim=1)
  assert bool(moved.any())


def test_post_step_kernel_on_edge_rows():
  rot = torch.randn(1000, 4, device="cuda")
  rot[0] = 0                                            # F.normalize: 0 / eps = 0
  rot[1] = 1e-20
  ls = 20 * torch.randn(1000, 3, device="cuda")
  ls[2, 0] = float("nan")
  want_rot, want_ls = F.normalize(rot, dim=1), ls.clone().clamp_(-8, 8)
  reg.scene_post_step(rot, ls)
  assert torch.equal(ls.nan_to_num(123.0), want_ls.nan_to_num(123.0)) and bool(torch.isnan(ls[2, 0]))
  assert bool(((rot - want_rot).abs() <= 2 * _ulp(want_rot)).all())


# ----------------------------------------------------------------------------- train, densify, save, load, export
STEPS, DENSIFY_AT = 60, 30
LOSS_RATIO_SEEN = 0.155         # end / start of the run below as first measured (profiles/r10_mlp_scene.txt)


def _psnr(a, b):
  return -10.0 * math.log10(max(F.mse_loss(a, b).item(), 1e-12))


@pytest.fixture(scope="module")
def trained():
  g, cams = synthetic.scene_b(4000, 160, 120, sh_degree=0, seed=9, num_cameras=8)
  cams = [c.to("cuda") for c in cams]
  teacher = _scene(g, 8, seed=21)
  with torch.no_grad():
    targets = [teacher.render(c, image_idx=i).image.contiguous() for i, c in enumerate(cams)]
  scene = _scene(g, 8, seed=22)
  n0 = scene.num_points
  state = PointState.new_zeros(n0, "cuda")
  gen = torch.Generator(device="cuda").manual_seed(3)
  losses, expect_n = [], None
  for step in range(STEPS):
    i = step % 8
    r = scene.render(cams[i], image_idx=i, compute_visibility=True, compute_point_heuristic=True)
    loss = sta.reference_loss(r.image, targets[i]) + scene.reg_loss(r)
    loss.backward()
    scene.add_rendering(i, r)
    state.add_rendering(r)
    scene.step()
    losses.append(loss.item())
    if step + 1 == DENSIFY_AT:
      split_mask, prune_mask = find_split_prune_indexes(state, (step + 1) / STEPS, int(1.1 * n0))
      keep_mask = ~(split_mask | prune_mask)
      n_split, n_keep = int(split_mask.sum()), int(keep_mask.sum())
      assert n_split > 0 and n_keep < n0
      expect_n = n_keep + 2 * n_split
      scene.split_and_prune(keep_mask, split_mask.nonzero().squeeze(1), generator=gen)
      state = PointState.new_zeros(scene.num_points, "cuda")
  return dict(scene=scene, cams=cams, targets=targets, losses=losses, n0=n0, expect_n=expect_n)


def test_train_densify_save_load(trained):
  scene, cams, losses = trained["scene"], trained["cams"], trained["losses"]
  start, end = sum(losses[:8]) / 8, sum(losses[-8:]) / 8        # one pass over the 8 cameras each
  _note(f"train: {STEPS} steps, loss (mean over 8 cameras) start {start:.4f} end {end:.4f} ratio {end / start:.3f}; "
        f"points {trained['n0']} -> {scene.num_points}")
  assert end < start
  assert end / start < 1.0 - 0.5 * (1.0 - LOSS_RATIO_SEEN)      # half of the drop first seen
  assert scene.num_points == trained["expect_n"] and scene.num_points != trained["n0"]
  assert scene.points.visible.shape[0] == scene.num_points
  sta.check_finite(scene.gaussians, "gaussians")
  sta.check_finite(dict(scene.color_model.state_dict()), "color_model")
  state = scene.state_dict()
  assert sorted(state) == ["color_model", "color_opt", "color_table", "glo_opt", "points"]
  loaded = scene.config.from_state_dict(state, 8)
  with torch.no_grad():
    for i in (0, 5):
      assert torch.equal(scene.render(cams[i], image_idx=i).image, loaded.render(cams[i], image_idx=i).image)
  # the copy shares nothing: a step of the original leaves it alone
  assert loaded.points.position.data_ptr() != scene.points.position.data_ptr()


def _hand_written_transfer(scene, cams, epochs):
  """The flow of tests/test_gpu_dropin_flow.py::test_transfer_sh_flow fed this scene's colours."""
  positions = scene.points.position.detach()
  n = positions.shape[0]
  base_sh = torch.nn.Parameter(torch.randn(n, 3, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)))
  higher_sh = torch.nn.Parameter(torch.zeros(n, 3, 8, device="cuda"))
  opt = torch.optim.Adam([dict(params=[base_sh], lr=0.1), dict(params=[higher_sh], lr=0.01, weight_decay=1e-4)],
                         betas=(0.9, 0.999))
  sh0 = 0.282094791773878
  for _ in range(epochs):
    for i, cam in enumerate(cams):
      opt.zero_grad()
      idx, vis = scene.query_visibility(cam)
      with torch.no_grad():
        colors = scene.color_model.post_activation(scene.eval_colors(idx, cam, i).total())
      with torch.enable_grad():
        pred = sta.evaluate_sh_at(torch.cat([base_sh, higher_sh], dim=2), positions, idx, cam.camera_position).clamp(0, 1)
        mse = F.mse_loss(pred, colors, reduction="none")
        rgb = F.l1_loss((base_sh.squeeze(2) * sh0 + 0.5)[idx], colors)
        v = vis.unsqueeze(1)
        loss = (mse * v).sum() / v.sum() + 0.1 * rgb
        loss.backward()
      opt.step()
  return torch.cat([base_sh, higher_sh], dim=2).detach()


def test_export_to_sh_gaussians(trained, tmp_path):
  scene, cams = trained["scene"], trained["cams"]
  epochs = 6
  exported = scene.to_sh_gaussians(cams, list(range(8)), epochs=epochs, sh_degree=2,
                                   generator=torch.Generator().manual_seed(0))
  assert exported.feature.shape == (scene.num_points, 3, 9)
  path = tmp_path / "scene.ply"
  ply_io.write_gaussians(path, exported.to("cpu"), with_sh=True)
  back = ply_io.read_gaussians(path, with_sh=True).to("cuda")
  assert torch.equal(back.feature.cpu(), exported.feature.cpu())
  by_hand = sta.Gaussians3D(position=back.position, rotation=back.rotation, log_scaling=back.log_scaling,
                            alpha_logit=back.alpha_logit, feature=_hand_written_transfer(scene, cams, epochs))
  got, ref = [], []
  with torch.no_grad():
    for i, cam in enumerate(cams):
      want = scene.render(cam, image_idx=i).image
      got.append(_psnr(sta.render_gaussians(back, cam, use_sh=True).image.clamp(0, 1), want))
      ref.append(_psnr(sta.render_gaussians(by_hand, cam, use_sh=True).image.clamp(0, 1), want))
  psnr, psnr_ref = sum(got) / 8, sum(ref) / 8
  _note(f"export: PSNR of the SH export against MLPScene.render {psnr:.2f} dB; hand-written transfer flow {psnr_ref:.2f} dB "
        f"({epochs} epochs, 8 cameras)")
  assert psnr > psnr_ref - 1.0
