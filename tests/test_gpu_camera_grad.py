"""Camera gradients (dL/dT_camera_world, dL/dprojection) of the render backward pass on the GPU against fp64 autograd of the
oracle, which uses plain torch ops on both; determinism, the default path left bit for bit as it was, edge cases, and a
pose + focal refinement that recovers a perturbed camera."""
import pytest
import torch

import pose_recovery
import splat_trainer_amd as sta
from helpers import oracle, rel_err, small_scene
from splat_trainer_amd import synthetic

pytestmark = pytest.mark.gpu


def _cam_leaves(cam, device="cuda", dtype=torch.float32):
  T = cam.T_camera_world.to(device=device, dtype=dtype).clone().requires_grad_(True)
  proj = cam.projection.to(device=device, dtype=dtype).clone().requires_grad_(True)
  return T, proj, sta.CameraParams(T, proj, cam.image_size, cam.near_plane, cam.far_plane)


def _leaves(g, device="cuda"):
  return sta.Gaussians3D(*(t.clone().to(device).requires_grad_(True) for t in
                           (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))


@pytest.mark.parametrize("antialias", [False, True])
def test_project_backward_camera_matches_oracle(antialias):
  g, cams = synthetic.scene_b(20_000, 320, 240, sh_degree=0, seed=4)
  cam = cams[1]
  cfg = sta.RasterConfig(antialias=antialias, blur_cov=0.0 if antialias else 0.3)
  gd = _leaves(g)
  T, proj, camd = _cam_leaves(cam)
  g2d, depth, idx = sta.project_to_image(gd, camd, cfg)
  To = cam.T_camera_world.double().clone().requires_grad_(True)
  po = cam.projection.double().clone().requires_grad_(True)
  og, od, _ = oracle.project(g.position.double(), g.log_scaling.double(), g.rotation.double(), g.alpha_logit.double(),
                             idx.cpu(), To, po, cfg)
  torch.manual_seed(1)
  dg = torch.randn(idx.numel(), 6, dtype=torch.float64)
  dd = torch.randn(idx.numel(), 1, dtype=torch.float64)
  ((og * dg).sum() + (od * dd).sum()).backward()
  ((g2d * dg.float().cuda()).sum() + (depth * dd.float().cuda()).sum()).backward()
  assert T.grad is not None and proj.grad is not None
  assert T.grad.cpu()[3].abs().max().item() == 0
  e_T, e_p = rel_err(T.grad[:3], To.grad[:3]), rel_err(proj.grad, po.grad)
  print(f"K2 camera aa={antialias}: dT {e_T:.2e} dproj {e_p:.2e}")
  assert e_T < 1e-4 and e_p < 1e-4


@pytest.mark.parametrize("K", [1, 4, 9, 16])
def test_sh_view_direction_camera_grad(K):
  g, cams = synthetic.scene_b(20_000, 320, 240, sh_degree=int(round(K ** 0.5)) - 1, seed=5)
  cam = cams[2]
  cfg = sta.RasterConfig()
  T, proj, camd = _cam_leaves(cam)
  idx = sta.frustum_cull(g.position.cuda(), camd, cfg)
  col = sta.evaluate_sh_at(g.feature.cuda(), g.position.cuda(), idx, camd.camera_position)
  torch.manual_seed(2)
  dcol = torch.randn(idx.numel(), 3, dtype=torch.float64)
  (col * dcol.float().cuda()).sum().backward()
  if K == 1:                                 # the colour does not depend on the view direction
    assert T.grad is not None and T.grad.abs().max().item() == 0
    return
  To = cam.T_camera_world.double().clone().requires_grad_(True)
  cp = -(To[:3, :3].t() @ To[:3, 3])
  (oracle.evaluate_sh_at(g.feature.double(), g.position.double(), idx.cpu(), cp) * dcol).sum().backward()
  e = rel_err(T.grad[:3], To.grad[:3])
  print(f"SH camera K={K}: dT {e:.2e}")
  assert e < 1e-4


def _clamped_mse(image, target=0.5):
  return ((image.clamp(0, 1) - target) ** 2).mean()


def _oracle_cam_grads(g, cam, cfg, form, wide=None):
  leaves = [t.double() for t in (g.position, g.log_scaling, g.rotation, g.alpha_logit, g.feature)]
  To = cam.T_camera_world.double().clone().requires_grad_(True)
  po = cam.projection.double().clone().requires_grad_(True)
  if wide is None:
    out, *_ = oracle.render(*leaves, To, po, cam.image_size, cam.near_plane, cam.far_plane, cfg, use_sh=True)
    image = out.image
  else:
    idx = oracle.frustum_cull(leaves[0], To, po, cam.image_size, cam.near_plane, cam.far_plane,
                              cfg.margin_tiles * cfg.tile_size)
    g2d, depth, _ = oracle.project(*leaves[:4], idx, To, po, cfg)
    image = oracle.rasterize(g2d, depth, wide.double()[idx], cam.image_size, cfg).image
  _clamped_mse(image).backward()
  return To.grad, po.grad, image.detach()


def _hip_cam_grads(g, cam, cfg, form, wide=None, grad_out=False, T_dtype=torch.float32):
  gd = _leaves(g)
  T, proj, camd = _cam_leaves(cam, dtype=T_dtype)
  go = None
  if grad_out:
    bufs = [torch.zeros_like(p) for p in (gd.position, gd.log_scaling, gd.rotation, gd.alpha_logit, gd.feature)]
    go = sta.GradOut(*bufs).begin_batch()
  if form == "one":
    r = sta.render_gaussians(gd, camd, cfg, use_sh=True, grad_out=go)
  else:
    g2d, depth, idx = sta.project_to_image(gd, camd, cfg, grad_out=go)
    if wide is None:
      feats = sta.evaluate_sh_at(gd.feature, gd.position, idx, camd.camera_position,
                                 grad_out=None if go is None else (go.feature, go.position, go))
    else:
      feats = wide.cuda()[idx]
    r = sta.render_projected(idx, g2d, feats, depth, camd, cfg)
  _clamped_mse(r.image).backward()
  params = {k: getattr(gd, k).grad for k in ("position", "log_scaling", "rotation", "alpha_logit", "feature")}
  return T.grad, proj.grad, r.image.detach(), params


END_TO_END = [("one", 1), ("one", 16), ("three", 16), ("wide", 1)]


@pytest.mark.parametrize("form,K", END_TO_END)
def test_end_to_end_camera_grads_match_oracle(form, K):
  g, cam = small_scene(400, 64, 48, sh_degree=int(round(K ** 0.5)) - 1, seed=3)
  cfg = sta.RasterConfig()
  wide = None
  if form == "wide":
    wide = torch.rand(g.position.shape[0], 8, generator=torch.Generator().manual_seed(7))
  dT, dp, img, _ = _hip_cam_grads(g, cam, cfg, "three" if form == "wide" else form, wide=wide)
  oT, op, oimg = _oracle_cam_grads(g, cam, cfg, form, wide=wide)
  e_img, e_T, e_p = rel_err(img, oimg), rel_err(dT[:3], oT[:3]), rel_err(dp, op)
  print(f"end to end {form} K={K}: image {e_img:.2e} dT {e_T:.2e} dproj {e_p:.2e}")
  assert e_img < 1e-4
  assert e_T < 1e-3 and e_p < 1e-3
  if form == "three":
    oT1, op1, _, _ = _hip_cam_grads(g, cam, cfg, "one")
    assert rel_err(dT, oT1) < 1e-5 and rel_err(dp, op1) < 1e-5


@pytest.mark.parametrize("form", ["one", "three"])
def test_camera_grads_change_nothing_else_and_are_deterministic(form):
  g, cam = small_scene(400, 64, 48, sh_degree=3, seed=3)
  cfg = sta.RasterConfig()
  # camera gradients off: the default path
  gd = _leaves(g)
  camd = cam.to("cuda")
  if form == "one":
    r = sta.render_gaussians(gd, camd, cfg, use_sh=True)
  else:
    g2d, depth, idx = sta.project_to_image(gd, camd, cfg)
    r = sta.render_projected(idx, g2d, sta.evaluate_sh_at(gd.feature, gd.position, idx, camd.camera_position), depth,
                             camd, cfg)
  _clamped_mse(r.image).backward()
  base = {k: getattr(gd, k).grad for k in ("position", "log_scaling", "rotation", "alpha_logit", "feature")}
  dT1, dp1, img1, p1 = _hip_cam_grads(g, cam, cfg, form)
  dT2, dp2, img2, _ = _hip_cam_grads(g, cam, cfg, form)
  assert torch.equal(img1, r.image.detach()) and torch.equal(img1, img2)
  for k in base:
    assert torch.equal(p1[k], base[k]), k
  assert torch.equal(dT1, dT2) and torch.equal(dp1, dp2)
  # grad_out= mode: parameter gradients to the caller's buffers, the camera's through autograd
  dT3, dp3, _, _ = _hip_cam_grads(g, cam, cfg, form, grad_out=True)
  assert rel_err(dT3, dT1) < 1e-6 and rel_err(dp3, dp1) < 1e-6


def test_camera_grad_edges():
  g, cam = small_scene(400, 64, 48, sh_degree=1, seed=3)
  cfg = sta.RasterConfig()
  # a camera that sees nothing (M = 0): zeros, not None
  away = cam.T_camera_world.clone()
  away[2, 3] -= 1000.0
  for form in ("one", "three"):
    gd = _leaves(g)
    T = away.cuda().requires_grad_(True)
    proj = cam.projection.cuda().requires_grad_(True)
    camd = sta.CameraParams(T, proj, cam.image_size, cam.near_plane, cam.far_plane)
    if form == "one":
      r = sta.render_gaussians(gd, camd, cfg, use_sh=True)
    else:
      g2d, depth, idx = sta.project_to_image(gd, camd, cfg)
      r = sta.render_projected(idx, g2d, sta.evaluate_sh_at(gd.feature, gd.position, idx, camd.camera_position), depth,
                               camd, cfg)
    assert r.points.idx.numel() == 0
    (r.image.sum() + 1.0).backward()
    assert T.grad is not None and T.grad.abs().max().item() == 0, form
    assert proj.grad is not None and proj.grad.abs().max().item() == 0, form
  # N = 0
  e = sta.Gaussians3D(*(t[:0].clone().cuda().requires_grad_(True) for t in
                        (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
  T, proj, camd = _cam_leaves(cam)
  r = sta.render_gaussians(e, camd, cfg, use_sh=True)
  (r.image.sum() + 1.0).backward()
  assert T.grad is not None and T.grad.abs().max().item() == 0
  # a float64 camera gets a float64 gradient, equal to the float32 one
  dT32, dp32, _, _ = _hip_cam_grads(g, cam, cfg, "one")
  dT64, dp64, _, _ = _hip_cam_grads(g, cam, cfg, "one", T_dtype=torch.float64)
  assert dT64.dtype == torch.float64 and dp64.dtype == torch.float64
  assert torch.equal(dT64.float(), dT32) and torch.equal(dp64.float(), dp32)
  # the same CameraParams rendered and back-propagated twice
  gd = _leaves(g)
  T, proj, camd = _cam_leaves(cam)
  for _ in range(2):
    for form in ("one", "three"):
      if form == "one":
        r = sta.render_gaussians(gd, camd, cfg, use_sh=True)
      else:
        g2d, depth, idx = sta.project_to_image(gd, camd, cfg)
        r = sta.render_projected(idx, g2d, sta.evaluate_sh_at(gd.feature, gd.position, idx, camd.camera_position),
                                 depth, camd, cfg)
      _clamped_mse(r.image).backward()
  assert torch.isfinite(T.grad).all()
  assert rel_err(T.grad, 4 * dT32) < 1e-5
  # data-parallel mode refuses a learnable camera
  with pytest.raises(ValueError):
    sta.render_gaussians(_leaves(g), camd, cfg, use_sh=True, sh_collector=sta.ShFactorCollector())
  from splat_trainer_amd.distributed import CameraShardedStep
  gd = _leaves(g)
  step = CameraShardedStep([gd.position, gd.log_scaling, gd.rotation, gd.alpha_logit, gd.feature], 1, 0)
  with pytest.raises(ValueError):
    step.run([camd], lambda j, c, go, col: sta.render_gaussians(gd, c, cfg, use_sh=True, grad_out=go, sh_collector=col))


def test_pose_and_focal_recovery():
  """2 degrees, 3 % of the scene depth and 2 % of fx off; pose_recovery.STEPS Adam steps on an se(3) twist + log focal
  scale, SH degree 1.  Calibrated on the fp64 oracle with the same loop (python tests/pose_recovery.py): see
  pose_recovery.MIN_RATIO."""
  g, cam = pose_recovery.scene()
  cfg = sta.RasterConfig()
  gd = sta.Gaussians3D(*(t.clone().cuda() for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))

  def render(T, proj):
    camd = sta.CameraParams(T, proj, cam.image_size, cam.near_plane, cam.far_plane)
    return sta.render_gaussians(gd, camd, cfg, use_sh=True).image

  with torch.no_grad():
    target = render(cam.T_camera_world.cuda(), cam.projection.cuda())
  T0, proj0 = pose_recovery.perturbed_start(cam.T_camera_world, cam.projection, depth=6.0)
  start = pose_recovery.errors(T0, proj0, cam.T_camera_world, cam.projection)
  T1, proj1, losses = pose_recovery.refine(render, T0.float().cuda(), proj0.float().cuda(), target)
  end = pose_recovery.errors(T1.cpu(), proj1.cpu(), cam.T_camera_world, cam.projection)
  print("pose recovery: start", start, "end", end, "loss", losses[0], losses[-1])
  for k in start:
    assert end[k] < start[k] / pose_recovery.MIN_RATIO[k], (k, start[k], end[k])


@pytest.mark.parametrize("form", ["one", "three"])
def test_same_camera_params_after_in_place_pose_update(form):
  """The natural refinement loop: one CameraParams, its T_camera_world updated in place between renders (as an optimiser
  does).  With SH colours (K = 4) the second render must see the camera where it is now -- image, parameter and camera
  gradients as from a CameraParams built fresh from the updated pose."""
  g, cam = small_scene(400, 64, 48, sh_degree=1, seed=3)
  cfg = sta.RasterConfig()

  def run(camd, gd):
    if form == "one":
      r = sta.render_gaussians(gd, camd, cfg, use_sh=True)
    else:
      g2d, depth, idx = sta.project_to_image(gd, camd, cfg)
      r = sta.render_projected(idx, g2d, sta.evaluate_sh_at(gd.feature, gd.position, idx, camd.camera_position),
                               depth, camd, cfg)
    _clamped_mse(r.image).backward()
    return r.image.detach()

  T, proj, camd = _cam_leaves(cam)
  run(camd, _leaves(g))
  with torch.no_grad():
    T[:3, 3] += torch.tensor([0.05, -0.03, 0.1], device="cuda")
    T.grad = None
    proj.grad = None
  gd = _leaves(g)
  img = run(camd, gd)
  T2, proj2, fresh = _cam_leaves(sta.CameraParams(T.detach().cpu(), proj.detach().cpu(), cam.image_size,
                                                  cam.near_plane, cam.far_plane))
  gd2 = _leaves(g)
  img2 = run(fresh, gd2)
  assert torch.equal(img, img2)
  assert torch.equal(gd.position.grad, gd2.position.grad) and torch.equal(gd.feature.grad, gd2.feature.grad)
  assert torch.equal(T.grad, T2.grad) and torch.equal(proj.grad, proj2.grad)
