"""Pose + focal refinement loop shared by tests/test_gpu_camera_grad.py (HIP renderer) and its calibration on the CPU
oracle (``python tests/pose_recovery.py``): an se(3) twist applied on the left of the starting pose plus a log focal
scale, fitted with Adam to a target image rendered at the true camera."""
import math

import torch

STEPS = 400
LR = 1e-2             # the twist
LR_FOCAL = 3e-2       # the log focal scale (fx trades against the camera's z translation, the slow direction)
# Calibration on the fp64 oracle (python tests/pose_recovery.py), SH degree 1 so that the view-direction term takes part:
# 400 steps: rotation error 0.0349 -> 0.00023 rad (155x), translation 0.180 -> 0.0044 (41x), fx 2 % -> 0.16 % (12.7x);
# 300 steps reach only 10.7x on fx.  The test asks for 10x on each.
MIN_RATIO = dict(rotation=10.0, translation=10.0, fx=10.0)
DECAY = 0.99          # per step


def hat(xi: torch.Tensor) -> torch.Tensor:
  w, v = xi[:3], xi[3:]
  z = torch.zeros((), dtype=xi.dtype, device=xi.device)
  return torch.stack([torch.stack([z, -w[2], w[1], v[0]]), torch.stack([w[2], z, -w[0], v[1]]),
                      torch.stack([-w[1], w[0], z, v[2]]), torch.stack([z, z, z, z])])


def perturbed_start(T_true: torch.Tensor, proj_true: torch.Tensor, depth: float, seed: int = 0):
  """2 degrees about a random axis, a translation of 3 % of the scene depth, fx (and fy) 2 % off."""
  gen = torch.Generator().manual_seed(seed)
  axis = torch.nn.functional.normalize(torch.randn(3, generator=gen, dtype=torch.float64), dim=0)
  shift = torch.nn.functional.normalize(torch.randn(3, generator=gen, dtype=torch.float64), dim=0) * 0.03 * depth
  xi = torch.cat([axis * math.radians(2.0), shift])
  T0 = torch.matrix_exp(hat(xi)) @ T_true.double()
  proj0 = proj_true.double().clone()
  proj0[:2] *= 1.02
  return T0, proj0


def errors(T, proj, T_true, proj_true):
  R = T[:3, :3].double() @ T_true[:3, :3].double().t()
  angle = math.acos(max(-1.0, min(1.0, (float(R.trace()) - 1.0) / 2.0)))
  return dict(rotation=angle, translation=float((T[:3, 3].double() - T_true[:3, 3].double()).norm()),
              fx=abs(float(proj[0]) - float(proj_true[0])) / float(proj_true[0]))


def refine(render, T0: torch.Tensor, proj0: torch.Tensor, target: torch.Tensor, steps: int = STEPS):
  """render(T (4,4), proj (4,)) -> image; returns the final (T, proj) and the loss history."""
  dev, dt = target.device, T0.dtype
  xi = torch.zeros(6, dtype=dt, device=dev, requires_grad=True)
  log_f = torch.zeros((), dtype=dt, device=dev, requires_grad=True)
  opt = torch.optim.Adam([dict(params=[xi], lr=LR), dict(params=[log_f], lr=LR_FOCAL)])
  sched = torch.optim.lr_scheduler.ExponentialLR(opt, DECAY)
  scale = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=dt, device=dev)
  losses = []
  for _ in range(steps):
    T = torch.matrix_exp(hat(xi)) @ T0
    proj = proj0 * (1.0 + scale * (torch.exp(log_f) - 1.0))
    loss = ((render(T, proj) - target) ** 2).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    sched.step()
    losses.append(float(loss.detach()))
  with torch.no_grad():
    return torch.matrix_exp(hat(xi)) @ T0, proj0 * (1.0 + scale * (torch.exp(log_f) - 1.0)), losses


def scene():
  import splat_trainer_amd.synthetic as syn
  return syn.scene_a(3000, 128, 96, sh_degree=1, seed=11, sigma_px=2.5)


if __name__ == "__main__":                  # calibration on the fp64 oracle (CPU)
  import os
  import sys
  ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sys.path.insert(0, ROOT)
  import splat_trainer_amd as sta
  from oracle import torch_oracle as oracle
  g, cam = scene()
  cfg = sta.RasterConfig()
  leaves = [t.double() for t in (g.position, g.log_scaling, g.rotation, g.alpha_logit, g.feature)]

  def render(T, proj):
    out, *_ = oracle.render(*leaves, T, proj, cam.image_size, cam.near_plane, cam.far_plane, cfg, use_sh=True)
    return out.image

  with torch.no_grad():
    target = render(cam.T_camera_world.double(), cam.projection.double())
  T0, proj0 = perturbed_start(cam.T_camera_world, cam.projection, depth=6.0)
  start = errors(T0, proj0, cam.T_camera_world, cam.projection)
  T1, proj1, losses = refine(render, T0, proj0, target, steps=int(sys.argv[1]) if len(sys.argv) > 1 else STEPS)
  end = errors(T1, proj1, cam.T_camera_world, cam.projection)
  print("start", start)
  print("end  ", end)
  print("ratio", {k: start[k] / max(end[k], 1e-30) for k in start})
  print("loss", losses[0], losses[len(losses) // 2], losses[-1])
