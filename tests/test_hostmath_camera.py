"""CPU checks of the camera terms of the K2 backward (csrc/gsr_math.h: gsr_project_one_bwd<true>, gsr_fold_camera_position)
through the host build of the shared maths header: dL/dT_camera_world and dL/dprojection against fp64 autograd of the
oracle, which uses plain torch ops on both."""
import numpy as np
import pytest
import torch

import hostmath
from helpers import oracle, small_scene
from splat_trainer_amd import RasterConfig
from splat_trainer_amd._lib import raster_params

TOL = 2e-4          # as test_hostmath.py: relative to the largest entry of the reference


def _np(t):
  return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))


def _rel(got, want):
  want = np.asarray(want, np.float64)
  return np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max()


@pytest.mark.parametrize("antialias", [False, True])
def test_camera_terms_match_autograd(built_libs, antialias):
  lib = hostmath.load(built_libs)
  g, cam = small_scene(2000, 96, 64, seed=23, sigma_px=3.0)
  cfg = RasterConfig(antialias=antialias, blur_cov=0.0 if antialias else 0.3)
  M = g.position.shape[0]
  torch.manual_seed(5)
  dg = torch.randn(M, 6, dtype=torch.float64)
  dd = torch.randn(M, 1, dtype=torch.float64)
  T = cam.T_camera_world.double().clone().requires_grad_(True)
  proj = cam.projection.double().clone().requires_grad_(True)
  og, od, _ = oracle.project(g.position.double(), g.log_scaling.double(), g.rotation.double(), g.alpha_logit.double(),
                             torch.arange(M), T, proj, cfg)
  ((og * dg).sum() + (od * dd).sum()).backward()

  per_splat = np.zeros((M, 16), np.float32)
  rp = raster_params(cfg)
  lib.hm_project_backward_camera(_np(cam.T_camera_world), _np(cam.projection), rp, M, _np(g.position),
                                 _np(g.log_scaling), _np(g.rotation), _np(g.alpha_logit), _np(dg), _np(dd[:, 0]),
                                 per_splat)
  total = per_splat.astype(np.float64).sum(0)
  dT, dproj = T.grad.numpy(), proj.grad.numpy()
  assert np.all(dT[3] == 0)
  assert _rel(total[:12].reshape(3, 4), dT[:3]) < TOL, (antialias, total[:12], dT[:3])
  assert _rel(total[12:], dproj) < TOL, (antialias, total[12:], dproj)


@pytest.mark.parametrize("K", [4, 16])
def test_camera_position_fold_matches_autograd(built_libs, K):
  """The view-direction term: dL/dcam from autograd of evaluate_sh_at, folded through cam = -R^T t by the shim, equals
  autograd straight through T."""
  lib = hostmath.load(built_libs)
  g, cam = small_scene(500, 96, 64, sh_degree=int(round(K ** 0.5)) - 1, seed=24)
  assert g.feature.shape[2] == K
  M = g.position.shape[0]
  torch.manual_seed(6)
  dcol = torch.randn(M, 3, dtype=torch.float64)
  sh, pos = g.feature.double(), g.position.double()

  T = cam.T_camera_world.double().clone().requires_grad_(True)
  cam_pos = -(T[:3, :3].t() @ T[:3, 3])
  (oracle.evaluate_sh_at(sh, pos, torch.arange(M), cam_pos) * dcol).sum().backward()

  leaf = (-(cam.T_camera_world.double()[:3, :3].t() @ cam.T_camera_world.double()[:3, 3])).requires_grad_(True)
  (oracle.evaluate_sh_at(sh, pos, torch.arange(M), leaf) * dcol).sum().backward()

  dT = np.zeros(12, np.float32)
  lib.hm_fold_camera_position(_np(cam.T_camera_world), _np(leaf.grad), dT)
  assert _rel(dT.reshape(3, 4), T.grad.numpy()[:3]) < TOL, (K, dT, T.grad)
