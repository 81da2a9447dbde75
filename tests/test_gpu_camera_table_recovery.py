"""A CameraRigTable recovers a perturbed rig pose through the native pose kernels and the HIP renderer: the loop of
tests/camera_table_recovery.py, calibrated there on the fp64 oracles."""
import pytest
import torch

import camera_table_oracle as co
import camera_table_recovery as rec
import pose_recovery
import splat_trainer_amd as sta

pytestmark = pytest.mark.gpu


def test_rig_pose_recovery_through_the_table():
  g, cam = pose_recovery.scene()
  cfg = sta.RasterConfig()
  gd = sta.Gaussians3D(*(t.clone().cuda() for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
  camera_t_rig, true, start = rec.rig()
  w, h = cam.image_size
  projection = sta.Projections(intrinsics=cam.projection.repeat(2, 1), image_size=torch.tensor([[w, h]] * 2),
                               depth_range=torch.tensor([[cam.near_plane, cam.far_plane]] * 2))
  names, labels = [f"frame{i // 2}_cam{i % 2}" for i in range(4)], torch.full((4,), sta.Label.Training.value)
  truth = sta.CameraRigTable(true.float(), camera_t_rig.float(), projection, names, labels).cuda()
  table = sta.CameraRigTable(start.float(), camera_t_rig.float(), projection, names, labels).cuda()
  image_idx = torch.tensor([2 * rec.FRAME, 2 * rec.FRAME + 1])

  def render(T, i):
    return sta.render_gaussians(gd, sta.CameraParams(T, projection.intrinsics[i].cuda(), cam.image_size, cam.near_plane,
                                                     cam.far_plane), cfg, use_sh=True).image

  with torch.no_grad():
    true_cameras = truth(image_idx)
    targets = [render(true_cameras.camera_t_world[i], i) for i in range(2)]
  poses = table._camera_poses
  poses.normalize()
  before = {k: v.clone() for k, v in table.state_dict().items()}
  q, t = poses.rig_t_world.q.requires_grad_(True), poses.rig_t_world.t.requires_grad_(True)

  def pose_error():
    # the trained rows' pose evaluated in fp64: errors() takes the angle from acos of a trace, which on a float32 matrix
    # resolves no finer than sqrt(2 * 2^-24) = 3.5e-4 rad
    return rec.errors(co.pose(q.detach().cpu().double(), t.detach().cpu().double())[rec.FRAME], true[rec.FRAME])

  begin = pose_error()
  losses = rec.refine(q, t, lambda: table(image_idx).camera_t_world, poses.normalize, render, targets)
  sta.check_indices()
  end = pose_error()
  print("rig recovery: start", begin, "end", end, "loss", losses[0], losses[-1], "asked", rec.MIN_RATIO)
  for k in begin:
    assert rec.MIN_RATIO[k] >= 1.0 and end[k] < begin[k] / rec.MIN_RATIO[k], (k, begin[k], end[k])
  after = table.state_dict()
  other = 1 - rec.FRAME
  assert torch.equal(after["_camera_poses.rig_t_world.q"][other], before["_camera_poses.rig_t_world.q"][other])
  assert torch.equal(after["_camera_poses.rig_t_world.t"][other], before["_camera_poses.rig_t_world.t"][other])
  assert not torch.equal(after["_camera_poses.rig_t_world.q"][rec.FRAME], before["_camera_poses.rig_t_world.q"][rec.FRAME])
  for key in ("_camera_poses.camera_t_rig.q", "_camera_poses.camera_t_rig.t", "_camera_projection.intrinsics", "_labels"):
    assert torch.equal(after[key], before[key]), key
