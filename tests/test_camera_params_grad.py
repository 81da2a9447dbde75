"""CPU checks of CameraParams.camera_position with a learnable pose: never cached, so that it follows in-place updates of
T_camera_world (what an optimiser does) in and out of grad mode, and carries no graph from one render into the next."""
import torch

from splat_trainer_amd import CameraParams


def _cam(requires_grad):
  T = torch.eye(4)
  T[:3, 3] = torch.tensor([1.0, 2.0, 3.0])
  return CameraParams(T.requires_grad_(requires_grad), torch.tensor([50.0, 50.0, 32.0, 24.0]), (64, 48))


def test_camera_position_follows_in_place_pose_updates():
  cam = _cam(True)
  for grad_mode in (False, True, False):
    with torch.set_grad_enabled(grad_mode):
      first = cam.camera_position.detach().clone()
    with torch.no_grad():
      cam.T_camera_world[:3, 3] += 1.0
    with torch.set_grad_enabled(grad_mode):
      again = cam.camera_position
    assert torch.equal(again.detach(), first - 1.0), (grad_mode, first, again)


def test_camera_position_carries_a_fresh_graph_each_time():
  cam = _cam(True)
  for _ in range(2):
    cam.camera_position.sum().backward()          # a cached graph would fail the second time
  assert torch.equal(cam.T_camera_world.grad[:3, 3], torch.full((3,), -2.0))


def test_fixed_pose_is_still_cached():
  cam = _cam(False)
  assert cam.camera_position is cam.camera_position
