"""Depth fusion on the host: the shim (libgsr_hostmath.so, the arithmetic of csrc/gsr_fusion.h compiled for the CPU) and
the package's CPU path against tests/fusion_oracle.py, bit for bit.  The cases are in tests/fusion_cases.py;
tests/test_gpu_fusion.py runs the same ones on the device."""
import numpy as np
import pytest
import torch

import fusion_cases as cases
import fusion_oracle as oracle
import hostmath
import splat_trainer_amd as sta
from splat_trainer_amd import fusion


@pytest.fixture(scope="module")
def backend(built_libs):
  return cases.HostBackend(hostmath.load(built_libs))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_case(backend, name):
  cases.CASES[name](backend)


def test_the_vote_one_double_beyond_the_bound(backend):
  """On doubles: zs (1 +- 2^-7) agrees, the next double above violates, the next double below is occluded."""
  zs = np.array([0.5, 1.0, 2.0, 8.0, 64.0, 1024.0])
  tol = 2.0 ** -7
  hi, lo = zs * (1 + tol), zs * (1 - tol)
  rows = [(hi, 1), (lo, 1), (np.nextafter(hi, np.inf), 2), (np.nextafter(lo, 0), 0), (np.nextafter(hi, 0), 1),
          (np.nextafter(lo, np.inf), 1), (np.full(6, np.nan), 0), (np.full(6, np.inf), 0), (-zs, 0), (np.zeros(6), 0)]
  for ds, expected in rows:
    out = np.full(6, -1, np.int32)
    backend.shim.hm_fuse_votes(np.ascontiguousarray(ds), zs, 6, np.array([tol]), out)
    assert out.tolist() == [expected] * 6, (ds, out)


def test_voxel_keys_are_the_oracles(backend):
  rng = np.random.default_rng(3)
  pts = np.concatenate([rng.normal(0, 50, (500, 3)), [[np.nan, 3e7, -3e7], [0.0, -0.0, 1e-45]]]).astype(np.float32)
  keys = np.zeros(len(pts), np.uint64)
  backend.shim.hm_voxel_keys(pts, len(pts), np.array([0.25, 1.0, -2.0, 0.5]), keys)
  assert keys.tolist() == oracle.voxel_keys(pts, 0.25, (1.0, -2.0, 0.5))


def test_the_pose_helpers_are_the_oracles():
  rng = np.random.default_rng(4)
  a, b = cases.pose(rng, 0.8, 3.0), cases.pose(rng, 0.8, 3.0)
  assert np.array_equal(fusion.rigid_inverse(oracle.pose(a)), oracle.rigid_inverse(oracle.pose(a)))
  assert np.array_equal(fusion.compose(oracle.pose(a), oracle.pose(b)), oracle.compose(oracle.pose(a), oracle.pose(b)))
  back = oracle.compose(oracle.pose(a), oracle.rigid_inverse(oracle.pose(a)))
  assert np.abs(back - np.eye(3, 4)).max() < 1e-6                              # (a float32 rotation is orthogonal to ~1e-7)


def test_select_sources():
  def cam(x, yaw):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[np.cos(yaw), 0, -np.sin(yaw)], [0, 1, 0], [np.sin(yaw), 0, np.cos(yaw)]]
    T[:3, 3] = -T[:3, :3] @ np.array([x, 0, 0], np.float32)
    return cases.camera(T, [10, 10, 5, 5], 10, 10)
  cams = [cam(0.0, 0.0), cam(1.0, 0.0), cam(-1.0, 0.0), cam(0.5, 2.0), cam(3.0, 0.3)]      # 3 looks away
  got = sta.select_sources(cams, 2)
  assert got == [[1, 2], [0, 2], [0, 1], [], [1, 0]]                      # 2 and 4 tie for view 1: the lower index
  assert sta.select_sources(cams, 0) == [[], [], [], [], []]
  assert sta.select_sources(cams, 9)[0] == [1, 2, 4]


def test_arguments_are_checked():
  depth = torch.ones(4, 5)
  cam = cases.camera(np.eye(4), [5, 5, 2.5, 2], 4, 5)
  with pytest.raises(ValueError):
    sta.depth_consistency(depth.double(), cam, [], 0.01)
  with pytest.raises(ValueError):
    sta.depth_consistency(depth, cases.camera(np.eye(4), [5, 5, 2.5, 2], 5, 4), [], 0.01)
  with pytest.raises(ValueError):
    sta.depth_consistency(depth, cam, [(depth, cam)], float("nan"))
  with pytest.raises(ValueError):
    sta.voxel_downsample(torch.zeros(3, 3), torch.zeros(3, 3, dtype=torch.uint8), 0.0)
  with pytest.raises(ValueError):
    sta.voxel_downsample(torch.zeros(3, 3), torch.zeros(3, 3, dtype=torch.uint8), 1.0, (0.0, float("inf"), 0.0))
  with pytest.raises(ValueError):
    sta.fuse_depth_maps([depth], None, [cam, cam])
  assert sta.depth_consistency(depth, cam, [], 0.01).sum() == 0


def test_transform_cloud_and_fuse_scene_on_the_host():
  """fuse_scene with a render function, and Normalization.transform_cloud on its result."""
  depths, images, cams = cases.plane_views()
  cameras = [cases.camera(T, proj, d.shape[0], d.shape[1], near) for (T, proj, near), d in zip(cams, depths)]

  def render(camera, idx):
    return sta.Rendering(image=torch.from_numpy(images[idx]), camera=camera, points=None,
                         median_depth_image=torch.from_numpy(depths[idx]))
  config = sta.FusionConfig(min_agree=1, num_sources=2)
  cloud, agree = sta.fuse_scene(render, cameras, config)
  want = cases.oracle_fusion(depths, images, cams, sta.select_sources(cameras, 2), 0.01, 1, 0)
  cases.check_fusion((cloud, agree), want)
  norm = sta.Normalization(config=None, translation=torch.tensor([1.0, -2.0, 0.5]), scaling=2.0)
  moved = norm.transform_cloud(cloud)
  assert torch.equal(moved.points, 2.0 * (cloud.points + torch.tensor([1.0, -2.0, 0.5]))) and moved.colors is cloud.colors
  assert torch.equal(norm.inverse.transform_cloud(moved).points, (moved.points * 0.5) + torch.tensor([-1.0, 2.0, -0.5]))
