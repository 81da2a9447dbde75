"""``COLMAPDataset(..., undistort=True)`` on the host (``device="cpu"``: the shim does the remap and the resize) on the
directory of tests/colmap_scene.py with its cameras swapped for a SIMPLE_RADIAL and an OPENCV one: projections against
the optimal pinholes times the scale, images against oracle remap then oracle area resize, a PINHOLE directory the same
with either setting, and the refusal that stays."""
import numpy as np
import pytest
import torch

import colmap_scene as cs
import image_oracle as io
import splat_trainer_amd as sta
import undistort_oracle as uo
from splat_trainer_amd import colmap_io as cio

# camera id -> the distorted camera of that id's size (64 x 48 and 50 x 40), in COLMAP's convention
DISTORTED = {3: cio.Camera("SIMPLE_RADIAL", 64, 48, np.array([60.0, 31.8, 24.1, -0.2])),
             8: cio.Camera("OPENCV", 50, 40, np.array([48.0, 49.0, 25.3, 19.6, 0.15, 0.04, -0.004, 0.003]))}


def write_distorted(path):
  """The directory of colmap_scene.write with both cameras distorted: (cameras, images, points, pixels)."""
  _, images, points, pixels = cs.write(path)
  cio.write_model(path / "sparse" / "0", DISTORTED, images, points)
  return DISTORTED, images, points, pixels


def expected_view(camera):
  """(target with centres at integers, map) of a distorted COLMAP camera, the map by the oracle."""
  lens = sta.LensCamera.from_colmap(camera)
  target = sta.optimal_pinhole(lens)
  m = uo.undistort_map(lens.source_array(), target, lens.height, lens.width, lens.height, lens.width)
  return target, m


@pytest.fixture(scope="module")
def scene(tmp_path_factory, built_libs):
  path = tmp_path_factory.mktemp("colmap_distorted")
  return (path,) + write_distorted(path)


@pytest.mark.parametrize("scale", [dict(), dict(image_scale=0.5), dict(resize_longest=37)],
                         ids=["full", "image_scale", "resize_longest"])
def test_projections_and_images(scene, scale):
  path, cameras, images, points, pixels = scene
  ds = sta.COLMAPDataset(path, device="cpu", test_every=4, undistort=True, **scale)
  views = {}
  for k, (camera_id, cam) in enumerate(sorted(cameras.items())):
    target, m = expected_view(cam)
    views[camera_id] = m
    s, (w, h) = cs.scaled_size(cam.width, cam.height, **scale) if scale else (1.0, (cam.width, cam.height))
    colmap_k = np.array([target[0], target[1], target[2] + 0.5, target[3] + 0.5])
    assert ds.projections.image_size[k].tolist() == [w, h]
    assert torch.equal(ds.projections.intrinsics[k], torch.tensor(colmap_k * s, dtype=torch.float32))
    assert ds.undistortions[k].target == tuple(target)
  for view, im in zip(ds.load_images(), images):
    cam = cameras[im.camera_id]
    _, (w, h) = cs.scaled_size(cam.width, cam.height, **scale) if scale else (1.0, (cam.width, cam.height))
    want = io.resize_area(uo.remap(pixels[im.image_id][None], views[im.camera_id]), h, w)[0]
    assert tuple(view.image.shape) == (h, w, 3) and np.array_equal(view.image.numpy(), want)


def test_the_views_sample_inside_the_source(scene):
  """No zero border: every entry of both maps lies inside the source, so the images differ from the source's only by
  the resampling."""
  for cam in scene[1].values():
    _, m = expected_view(cam)
    assert m.min() >= 0 and m[..., 0].max() <= 32 * (cam.width - 1) and m[..., 1].max() <= 32 * (cam.height - 1)


def test_a_pinhole_directory_loads_identically_with_either_setting(tmp_path, built_libs):
  cs.write(tmp_path)
  a = sta.COLMAPDataset(tmp_path, device="cpu", image_scale=0.5)
  b = sta.COLMAPDataset(tmp_path, device="cpu", image_scale=0.5, undistort=True)
  assert b.undistortions == [None, None]
  assert torch.equal(a.projections.intrinsics, b.projections.intrinsics)
  assert torch.equal(a.projections.image_size, b.projections.image_size)
  for x, y in zip(a.load_images(), b.load_images()):
    assert torch.equal(x.image, y.image)


def test_refusals(scene, tmp_path, built_libs):
  with pytest.raises(ValueError, match="SIMPLE_RADIAL.*undistorted"):
    sta.COLMAPDataset(scene[0], device="cpu")                                  # undistort=False: as before
  with pytest.raises(ValueError, match="SIMPLE_RADIAL.*undistorted"):
    sta.COLMAPDataset(scene[0], device="cpu", undistort=False)
  cs.write(tmp_path, bad_camera=cio.Camera("FULL_OPENCV", 64, 48, np.array([60.0, 60.0, 32.0, 24.0] + [0.0] * 8)))
  with pytest.raises(ValueError, match="FULL_OPENCV"):
    sta.COLMAPDataset(tmp_path, device="cpu", undistort=True)
