"""The lens undistortion on the host (the shim of csrc/gsr_undistort.h, and splat_trainer_amd.undistort on "cpu") against
the numpy oracle (tests/undistort_oracle.py): the map int32 for int32 at every shape, the remap byte for byte at every
hand-made map with 1 and 3 channels and 1 and 3 images, the optimal pinhole by the two properties that define it, the
short-circuit without distortion, a folding distortion, and ``LensCamera.from_colmap``."""
import numpy as np
import pytest
import torch

import hostmath
import splat_trainer_amd as sta
import undistort_oracle as uo
from splat_trainer_amd import colmap_io as cio


def lens(name, **over):
  H, W, (fx, fy, cx, cy), (k1, k2, k3, p1, p2) = uo.CAMERAS[name]
  return sta.LensCamera(**{**dict(width=W, height=H, fx=fx, fy=fy, cx=cx, cy=cy, k1=k1, k2=k2, p1=p1, p2=p2, k3=k3), **over})


@pytest.mark.parametrize("case", list(uo.MAP_CASES))
def test_shim_map_equals_oracle(built_libs, case):
  name, target, (Hd, Wd) = uo.MAP_CASES[case]
  H, W, _, _ = uo.CAMERAS[name]
  got = np.full((Hd, Wd, 2), 12345, np.int32)
  code = hostmath.load(built_libs).hm_undistort_map(uo.source_array(name), np.array(target, np.float64), H, W, Hd, Wd, got)
  want = uo.case_map(case)
  assert code == 0 and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} entries differ"
  # the package's host path is the same call
  assert np.array_equal(sta.undistort_map(lens(name), target, (Hd, Wd)).numpy(), want)


def test_own_K_of_the_pincushion_samples_outside(built_libs):
  m = uo.case_map("pincushion-own-K")
  assert (m[..., 0] < 0).any() and (m[..., 0] > 32 * 63).any() and (m[..., 1] < 0).any() and (m[..., 1] > 32 * 47).any()
  assert m.min() >= -32 and m[..., 0].max() <= 32 * 64 and m[..., 1].max() <= 32 * 48          # the clamp


def test_non_finite_coordinates_become_minus_one(built_libs):
  shim = hostmath.load(built_libs)
  source = np.array([60.0, 61.0, 31.3, 23.6, 1e300, 1e300, 0.0, 0.0, 1e300])     # overflows to inf - inf away from the centre
  target = np.array([1e-3, 1e-3, 5.0, 5.0])
  got = np.zeros((11, 11, 2), np.int32)
  assert shim.hm_undistort_map(source, target, 48, 64, 11, 11, got) == 0
  with np.errstate(over="ignore", invalid="ignore"):
    want = uo.undistort_map(source, target, 48, 64, 11, 11)
  assert np.array_equal(got, want) and (want == -32).any()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("case", uo.REMAP_IDS)
def test_shim_remap_equals_oracle(built_libs, case, C, B):
  (Hs, Ws), m = uo.remap_cases()[case]
  src, want = uo.remap_reference(case, C, B)
  got = np.full(want.shape, 0xA5, np.uint8)
  code = hostmath.load(built_libs).hm_image_remap_u8(np.array(src), B, Hs, Ws, C, m, got, m.shape[0], m.shape[1])
  assert code == 0 and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"


def test_identity_map_copies_and_package_remap_takes_three_dimensions(built_libs):
  (Hs, Ws), m = uo.remap_cases()["identity"]
  src, want = uo.remap_reference("identity", 3, 1)
  assert np.array_equal(want, src)
  got = sta.remap(torch.from_numpy(np.array(src[0])), torch.from_numpy(m))
  assert tuple(got.shape) == (Hs, Ws, 3) and np.array_equal(got.numpy(), src[0])
  with pytest.raises(ValueError, match="uint8"):
    sta.remap(torch.zeros((4, 4, 3)), torch.from_numpy(m))
  with pytest.raises(ValueError, match="1 or 3 channels"):
    sta.remap(torch.zeros((4, 4, 2), dtype=torch.uint8), torch.from_numpy(m))
  with pytest.raises(ValueError, match="int32"):
    sta.remap(torch.zeros((4, 4, 3), dtype=torch.uint8), torch.from_numpy(m).long())


def test_empty_source_gives_zeros(built_libs):
  m = torch.from_numpy(uo.remap_cases()["identity"][1])
  out = sta.remap(torch.zeros((2, 0, 5, 3), dtype=torch.uint8), m)
  assert tuple(out.shape) == (2, 48, 64, 3) and not out.any()


@pytest.mark.parametrize("name", list(uo.CAMERAS))
def test_optimal_pinhole_lies_inside_and_reaches_every_side(built_libs, name):
  """Every quantised border entry of the view lies in [0, 32 (S - 1)], and on each side some entry comes within one
  pixel (32 units) of the source's border: inside, and no smaller than it has to be."""
  H, W, _, _ = uo.CAMERAS[name]
  target = sta.optimal_pinhole(lens(name))
  uv = uo.border(W, H)
  m = uo.map_points(uo.source_array(name), target, H, W, uv[:, 0], uv[:, 1])
  print(name, target, m[:, 0].min(), m[:, 0].max(), m[:, 1].min(), m[:, 1].max())
  assert m.min() >= 0 and m[:, 0].max() <= 32 * (W - 1) and m[:, 1].max() <= 32 * (H - 1)
  assert m[:, 0].min() <= 32 and m[:, 0].max() >= 32 * (W - 2) and m[:, 1].min() <= 32 and m[:, 1].max() >= 32 * (H - 2)
  und = sta.Undistortion(lens(name), target)
  assert und.target == tuple(target)


def test_zero_coefficients_give_the_source_K_and_the_identity_map(built_libs):
  cam = lens("barrel", k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0)
  assert sta.optimal_pinhole(cam) == (60.0, 61.0, 31.3, 23.6)
  und = sta.Undistortion(cam)
  assert und.target == (60.0, 61.0, 31.3, 23.6)
  assert np.array_equal(und.map.numpy(), uo.remap_cases()["identity"][1])
  image = torch.from_numpy(uo.make_input(2, 48, 64, 3))
  assert torch.equal(und(image), image)
  with pytest.raises(ValueError, match="the camera is 64 x 48"):
    und(image[:, :40])


def test_a_folding_distortion_raises(built_libs):
  with pytest.raises(ValueError, match="folds"):
    sta.optimal_pinhole(lens("barrel", k1=-2.0))


def test_from_colmap_parameter_orders_and_the_half_pixel():
  L = sta.LensCamera
  assert L.from_colmap(cio.Camera("SIMPLE_RADIAL", 64, 48, np.array([60.0, 32.0, 24.0, 0.01]))) == \
      L(64, 48, 60.0, 60.0, 31.5, 23.5, k1=0.01)
  assert L.from_colmap(cio.Camera("RADIAL", 64, 48, np.array([60.0, 32.0, 24.0, 0.01, -0.02]))) == \
      L(64, 48, 60.0, 60.0, 31.5, 23.5, k1=0.01, k2=-0.02)
  assert L.from_colmap(cio.Camera("OPENCV", 64, 48, np.array([60.0, 61.0, 32.0, 24.0, 0.01, -0.02, 0.003, -0.004]))) == \
      L(64, 48, 60.0, 61.0, 31.5, 23.5, k1=0.01, k2=-0.02, p1=0.003, p2=-0.004)
  assert L.from_colmap(cio.Camera("PINHOLE", 64, 48, np.array([60.0, 61.0, 32.0, 24.0]))) == L(64, 48, 60.0, 61.0, 31.5, 23.5)
  assert L.from_colmap(cio.Camera("SIMPLE_PINHOLE", 64, 48, np.array([60.0, 32.0, 24.0]))) == L(64, 48, 60.0, 60.0, 31.5, 23.5)
  assert not L(64, 48, 60.0, 61.0, 31.5, 23.5).distorted and L(64, 48, 60.0, 61.0, 31.5, 23.5, p2=1e-9).distorted
  for model, n in (("FULL_OPENCV", 12), ("OPENCV_FISHEYE", 8), ("SIMPLE_RADIAL_FISHEYE", 4), ("FOV", 5)):
    with pytest.raises(ValueError, match=model):
      L.from_colmap(cio.Camera(model, 64, 48, np.zeros(n)))
