"""gsr_undistort_map and gsr_image_remap_u8 on the GPU against the numpy oracle (tests/undistort_oracle.py): the map
int32 for int32 at every shape of the list the host test runs, the remap byte for byte at every hand-made map with 1 and
3 channels and 1 and 3 images; unaligned pointers with a fill around dst; bit-identical repeats; B = 0; ``Undistortion``
on a device tensor against the host; and ``COLMAPDataset(..., undistort=True)`` on the device against the host path."""
import numpy as np
import pytest
import torch

import splat_trainer_amd as sta
import undistort_oracle as uo
from splat_trainer_amd import _lib
from test_colmap_undistort_host import write_distorted
from test_undistort_host import lens

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(uo.MAP_CASES))
def test_map_equals_oracle(built_libs, case):
  name, target, size = uo.MAP_CASES[case]
  got, want = sta.undistort_map(lens(name), target, size, device="cuda").cpu().numpy(), uo.case_map(case)
  assert got.shape == want.shape
  assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} entries differ"


def test_map_of_non_finite_coordinates(built_libs):
  cam = sta.LensCamera(64, 48, 60.0, 61.0, 31.3, 23.6, k1=1e300, k2=1e300, k3=1e300)
  target = (1e-3, 1e-3, 5.0, 5.0)
  with np.errstate(over="ignore", invalid="ignore"):
    want = uo.undistort_map(cam.source_array(), target, 48, 64, 11, 11)
  assert np.array_equal(sta.undistort_map(cam, target, (11, 11), device="cuda").cpu().numpy(), want)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("case", uo.REMAP_IDS)
def test_remap_equals_oracle(built_libs, case, C, B):
  _, m = uo.remap_cases()[case]
  src, want = uo.remap_reference(case, C, B)
  got = sta.remap(torch.from_numpy(np.array(src)).cuda(), torch.from_numpy(m).cuda()).cpu().numpy()
  assert got.shape == want.shape
  assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"


def test_more_images_than_one_sweep(built_libs):
  """19 images: a second slice of the batch, with the map's entries read again."""
  _, m = uo.remap_cases()["half-pixel"]
  src = uo.make_input(19, 48, 64, 3)
  got = sta.remap(torch.from_numpy(src).cuda(), torch.from_numpy(m).cuda()).cpu().numpy()
  assert np.array_equal(got, uo.remap(src, m))


@pytest.mark.parametrize("offset", [1, 2, 3, 5])
def test_unaligned_pointers(built_libs, offset):
  """Source and destination that start `offset` bytes into an allocation: no alignment is asked of either."""
  (Hs, Ws), m = uo.remap_cases()["barrel-517x1031"]
  C, B = 3, 2
  src, want = uo.remap_reference("barrel-517x1031", C, 3)
  src, want = src[:B], want[:B]
  Hd, Wd = m.shape[:2]
  n_src, n_dst = src.size, want.size
  src_buf = torch.zeros(n_src + 16, dtype=torch.uint8, device="cuda")
  dst_buf = torch.full((n_dst + 16,), 0xA5, dtype=torch.uint8, device="cuda")
  src_buf[offset:offset + n_src] = torch.from_numpy(np.array(src).reshape(-1)).cuda()
  map_dev = torch.from_numpy(m).cuda()
  code = _lib.load().gsr_image_remap_u8(src_buf.data_ptr() + offset, B, Hs, Ws, C, map_dev.data_ptr(),
                                        dst_buf.data_ptr() + offset, Hd, Wd, _lib.current_stream_ptr())
  assert code == 0
  out = dst_buf.cpu().numpy()
  assert np.array_equal(out[offset:offset + n_dst].reshape(B, Hd, Wd, C), want)
  assert (out[:offset] == 0xA5).all() and (out[offset + n_dst:] == 0xA5).all()        # nothing outside dst is written


def test_two_runs_are_bit_identical(built_libs):
  m = torch.from_numpy(uo.remap_cases()["random-96x120"][1]).cuda()
  src = torch.from_numpy(uo.make_input(3, 96, 120, 3)).cuda()
  assert torch.equal(sta.remap(src, m), sta.remap(src, m))
  cam = lens("barrel")
  a, b = (sta.undistort_map(cam, (55.0, 58.0, 31.0, 23.5), device="cuda") for _ in range(2))
  assert torch.equal(a, b)


def test_no_images_touch_nothing(built_libs):
  dst = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
  src = torch.zeros(64, dtype=torch.uint8, device="cuda")
  m = torch.zeros((2, 2, 2), dtype=torch.int32, device="cuda")
  lib, stream = _lib.load(), _lib.current_stream_ptr()
  assert lib.gsr_image_remap_u8(src.data_ptr(), 0, 4, 4, 3, m.data_ptr(), dst.data_ptr(), 2, 2, stream) == 0
  assert lib.gsr_image_remap_u8(src.data_ptr(), 2, 4, 4, 3, m.data_ptr(), dst.data_ptr(), 0, 2, stream) == 0
  torch.cuda.synchronize()
  assert (dst == 0xA5).all()
  assert tuple(sta.remap(torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device="cuda"), m).shape) == (0, 2, 2, 3)
  out = sta.remap(torch.zeros((2, 0, 4, 3), dtype=torch.uint8, device="cuda"), m)      # an empty source: all outside
  assert tuple(out.shape) == (2, 2, 2, 3) and not out.any()


def test_undistortion_on_a_device_tensor_equals_the_host(built_libs):
  und = sta.Undistortion(lens("barrel"))
  images = torch.from_numpy(uo.make_input(3, 48, 64, 3))
  host = und(images)
  assert torch.equal(und.map_on("cuda").cpu(), und.map)
  device = und(images.cuda())
  assert device.is_cuda and torch.equal(device.cpu(), host)
  assert torch.equal(und(images[0].cuda()).cpu(), host[0])


@pytest.mark.parametrize("scale", [dict(), dict(image_scale=0.5)], ids=["full", "image_scale"])
def test_colmap_dataset_device_path_gives_the_host_path_bytes(tmp_path, built_libs, scale):
  write_distorted(tmp_path)
  host = sta.COLMAPDataset(tmp_path, device="cpu", undistort=True, **scale)
  resident = sta.COLMAPDataset(tmp_path, resident=True, undistort=True, **scale)
  assert resident.device.type == "cuda" and torch.equal(resident.projections.intrinsics, host.projections.intrinsics)
  for h, r in zip(host.load_images(), resident.load_images()):
    assert r.image.is_cuda and r.image.dtype is torch.uint8 and torch.equal(r.image.cpu(), h.image)
