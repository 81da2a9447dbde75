"""gsr_image_resize_area_u8 on the GPU against the numpy oracle (tests/image_oracle.py): equal bytes on every pixel, at
every shape of the list the host test runs, with 1 and 3 channels and with 1 and 3 images (with Hs Ws C odd the second
image starts misaligned); sums that pass 2^32; long rows staged in pieces; bit-identical repeats; B = 0."""
import numpy as np
import pytest
import torch

import image_oracle as io
import splat_trainer_amd as sta
from splat_trainer_amd import _lib

pytestmark = pytest.mark.gpu


def _resize(src: np.ndarray, Hd: int, Wd: int) -> np.ndarray:
  return sta.resize_area(torch.from_numpy(src).cuda(), (Hd, Wd)).cpu().numpy()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", io.SHAPES, ids=io.SHAPE_IDS)
def test_equals_oracle(built_libs, shape, C, B):
  (Hs, Ws), (Hd, Wd) = shape
  src = io.make_input(B, Hs, Ws, C)
  got, want = _resize(src, Hd, Wd), io.resize_area(src, Hd, Wd)
  assert got.shape == want.shape
  assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"


@pytest.mark.parametrize("offset", [1, 2, 3, 5])
def test_unaligned_pointers(built_libs, offset):
  """Source and destination that start `offset` bytes into an allocation: no alignment is asked of either."""
  (Hs, Ws), (Hd, Wd), C, B = (70, 119), (33, 50), 3, 2
  src = io.make_input(B, Hs, Ws, C)
  n_src, n_dst = src.size, B * Hd * Wd * C
  src_buf = torch.zeros(n_src + 16, dtype=torch.uint8, device="cuda")
  dst_buf = torch.full((n_dst + 16,), 0xA5, dtype=torch.uint8, device="cuda")
  src_buf[offset:offset + n_src] = torch.from_numpy(src.reshape(-1)).cuda()
  code = _lib.load().gsr_image_resize_area_u8(src_buf.data_ptr() + offset, B, Hs, Ws, C, dst_buf.data_ptr() + offset, Hd, Wd,
                                              _lib.current_stream_ptr())
  assert code == 0
  out = dst_buf.cpu().numpy()
  assert np.array_equal(out[offset:offset + n_dst].reshape(B, Hd, Wd, C), io.resize_area(src, Hd, Wd))
  assert (out[:offset] == 0xA5).all() and (out[offset + n_dst:] == 0xA5).all()        # nothing outside dst is written


def test_sums_above_32_bits(built_libs):
  """255 Ws Hs passes 2^32 here: every output that does not touch the random corner must be exactly 255, and the
  corner pixel equals the oracle of its own source block (its weights reach no further)."""
  Hs, Ws, Hd, Wd, C = 4100, 4200, 8, 8, 3
  assert 255 * Hs * Ws > 2 ** 32
  src = torch.full((1, Hs, Ws, C), 255, dtype=torch.uint8)
  corner = np.random.default_rng(3).integers(0, 256, size=(64, 64, C), dtype=np.uint8)
  src[0, :64, :64] = torch.from_numpy(corner)
  got = _resize(src.numpy(), Hd, Wd)
  rest = got.copy()
  rest[0, 0, 0] = 255
  assert (rest == 255).all()
  # the corner pixel covers source rows 0 .. ceil(4100 / 8) - 1 and columns 0 .. 524, all 255 outside the 64 x 64 block
  wy, wx = io.weights(Hs, Hd)[0], io.weights(Ws, Wd)[0]
  block = src[0].numpy().astype(np.int64)[:wy.nonzero()[0].max() + 1, :wx.nonzero()[0].max() + 1]
  S = np.einsum("y,x,yxc->c", wy[:block.shape[0]], wx[:block.shape[1]], block)
  D = Ws * Hs
  assert got[0, 0, 0].tolist() == ((2 * S + D) // (2 * D)).tolist()
  assert (got[0, 0, 0] < 255).all()


@pytest.mark.parametrize("C", [1, 3])
def test_rows_longer_than_the_staging_buffer(built_libs, C):
  """A ratio of 10000: a row of a block's source (30 and 90 KB) is staged in pieces of 16 KiB."""
  src = io.make_input(2, 3, 30000, C)
  assert np.array_equal(_resize(src, 2, 3), io.resize_area(src, 2, 3))


def test_two_runs_are_bit_identical(built_libs):
  src = torch.from_numpy(io.make_input(3, 96, 120, 3)).cuda()
  assert torch.equal(sta.resize_area(src, (61, 77)), sta.resize_area(src, (61, 77)))


def test_no_images_touch_nothing(built_libs):
  dst = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
  src = torch.zeros(64, dtype=torch.uint8, device="cuda")
  lib = _lib.load()
  assert lib.gsr_image_resize_area_u8(src.data_ptr(), 0, 4, 4, 3, dst.data_ptr(), 2, 2, _lib.current_stream_ptr()) == 0
  assert lib.gsr_image_resize_area_u8(src.data_ptr(), 2, 0, 4, 3, dst.data_ptr(), 0, 0, _lib.current_stream_ptr()) == 0
  torch.cuda.synchronize()
  assert (dst == 0xA5).all()
  assert tuple(sta.resize_area(torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device="cuda"), (2, 2)).shape) == (0, 2, 2, 3)
