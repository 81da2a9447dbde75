"""The area resize on the host (csrc/gsr_image.h through the shim: the source the kernel compiles) against the numpy
oracle (tests/image_oracle.py), byte for byte at every shape of the GPU test; the oracle itself against PIL's box
reduction at the ratios where PIL is exact; and the multiply-shift that stands in for the division against ``//``."""
import numpy as np
import pytest
import torch
from PIL import Image

import hostmath
import image_oracle as io
import splat_trainer_amd as sta


@pytest.fixture(scope="module")
def hm(built_libs):
  return hostmath.load(built_libs)


def _shim_resize(hm, src, Hd, Wd):
  B, Hs, Ws, C = src.shape
  dst = np.full((B, Hd, Wd, C), 0xA5, np.uint8)
  assert hm.hm_image_resize_area_u8(src, B, Hs, Ws, C, dst, Hd, Wd) == 0
  return dst


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", io.SHAPES, ids=io.SHAPE_IDS)
def test_shim_equals_oracle(hm, shape, C, B):
  (Hs, Ws), (Hd, Wd) = shape
  src = io.make_input(B, Hs, Ws, C)
  assert np.array_equal(_shim_resize(hm, src, Hd, Wd), io.resize_area(src, Hd, Wd))


def test_equal_sizes_copy(hm):
  src = io.make_input(2, 48, 64, 3)
  assert np.array_equal(_shim_resize(hm, src, 48, 64), src)
  assert np.array_equal(io.resize_area(src, 48, 64), src)


@pytest.mark.parametrize("ratio", [2, 4])
def test_oracle_equals_pil_box_reduction(ratio):
  """An anchor outside this project: at ratios 2 and 4 PIL's ``reduce`` is the exact mean rounded half up."""
  src = np.random.default_rng(5).integers(0, 256, size=(96, 120, 3), dtype=np.uint8)
  want = np.asarray(Image.fromarray(src).reduce(ratio))
  got = io.resize_area(src[None], 96 // ratio, 120 // ratio)[0]
  assert np.array_equal(got, want)


def test_package_cpu_path_is_the_shim(built_libs):
  src = io.make_input(3, 70, 119, 3)
  got = sta.resize_area(torch.from_numpy(src), (33, 50))
  assert got.dtype is torch.uint8 and tuple(got.shape) == (3, 33, 50, 3)
  assert np.array_equal(got.numpy(), io.resize_area(src, 33, 50))
  one = sta.resize_area(torch.from_numpy(src[1]), (33, 50))
  assert np.array_equal(one.numpy(), got[1].numpy())
  for size in [(71, 50), (33, 120), (0, 50)]:
    with pytest.raises(ValueError, match="only downscaling"):
      sta.resize_area(torch.from_numpy(src), size)
  with pytest.raises(ValueError, match="1 or 3 channels"):
    sta.resize_area(torch.zeros((1, 4, 4, 2), dtype=torch.uint8), (2, 2))
  with pytest.raises(ValueError, match="uint8"):
    sta.resize_area(torch.zeros((1, 4, 4, 3)), (2, 2))


# ------------------------------------------------------------------------------------------- the multiply-shift
DIVISORS = sorted({(ws, hs) for (hs, ws), _ in io.SHAPES} | {(4200, 4100), (1, 1), (32768, 32768), (32768, 32767),
                                                              (4032, 3024), (3, 1)})


@pytest.mark.parametrize("Ws,Hs", DIVISORS)
def test_round_div_equals_floor_division(hm, Ws, Hs):
  """floor((2 S + D) / (2 D)) at the ends of S's range, either side of the first tie, and at random S."""
  D = Ws * Hs
  rng = np.random.default_rng(D)
  edge = [0, 1, D // 2 - 1, D // 2, D // 2 + 1, 255 * D - 1, 255 * D]
  ties = [(2 * k + 1) * D // 2 + o for k in (0, 1, 127, 253, 254) for o in (-1, 0, 1)]      # either side of q + 1/2
  multiples = [k * D + o for k in (1, 2, 128, 254) for o in (-1, 0, 1)]
  S = np.array([s for s in edge + ties + multiples if 0 <= s <= 255 * D] +
               rng.integers(0, 255 * D + 1, size=20000).tolist(), dtype=np.uint64)
  out = np.zeros(S.size, np.uint32)
  hm.hm_image_round_div(S, S.size, Ws, Hs, out)
  want = [(2 * int(s) + D) // (2 * D) for s in S]                          # Python integers: no width to overflow
  assert out.tolist() == want
