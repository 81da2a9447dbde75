"""Static budget of the neighbour-search kernels (csrc/neighbours.hip) on gfx950 -- hipcc cross-compiles without a GPU:
every kernel (each k of the kNN templates) is there with no scratch and at most 128 VGPRs, and the code holds no float
atomic (the centroid sums are fixed-order reductions)."""
import re

import pytest

from isa import FLOAT_ATOMIC, compiled

KERNELS = {"knn_kernel": 16, "knn_merge_kernel": 16, "km_assign_kernel": 1, "km_chunk_sum_kernel": 1,
           "km_finish_kernel": 1}


@pytest.fixture(scope="module")
def isa():
  return compiled("neighbours.hip")


def test_every_neighbours_kernel_is_there_inside_its_budget(isa):
  _, meta = isa
  for needle, count in KERNELS.items():
    names = [n for n in meta if re.search(rf"\d{needle}E", n) or re.search(rf"\d{needle}ILi\d+E", n)]
    assert len(names) == count, (needle, names)
    for n in names:
      k = meta[n]
      assert k["scratch"] == 0 and k["vgpr"] <= 128, (n, k["vgpr"], k["scratch"])


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)
