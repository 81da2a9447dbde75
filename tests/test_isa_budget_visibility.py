"""Static budget of the visibility kernels (csrc/visibility.hip) on gfx950 -- hipcc cross-compiles without a GPU: every
kernel is there with no scratch and at most 128 VGPRs, and the code holds no float atomic (the counts are integers, the
feature sums fixed-order reductions)."""
import re

import pytest

from isa import FLOAT_ATOMIC, compiled, ops as ops_of

KERNELS = ("frustum_counts_kernel", "vf_scatter_kernel", "vf_chunk_sum_kernel", "vf_finish_kernel")


@pytest.fixture(scope="module")
def isa():
  return compiled("visibility.hip")


def test_every_visibility_kernel_is_there_inside_its_budget(isa):
  _, meta = isa
  for needle in KERNELS:
    names = [n for n in meta if re.search(rf"\d{needle}E", n)]
    assert len(names) == 1, (needle, names)
    k = meta[names[0]]
    assert k["scratch"] == 0 and k["vgpr"] <= 128, (names[0], k["vgpr"], k["scratch"])
  assert len(meta) == len(KERNELS), sorted(meta)


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)


def test_camera_records_come_through_the_scalar_cache(isa):
  _, meta = isa
  body = meta[next(n for n in meta if "frustum_counts_kernel" in n)]["body"]
  ops = ops_of(body)
  assert sum(op.startswith("s_load_dwordx") for op in ops) >= 4
  assert sum(op.startswith("global_load") for op in ops) <= 12       # the lane's own points, nothing per camera
