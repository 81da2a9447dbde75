"""Static budget of the 3-D smoothing filter's kernels (csrc/filter3d.hip) on gfx950 -- hipcc cross-compiles without a
GPU: the three kernels are there, with no scratch, no LDS and no more registers than the build they were measured in
(profiles/r17_filter3d.txt), the code holds no float atomic, and the rate kernel's cameras come through the scalar
cache."""
import re

import pytest

from isa import FLOAT_ATOMIC, compiled, ops as ops_of

VGPRS = {"sampling_rate_kernel": 107, "filter3d_forward_kernel": 59, "filter3d_backward_kernel": 77}     # as built


@pytest.fixture(scope="module")
def isa():
  return compiled("filter3d.hip")


def test_every_filter_kernel_is_there_inside_its_budget(isa):
  _, meta = isa
  for needle, vgprs in VGPRS.items():
    names = [n for n in meta if re.search(rf"\d{needle}E", n)]
    assert len(names) == 1, (needle, names)
    k = meta[names[0]]
    print(f"{needle}: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, scratch {k['scratch']} B, LDS {k['lds']} B")
    assert k["scratch"] == 0 and not k["lds"] and k["vgpr"] <= vgprs, (names[0], k["vgpr"], k["scratch"], k["lds"])
  assert len(meta) == len(VGPRS), sorted(meta)


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)


def test_cameras_come_through_the_scalar_cache(isa):
  _, meta = isa
  body = meta[next(n for n in meta if "sampling_rate_kernel" in n)]["body"]
  ops = ops_of(body)
  assert sum(op.startswith("s_load_dwordx") for op in ops) >= 4
  assert sum(op.startswith("global_load") for op in ops) <= 12       # the lane's own points, nothing per camera


def test_filter_rows_travel_as_float4(isa):
  _, meta = isa
  for needle, loads, stores in (("filter3d_forward_kernel", 5, 4), ("filter3d_backward_kernel", 9, 4)):
    body = meta[next(n for n in meta if needle in n)]["body"]
    ops = ops_of(body)
    assert sum(op == "global_load_dwordx4" for op in ops) >= loads, needle
    assert sum(op == "global_store_dwordx4" for op in ops) >= stores, needle
