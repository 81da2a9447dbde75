"""Static budget of the neighbour-search kernels (csrc/neighbours.hip) on gfx950 -- hipcc cross-compiles without a GPU:
every kernel (each k of the kNN templates) is there with no scratch and at most 128 VGPRs, and the code holds no float
atomic (the centroid sums are fixed-order reductions)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"knn_kernel": 16, "knn_merge_kernel": 16, "km_assign_kernel": 1, "km_chunk_sum_kernel": 1,
           "km_finish_kernel": 1}
FLOAT_ATOMIC = re.compile(r"^\s*(\S*atomic_add_f\S*|\S*atomic_pk_add\S*|ds_add_f32|ds_add_rtn_f32|ds_pk_add_\S*)\b",
                          re.M)


@pytest.fixture(scope="module")
def isa():
  spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  asm = mod.compile_isa("neighbours.hip")
  return asm, mod.kernels(asm)


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
