"""Static budget of the visibility kernels (csrc/visibility.hip) on gfx950 -- hipcc cross-compiles without a GPU: every
kernel is there with no scratch and at most 128 VGPRs, and the code holds no float atomic (the counts are integers, the
feature sums fixed-order reductions)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("frustum_counts_kernel", "vf_scatter_kernel", "vf_chunk_sum_kernel", "vf_finish_kernel")
FLOAT_ATOMIC = re.compile(r"^\s*(\S*atomic_add_f\S*|\S*atomic_pk_add\S*|ds_add_f32|ds_add_rtn_f32|ds_pk_add_\S*)\b",
                          re.M)


@pytest.fixture(scope="module")
def isa():
  spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  asm = mod.compile_isa("visibility.hip")
  return asm, mod.kernels(asm)


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
  ops = [ln.split()[0] for ln in body if ln.strip() and not ln.strip().startswith((";", "."))]
  assert sum(op.startswith("s_load_dwordx") for op in ops) >= 4
  assert sum(op.startswith("global_load") for op in ops) <= 12       # the lane's own points, nothing per camera
