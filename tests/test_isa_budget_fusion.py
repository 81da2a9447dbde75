"""Static budget of the depth-fusion kernels (csrc/fusion.hip) on gfx950 -- hipcc cross-compiles without a GPU: the file
holds the fusion kernels and nothing else, none uses scratch, the code holds no float atomic (the voxel sums are integer
shuffles, the counters have one writer each), and registers and LDS are no more than recorded when the kernels were
written -- a guard against a later change that spills or bloats them, not a tuned target."""
import pytest

from isa import FLOAT_ATOMIC, compiled, ops

# kernel -> (VGPRs, LDS bytes) as built
BUDGET = {
    "fuse_check_kernel": (28, 0),
    "fuse_mask_kernel": (6, 0),
    "fuse_emit_kernel": (26, 16),
    "voxel_low_keys_kernel": (7, 0),
    "voxel_high_keys_kernel": (8, 0),
    "voxel_heads_kernel": (19, 0),
    "voxel_starts_kernel": (8, 0),
    "voxel_reduce_kernel": (68, 0),
}


@pytest.fixture(scope="module")
def isa():
  return compiled("fusion.hip")


def test_the_file_holds_the_fusion_kernels_and_nothing_else(isa):
  _, meta = isa
  assert len(meta) == len(BUDGET)
  for needle in BUDGET:
    assert len([n for n in meta if needle in n]) == 1, needle


def test_every_kernel_is_inside_its_budget(isa):
  _, meta = isa
  for needle, (vgpr, lds) in BUDGET.items():
    k = meta[[n for n in meta if needle in n][0]]
    assert k["scratch"] == 0, (needle, k["scratch"])
    assert k["vgpr"] <= vgpr and k["lds"] <= lds, (needle, k["vgpr"], k["lds"])


def test_no_float_atomics_and_no_atomics_at_all(isa):
  asm, meta = isa
  assert not FLOAT_ATOMIC.findall(asm)
  for name, k in meta.items():
    assert not [op for op in ops(k["body"]) if "atomic" in op], name


def test_the_arithmetic_is_not_contracted(isa):
  """fp64 fused multiply-adds appear only inside the division's expansion: three per division, one division in the
  check kernel and one per axis and path in the reduction, none anywhere else."""
  _, meta = isa
  fused = {needle: sum(1 for op in ops(meta[[n for n in meta if needle in n][0]]["body"]) if op.startswith("v_fma_f64"))
           for needle in BUDGET}
  divisions = {needle: sum(1 for op in ops(meta[[n for n in meta if needle in n][0]]["body"]) if op.startswith("v_div_fmas_f64"))
               for needle in BUDGET}
  assert divisions == dict({k: 0 for k in BUDGET}, fuse_check_kernel=1, voxel_reduce_kernel=6)
  assert fused == {k: 3 * v for k, v in divisions.items()}
