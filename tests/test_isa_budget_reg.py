"""Static budget of the regulariser and post-step kernels (csrc/reg.hip) on gfx950 -- hipcc cross-compiles without a
GPU: every kernel is there once with no scratch and at most 128 VGPRs, and the code holds no float atomic (the sums are
fixed-order reductions, the log_scaling gradient a plain read-modify-write on unique rows)."""
import pytest

from isa import FLOAT_ATOMIC, compiled

KERNELS = ("reg_fwd_kernel", "reg_finish_kernel", "reg_bwd_kernel", "scene_post_step_kernel")
# registers the compiler gives today (29 / 24 / 32 / 32): far inside the budget, pinned with a little slack so that a
# change that doubles them is noticed
VGPR_SEEN_MAX = 48


@pytest.fixture(scope="module")
def isa():
  return compiled("reg.hip")


def test_every_reg_kernel_is_there_inside_its_budget(isa):
  _, meta = isa
  for needle in KERNELS:
    names = [n for n in meta if needle in n]
    assert len(names) == 1, (needle, names)
    k = meta[names[0]]
    assert k["scratch"] == 0 and k["vgpr"] <= 128, (needle, k["vgpr"], k["scratch"])
    assert k["vgpr"] <= VGPR_SEEN_MAX, (needle, k["vgpr"])


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)
  assert "atomic" not in asm.lower()
