"""Static budget of the normal-consistency kernels (csrc/normals.hip) on gfx950 -- hipcc cross-compiles without a GPU: the
file holds these kernels and nothing else, none uses scratch, the code holds no float atomic (every element has one
writer, the loss is a fixed-order sum), and registers and LDS are no more than recorded when the kernels were written --
a guard against a later change that spills or bloats them, not a tuned target."""
import pytest

from isa import FLOAT_ATOMIC, compiled

# kernel -> (VGPRs, LDS bytes) as built.  LDS: 34 x 10 depths (+ the 16 bytes of the block hand-off with the loss);
# 36 x 12 depths + 9 x 340 stencil terms in the backward
BUDGET = {
    "splat_normals_forward_kernel": (20, 0),
    "splat_normals_backward_kernel": (30, 0),
    "pixel_normals_kernelILb0E": (24, 1360),
    "pixel_normals_kernelILb1E": (24, 1376),
    "normal_loss_finish_kernel": (8, 16),
    "normal_loss_backward_kernel": (41, 13968),
}


@pytest.fixture(scope="module")
def isa():
  return compiled("normals.hip")


def _kernel(meta, needle):
  return meta[[n for n in meta if needle in n][0]]


def test_the_file_holds_the_normal_kernels_and_nothing_else(isa):
  _, meta = isa
  assert len(meta) == len(BUDGET)
  for needle in BUDGET:
    assert len([n for n in meta if needle in n]) == 1, needle


def test_every_kernel_is_inside_its_budget(isa):
  _, meta = isa
  for needle, (vgpr, lds) in BUDGET.items():
    k = _kernel(meta, needle)
    assert k["scratch"] == 0, (needle, k["scratch"])
    assert k["vgpr"] <= vgpr and k["lds"] <= lds, (needle, k["vgpr"], k["lds"])


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)
