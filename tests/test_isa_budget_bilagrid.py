"""Static budget of the bilateral-grid kernels (csrc/bilagrid.hip) on gfx950 -- hipcc cross-compiles without a GPU: every
kernel is there with no scratch and at most 128 VGPRs, and the code holds no float atomic (the grid gradient and the
TV sum are fixed-order reductions)."""
import pytest

from isa import FLOAT_ATOMIC, compiled

KERNELS = ("bg_slice_fwd_kernel", "bg_slice_bwd_kernel", "bg_grad_finish_kernel", "bg_tv_kernel", "bg_tv_finish_kernel")


@pytest.fixture(scope="module")
def isa():
  return compiled("bilagrid.hip")


def test_every_bilagrid_kernel_is_there_inside_its_budget(isa):
  _, meta = isa
  for needle in KERNELS:
    names = [n for n in meta if needle in n]
    assert len(names) == 1, (needle, names)
    k = meta[names[0]]
    assert k["scratch"] == 0 and k["vgpr"] <= 128, (needle, k["vgpr"], k["scratch"])


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)
