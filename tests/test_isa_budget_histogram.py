"""Static budget of the histogram kernels (csrc/histogram.hip) on gfx950 -- hipcc cross-compiles without a GPU: the five
kernels are there (the range and the binning sweep once per load width, the finalize pass), with no scratch, no float
atomic and no more registers or LDS than the build they were measured in (profiles/r22_trainer.txt)."""
import re

import pytest

from isa import FLOAT_ATOMIC, compiled

# needle -> (VGPRs, LDS bytes) as built
BUDGET = {"hist_range_kernelILi1E": (20, 32), "hist_range_kernelILi4E": (22, 32), "hist_bin_kernelILi1E": (40, 4208),
          "hist_bin_kernelILi4E": (46, 4208), "hist_finalize_kernelE": (41, 4096)}


@pytest.fixture(scope="module")
def built():
  return compiled("histogram.hip")


def test_the_kernels_are_there_inside_their_budget(built):
  asm, isa = built
  for needle, (vgprs, lds) in BUDGET.items():
    names = [n for n in isa if re.search(rf"\d{needle}", n)]
    assert len(names) == 1, (needle, names)
    k = isa[names[0]]
    # (the kernel descriptor's own directive: the metadata lists the LDS size ahead of the name, where kernels() does not look)
    used = int(re.search(rf"\.amdhsa_kernel {re.escape(names[0])}\n.*?\.amdhsa_group_segment_fixed_size (\d+)", asm, re.S).group(1))
    print(f"{needle}: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, scratch {k['scratch']} B, LDS {used} B")
    assert k["scratch"] == 0 and used <= lds and k["vgpr"] <= vgprs, (names[0], k["vgpr"], k["scratch"], used)
  assert len(isa) == len(BUDGET), sorted(isa)


def test_no_float_atomics(built):
  assert not FLOAT_ATOMIC.search(built[0])
