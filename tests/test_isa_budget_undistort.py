"""Static budget of the undistortion kernels (csrc/undistort.hip) on gfx950 -- hipcc cross-compiles without a GPU: the
map kernel and the remap's two instantiations (1 and 3 channels) are there and nothing else, with no scratch, no float
atomic and no more registers or LDS than the build that was measured (profiles/r27_undistort.txt)."""
import re

import pytest

from isa import FLOAT_ATOMIC, compiled

# needle -> (VGPRs, LDS bytes) as built
BUDGET = {"undistort_map_kernel": (18, 0), "image_remap_kernelILi1E": (122, 17280), "image_remap_kernelILi3E": (126, 17280)}


@pytest.fixture(scope="module")
def built():
  return compiled("undistort.hip")


def test_the_kernels_are_there_inside_their_budget(built):
  asm, isa = built
  for needle, (vgprs, lds) in BUDGET.items():
    names = [n for n in isa if re.search(rf"\d{needle}", n)]
    assert len(names) == 1, (needle, names)
    k = isa[names[0]]
    used = int(re.search(rf"\.amdhsa_kernel {re.escape(names[0])}\n.*?\.amdhsa_group_segment_fixed_size (\d+)", asm, re.S).group(1))
    print(f"{needle}: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, scratch {k['scratch']} B, LDS {used} B")
    assert k["scratch"] == 0 and used <= lds and k["vgpr"] <= vgprs, (names[0], k["vgpr"], k["scratch"], used)
  assert len(isa) == len(BUDGET), sorted(isa)


def test_no_float_atomics(built):
  assert not FLOAT_ATOMIC.search(built[0])
