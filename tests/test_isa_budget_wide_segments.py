"""Static budget of the segmented wide-frame kernels (composite_wide.inc: wide_ckpt_fwd, wide_seg_fwd, wide_seg_combine)
on gfx950 -- hipcc cross-compiles without a GPU: no scratch, no barrier, no matrix instructions, and the VGPR counts the
occupancy of DESIGN.md section 4 rests on."""
import re

import pytest

from isa import compiled

FWD_VGPR = {4: 64, 8: 80, 16: 112}      # the K6 wide ceilings: 8 / 6 / 4 waves per SIMD
COMBINE_VGPR = 64                        # 8 waves per SIMD at every width (four channels at a time)
NEW = ("wide_ckpt_fwd", "wide_seg_fwd", "wide_seg_combine")


@pytest.fixture(scope="module")
def seg_kernels():
  meta = compiled("composite.hip")[1]
  return {n: k for n, k in meta.items() if any(s in n for s in NEW)}


def _width(name):
  return int(re.search(r"wide_\w+?ILi(\d+)E", name).group(1))


def test_every_instantiation_is_there(seg_kernels):
  for stem, count in (("wide_ckpt_fwd", 12), ("wide_seg_fwd", 12), ("wide_seg_combine", 6)):
    names = [n for n in seg_kernels if stem in n]
    assert len(names) == count and sorted({_width(n) for n in names}) == [4, 8, 16], (stem, names)
  # the kernel counts of tests/test_isa_budget_wide.py are by substring: no new kernel may match them
  assert not any("composite_fwd_wide" in n or "composite_bwd_wide" in n for n in seg_kernels)


def test_segment_kernels_stay_inside_their_budget(seg_kernels):
  for name, k in seg_kernels.items():
    body = k["body"]
    assert k["scratch"] == 0, (name, k["scratch"])
    assert not any(ln.strip().startswith("s_barrier") for ln in body), name
    assert not any("mfma" in ln for ln in body), name
    assert k["sgpr"] <= 102, (name, k["sgpr"])
    limit = COMBINE_VGPR if "wide_seg_combine" in name else FWD_VGPR[_width(name)]
    assert k["vgpr"] <= limit, (name, k["vgpr"], limit)
