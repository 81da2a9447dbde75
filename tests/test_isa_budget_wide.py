"""Static budget of the wide-feature kernels (K6 / K7 for 4..16 channels, composite_wide.inc compiled into
composite.hip) on gfx950 -- hipcc cross-compiles without a GPU: no scratch, no barrier, no matrix instructions, and the
VGPR counts the occupancy of DESIGN.md section 4 rests on."""
import re

import pytest

from isa import compiled

# VGPR ceilings per feature-table width: K6 wide (every VIS / MEDIAN form) and K7 wide
K6_VGPR = {4: 64, 8: 80, 16: 112}      # 8 / 6 / 4 waves per SIMD
K7_VGPR = {4: 102, 8: 168, 16: 256}    # 5 / 3 / 2 waves per SIMD


@pytest.fixture(scope="module")
def wide_kernels():
  meta = compiled("composite.hip")[1]
  return {n: k for n, k in meta.items() if "composite_fwd_wide" in n or "composite_bwd_wide" in n}


def _width(name):
  return int(re.search(r"_wideILi(\d+)E", name).group(1))


def test_every_wide_instantiation_is_there(wide_kernels):
  fwd = [n for n in wide_kernels if "fwd_wide" in n]
  bwd = [n for n in wide_kernels if "bwd_wide" in n]
  assert sorted({_width(n) for n in fwd}) == [4, 8, 16] and len(fwd) == 12      # 3 widths x (VIS, MEDIAN)
  assert sorted(_width(n) for n in bwd) == [4, 8, 16]


def test_wide_kernels_stay_inside_their_budget(wide_kernels):
  for name, k in wide_kernels.items():
    cw = _width(name)
    body = k["body"]
    assert k["scratch"] == 0, (name, k["scratch"])
    assert not any(ln.strip().startswith("s_barrier") for ln in body), name
    assert not any("mfma" in ln for ln in body), name
    limit = (K6_VGPR if "fwd_wide" in name else K7_VGPR)[cw]
    assert k["vgpr"] <= limit, (name, k["vgpr"], limit)
    assert k["sgpr"] <= 102, (name, k["sgpr"])
