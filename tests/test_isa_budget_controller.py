"""Static budget of the MCMC noise kernels (csrc/controller.hip) on gfx950 -- hipcc cross-compiles without a GPU: the two
kernels are there, with no scratch, no LDS and no more registers than the build they were measured in
(profiles/r20_controllers.txt)."""
import re

import pytest

from isa import compiled

VGPRS = {"mcmc_noise_kernel": 70, "mcmc_draws_kernel": 42}     # as built


@pytest.fixture(scope="module")
def isa():
  return compiled("controller.hip")[1]


def test_both_kernels_are_there_inside_their_budget(isa):
  for needle, vgprs in VGPRS.items():
    names = [n for n in isa if re.search(rf"\d{needle}E", n)]
    assert len(names) == 1, (needle, names)
    k = isa[names[0]]
    print(f"{needle}: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, scratch {k['scratch']} B, LDS {k['lds']} B")
    assert k["scratch"] == 0 and not k["lds"] and k["vgpr"] <= vgprs, (names[0], k["vgpr"], k["scratch"], k["lds"])
  assert len(isa) == len(VGPRS), sorted(isa)
