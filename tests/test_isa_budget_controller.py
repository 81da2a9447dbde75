"""Static budget of the MCMC noise kernels (csrc/controller.hip) on gfx950 -- hipcc cross-compiles without a GPU: the two
kernels are there, with no scratch, no LDS and no more registers than the build they were measured in
(profiles/r20_controllers.txt)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGPRS = {"mcmc_noise_kernel": 70, "mcmc_draws_kernel": 42}     # as built


@pytest.fixture(scope="module")
def isa():
  spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod.kernels(mod.compile_isa("controller.hip"))


def test_both_kernels_are_there_inside_their_budget(isa):
  for needle, vgprs in VGPRS.items():
    names = [n for n in isa if re.search(rf"\d{needle}E", n)]
    assert len(names) == 1, (needle, names)
    k = isa[names[0]]
    print(f"{needle}: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, scratch {k['scratch']} B, LDS {k['lds']} B")
    assert k["scratch"] == 0 and not k["lds"] and k["vgpr"] <= vgprs, (names[0], k["vgpr"], k["scratch"], k["lds"])
  assert len(isa) == len(VGPRS), sorted(isa)
