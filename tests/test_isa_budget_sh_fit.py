"""Static budget of the SH export fit's kernels (csrc/sh_fit.hip) on gfx950 -- hipcc cross-compiles without a GPU: the
two kernels exist for K = 1, 4, 9, 16 and nothing else, with no scratch and no more registers than the build they were
measured in (profiles/r18_sh_fit.txt), the code holds no float atomic, the accumulation is fused fp64 multiply-adds and
its rows travel as 8-byte words."""
import re

import pytest

from isa import FLOAT_ATOMIC, compiled, ops as ops_of

KS = (1, 4, 9, 16)
VGPRS = {("sh_fit_accumulate_kernel", 1): 13, ("sh_fit_accumulate_kernel", 4): 18, ("sh_fit_accumulate_kernel", 9): 33,
         ("sh_fit_accumulate_kernel", 16): 54, ("sh_fit_solve_kernel", 1): 30, ("sh_fit_solve_kernel", 4): 38,
         ("sh_fit_solve_kernel", 9): 40, ("sh_fit_solve_kernel", 16): 68}                                  # as built


@pytest.fixture(scope="module")
def isa():
  return compiled("sh_fit.hip")


def test_every_instantiation_is_there_inside_its_budget(isa):
  _, meta = isa
  for (needle, K), vgprs in VGPRS.items():
    names = [n for n in meta if re.search(rf"\d{needle}ILi{K}E", n)]
    assert len(names) == 1, (needle, K, names)
    k = meta[names[0]]
    print(f"{needle}<{K}>: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, scratch {k['scratch']} B")
    assert k["scratch"] == 0 and k["vgpr"] <= vgprs, (names[0], k["vgpr"], k["scratch"])
    assert not any(op.startswith("scratch_") for op in ops_of(k["body"])), names[0]
  assert len(meta) == len(VGPRS), sorted(meta)


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)


def test_accumulation_is_fused_fp64_on_8_byte_words(isa):
  """One fused multiply-add per component (v_fma_f64, or v_fmac_f64 -- the same operation with the accumulator as the
  destination, which is what the compiler picks for acc = fma(a, b, acc)) and no narrower access to the rows."""
  _, meta = isa
  for K in KS:
    k = meta[next(n for n in meta if f"sh_fit_accumulate_kernelILi{K}E" in n)]
    ops = ops_of(k["body"])
    components = K * (K + 1) // 2 + 3 * K + 1
    per_lane = -(-components // 16)
    fused = sum(op.startswith(("v_fma_f64", "v_fmac_f64")) for op in ops)
    wide_loads = sum(op.startswith(("global_load_dwordx2", "global_load_dwordx3", "global_load_dwordx4")) for op in ops)
    stores = [op for op in ops if op.startswith("global_store")]
    print(f"accumulate<{K}>: {fused} fused fp64 multiply-adds, {wide_loads} loads of 8 bytes or more, {len(stores)} stores")
    assert fused >= per_lane
    assert wide_loads >= per_lane
    assert len(stores) == per_lane and all(op == "global_store_dwordx2" for op in stores)
