"""Static budget of the colour-model kernels (csrc/color_model.hip) on gfx950 -- hipcc cross-compiles without a GPU:
every instantiation (L in {1, 2} x F blocks in {1, 2} x SH degree 2..5) is there with no scratch and within its VGPR
budget (arch + accumulation registers: the backward keeps the workgroup's weight-gradient tiles and the recomputed
forward in registers at one wave per SIMD), the forward and backward run their Linears on f16 MFMA, and the code holds
no float atomic (the gradient slots are summed in a fixed order)."""
import re

import pytest

from isa import FLOAT_ATOMIC, compiled

KERNELS = {"cm_pack_kernel": (1, 64), "cm_forward_kernel": (16, 160), "cm_backward_kernel": (16, 512),
           "cm_finish_kernel": (16, 32)}


@pytest.fixture(scope="module")
def isa():
  return compiled("color_model.hip")


def _names(meta, needle):
  return [n for n in meta if re.search(rf"\d{needle}E", n) or re.search(rf"\d{needle}ILi\d+E", n)]


def test_every_color_kernel_is_there_inside_its_budget(isa):
  _, meta = isa
  for needle, (count, vgpr) in KERNELS.items():
    names = _names(meta, needle)
    assert len(names) == count, (needle, names)
    for n in names:
      k = meta[n]
      assert k["scratch"] == 0 and k["vgpr"] <= vgpr, (n, k["vgpr"], k["scratch"])


def _body(asm, name):
  start = asm.index(f"{name}:")
  return asm[start:asm.index("s_endpgm", start)]


def test_forward_and_backward_use_f16_mfma(isa):
  asm, meta = isa
  for needle in ("cm_forward_kernel", "cm_backward_kernel"):
    for n in _names(meta, needle):
      body = _body(asm, n)
      assert re.search(r"v_mfma_f32_16x16x32_f16", body), n
  for n in _names(meta, "cm_backward_kernel"):
    assert re.search(r"v_mfma_f32_16x16x16_?f16", _body(asm, n)), n


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)
