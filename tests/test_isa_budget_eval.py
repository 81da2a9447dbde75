"""Static budget of the evaluation kernels (csrc/eval.hip) on gfx950 -- hipcc cross-compiles without a GPU: every kernel
is there once with no scratch (the pass kernel carries 45 fp64 accumulators per thread, one channel per blockIdx.y, so
that they stay in registers; the solve works in LDS), and the code holds no float atomic: the sums are fixed-order
reductions."""
import re

import pytest

from isa import compiled

# registers the compiler gives today, pinned with a little slack so that a change that spills or doubles them is noticed
KERNELS = {"color_fit_pass_kernel": (184, 208), "color_fit_finish_kernel": (104, 128)}
FLOAT_ATOMIC = re.compile(r"^\s*(\S*atomic_add_f\S*|\S*atomic_pk_add\S*|ds_add_f32|ds_add_rtn_f32|ds_pk_add_\S*|"
                          r"ds_add_f64|ds_add_rtn_f64)\b", re.M)


@pytest.fixture(scope="module")
def isa():
  return compiled("eval.hip")


def test_every_eval_kernel_is_there_inside_its_budget(isa):
  _, meta = isa
  assert len(meta) == len(KERNELS), sorted(meta)
  for needle, (seen, budget) in KERNELS.items():
    names = [n for n in meta if needle in n]
    assert len(names) == 1, (needle, names)
    k = meta[names[0]]
    assert k["scratch"] == 0, (needle, k["scratch"])
    # 256 threads per block: one wave per SIMD, so up to 512 registers would still launch; the pin is what matters
    assert k["vgpr"] <= budget, (needle, k["vgpr"], seen)


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)
  assert "atomic" not in asm.lower()
