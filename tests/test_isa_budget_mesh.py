"""Static budget of the TSDF meshing kernels (csrc/mesh.hip) on gfx950 -- hipcc cross-compiles without a GPU: the file
holds the mesh kernels and nothing else, none uses scratch, the code holds no atomic of any kind (every node, cell and
edge has one writer), fp64 fused multiply-adds appear only inside division expansions, and registers and LDS are no more
than recorded when the kernels were written -- a guard against a later change that spills or bloats them, not a tuned
target."""
import pytest

from isa import FLOAT_ATOMIC, compiled, ops

# kernel -> (VGPRs, LDS bytes) as built; the 16 bytes are the block hand-off of gsr_block_rank
BUDGET = {
    "tsdf_integrate_kernel": (28, 0),
    "mesh_vertex_mask_kernel": (34, 0),
    "mesh_vertex_emit_kernel": (82, 16),
    "mesh_face_mask_kernel": (22, 0),
    "mesh_face_emit_kernel": (23, 16),
}
# fp64 divisions: 1 / p_2 of the projection; per active cell eight m = sum_d / n, twelve t = m_A / (m_A - m_B), three acc / c
DIVISIONS = dict({k: 0 for k in BUDGET}, tsdf_integrate_kernel=1, mesh_vertex_emit_kernel=23)


@pytest.fixture(scope="module")
def isa():
  return compiled("mesh.hip")


def _kernel(meta, needle):
  return meta[[n for n in meta if needle in n][0]]


def test_the_file_holds_the_mesh_kernels_and_nothing_else(isa):
  _, meta = isa
  assert len(meta) == len(BUDGET)
  for needle in BUDGET:
    assert len([n for n in meta if needle in n]) == 1, needle


def test_every_kernel_is_inside_its_budget(isa):
  _, meta = isa
  for needle, (vgpr, lds) in BUDGET.items():
    k = _kernel(meta, needle)
    assert k["scratch"] == 0, (needle, k["scratch"])
    assert k["vgpr"] <= vgpr and k["lds"] <= lds, (needle, k["vgpr"], k["lds"])


def test_no_atomics_of_any_kind(isa):
  asm, meta = isa
  assert not FLOAT_ATOMIC.findall(asm)
  for name, k in meta.items():
    assert not [op for op in ops(k["body"]) if "atomic" in op], name


def test_the_arithmetic_is_not_contracted(isa):
  """fp64 fused multiply-adds appear only inside the division's expansion, three per division, and the divisions are the
  contract's."""
  _, meta = isa
  fused = {needle: sum(1 for op in ops(_kernel(meta, needle)["body"]) if op.startswith("v_fma_f64")) for needle in BUDGET}
  divisions = {needle: sum(1 for op in ops(_kernel(meta, needle)["body"]) if op.startswith("v_div_fmas_f64"))
               for needle in BUDGET}
  assert divisions == DIVISIONS
  assert fused == {k: 3 * v for k, v in divisions.items()}
  for needle in BUDGET:                                               # ... and no fp32 ones: the kernels hold no float arithmetic
    assert not [op for op in ops(_kernel(meta, needle)["body"]) if op.startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32"))], needle
