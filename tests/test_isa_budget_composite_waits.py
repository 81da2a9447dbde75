"""Where the composite walks may wait for memory (static, from the gfx950 code hipcc cross-compiles):
the forward walk's four-pair loop holds no wait on the vector-memory counter -- the per-pair visibility is parked in LDS
and handed over once per 64 list positions, outside that loop -- and the backward kernel's entry state arrives with one
wait, next to the one of the launch-order lookup."""
import pytest

from isa import audit


@pytest.fixture(scope="module")
def waits():
  return audit()["composite_waits"]


@pytest.mark.parametrize("kernel,copies", [("K6_fwd_C3_vis", 2), ("K6_segC_C3_vis", 1)])
def test_four_pair_loop_holds_no_vector_memory_wait(waits, kernel, copies):
  loops = waits[kernel]["four_pair_loops"]
  print(kernel, loops)
  # the tile kernel holds two copies of the walk (whole list / checkpointed), pass C of a heavy tile one
  assert len(loops) == copies, loops
  for lp in loops:
    assert lp["blocks"] > 1, lp
    assert lp["vmcnt_waits"] == 0, lp


def test_backward_prologue_waits_at_most_twice(waits):
  n = waits["K7_bwd_C3"]["prologue_vmcnt_waits"]
  print("K7 prologue vmcnt waits", n)
  assert n <= 2, n
