"""Where the per-splat and sort kernels of a frame wait for memory (static, from the gfx950 code hipcc cross-compiles;
DESIGN.md section 4, profiles/r23_frame_waits.txt).  Their loads go out when their address is known -- next to the
device count, at positions clamped to the capacity -- so the way from the kernel's entry to its first global store holds
one memory round trip per truly dependent step.  A round trip = a wait on the vector-memory (scalar-memory) counter with
at least one vector (scalar) load outstanding since the last one counted, in layout order (tools/isa_stats.py:
waits_to_first_store).  The counts reached, (vector, scalar), with the parent's in brackets -- asserted as ceilings
(`<=`): the count follows the compiler's block layout, and a layout that puts a cold path behind the store lowers it:

  rs_scatter, all four instantiations a frame runs   1, 4   [6 and 18 (16 rounds), 5]
                   the block's elements, the digit totals and its column of the offset table, all at entry
  rs_hist<9>       2, 4   [9, 4]   1 at entry + the prefetch of the next four rounds inside the loop
  rs_hist<8>       1, 4   [9, 4]
  cull_count       6, 4   [4, 3]   2 on the path of a wave whose span lies inside N (two batches of eight positions)
                   + 4 on the point-by-point path of the one wave that crosses N, which the layout puts in front of the
                   store as well; the fourth scalar trip is the second half of the camera
  cull_write       2, 3   [3, 3]   the first batch with the wave's own count; the second batch
  project_sh_fwd   K = 16 and 4: 2, 9 / 2, 10   [14, 9 / 5, 9]  the index; then the thread's parameters and all its
                   coefficient pieces.  K = 9: 4, 9 (4, 10 without Jacobian)  [29, 9 / 29, 8]  its 27 scalar pieces go in three
                   batches of nine: all 27 at once cost 134 VGPRs, three waves per SIMD where the LDS allows five.  K = 1: 2, 9
  tile_count       2, 6   [2, 6]   the rank's splat id and the row it names: a true dependence, as in the parent; what
                   changed is the ORDER -- the splat id is requested in front of the scalar load of the device count
                   (asserted below), not behind its wait
  reduce_grad      6, 5   [8, 6]   over the whole kernel, the wave pass over large ranks included: the three pieces a
                   thread fetches of a chunk are one trip, and the row id it scatters to arrives with its first words

Registers: every kernel of the table keeps the waves per SIMD it had (64 VGPRs = 8 waves; the scatter of 16 rounds is
held to two blocks per CU by its 54 KB of LDS, the degree-3 projection to three by its 50 KB -- 168 VGPRs; degrees 0-2
to five by their 27-28 KB -- 96 VGPRs, and they stay at their parents' 52 / 52 / 93 and 58).  No scratch anywhere."""
import pytest

from isa import compiled, stats

# label -> ceilings: (vector-memory round trips to the first store, scalar-memory round trips, VGPRs)
BUDGET = {
    "rs_scatter_1v_4_9": (1, 4, 64), "rs_scatter_1v_4_8": (1, 4, 64), "rs_scatter_2v_4_8": (1, 4, 64),
    "rs_scatter_2v_16_8": (1, 4, 128),
    "rs_hist_9": (2, 4, 64), "rs_hist_8": (1, 4, 64),
    "cull_count": (6, 4, 64), "cull_write": (2, 3, 64),
    "project_sh_fwd_K16": (2, 9, 168), "project_sh_fwd_K9": (4, 9, 96), "project_sh_fwd_K9_nojac": (4, 10, 96),
    "project_sh_fwd_K4": (2, 10, 64), "project_sh_fwd_K1": (2, 9, 64),
    "tile_count": (2, 6, 64), "reduce_grad": (6, 5, 64),
}


@pytest.fixture(scope="module")
def waits():
  return stats.frame_waits()


def test_every_kernel_of_the_table_is_budgeted(waits):
  assert set(waits) == set(BUDGET)


@pytest.mark.parametrize("label", sorted(BUDGET))
def test_round_trips_to_the_first_store(waits, label):
  w = waits[label]
  vmem, smem, vgpr = BUDGET[label]
  print(label, w)
  assert w["vmem_waits"] <= vmem, w
  assert w["smem_waits"] <= smem, w
  assert w["scratch_bytes"] == 0, w
  assert w["vgpr"] <= vgpr, w


def test_scatter_requests_everything_before_its_first_wait(waits):
  """keys, values (the second pass on: the first takes iota) and second values of every round, the digit totals and the
  offset column: no vector load is left behind the single wait."""
  assert waits["rs_scatter_2v_4_8"]["vmem_loads"] == 4 * 3 + 2
  assert waits["rs_scatter_2v_16_8"]["vmem_loads"] == 16 * 3 + 2
  assert waits["rs_scatter_1v_4_9"]["vmem_loads"] == 4 * 2 + 2 + 1          # (two digits per thread: one more word)


def test_tile_count_requests_the_splat_id_in_front_of_the_device_count():
  _, kernels = compiled("binning.hip")
  body = [ln.strip() for ln in kernels[stats.find(kernels, "tile_count_kernel")]["body"]]
  first_vector_load = next(i for i, ln in enumerate(body) if ln.startswith("global_load"))
  count_load = next(i for i, ln in enumerate(body) if ln.startswith("s_load_dword ") and ln.endswith(", 0x0"))
  assert first_vector_load < count_load, (body[first_vector_load], body[count_load])


def test_lds_footprints_are_what_they_were(waits):
  assert waits["project_sh_fwd_K16"]["lds_bytes"] == 51200            # three blocks per CU
  assert waits["project_sh_fwd_K9"]["lds_bytes"] == 28672             # five
  assert waits["rs_scatter_1v_4_9"]["lds_bytes"] == 20512
  assert waits["rs_scatter_2v_16_8"]["lds_bytes"] == 55328
  assert waits["cull_count"]["lds_bytes"] == 0 and waits["cull_write"]["lds_bytes"] == 0

