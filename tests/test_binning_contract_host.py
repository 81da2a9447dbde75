"""The binning / reduction contract (tests/binning_contract.py) on the CPU: the reference against brute force, the
comparator against planted defects in its input data, the project's own tile maths (gsr_math.h compiled for the host)
through the comparator, and the reduction model against its fp64 bound."""
import numpy as np
import pytest

import binning_contract as bc
import hostmath
from splat_trainer_amd import _lib

CASES = [c.name for c in bc.binning_cases()]


def _params():
  return _lib.GsrRasterParamsC(**bc.PARAMS)


def _bits(masks, case):
  return np.stack([(masks & 1) != 0, (masks & 2) != 0], axis=-1).reshape(case.M, case.tiles_y, case.tiles_x, 2)


# ------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("name", CASES)
def test_need_lies_inside_firm_hit_plus_undecided(name):
  case = bc.binning_case(name)
  assert not (case.ref.firm_hit & case.ref.firm_miss).any()
  lost = case.need & case.ref.firm_miss
  assert not lost.any(), np.argwhere(lost)[:5]
  if case.family not in ("map edge", "counts"):
    assert case.need.any() and case.ref.firm_miss.any()


def test_undecided_share_stays_under_the_cap():
  stats = bc.family_stats(bc.binning_cases())
  for family, s in stats.items():
    print(f"{family:10s} firm hits {s['firm_hit']:7d}  undecided {s['undecided']:5d}  share {100 * s['share']:.4f} %  "
          f"max rho {s['max_rho']:.3e}")
  assert set(stats) == {"grid", "needles", "giants", "map edge", "tiny", "counts"}
  for family, s in stats.items():
    assert s["firm_hit"] > 0 and s["share"] <= bc.UNDECIDED_CAP, (family, s)


def test_cases_reach_every_path(built_libs):
  shim = hostmath.load(built_libs)
  area = lambda e: (e[:, 1] - e[:, 0]) * (e[:, 3] - e[:, 2])
  for name, placed in (("map edge wide", bc.MAP_EDGE_WIDE), ("map edge tall", bc.MAP_EDGE_TALL)):
    case = bc.binning_case(name)
    ext, _ = bc.shim_extents(shim, _params(), case)
    want = np.array([[x0, x0 + nx, y0, y0 + ny] for nx, ny, x0, y0 in placed], np.int32)
    assert np.array_equal(ext, want)
    assert not case.ref.undecided.any()                      # no splat of this family has an undecided column or half
  both = np.concatenate([area(bc.shim_extents(shim, _params(), bc.binning_case(n))[0]) for n in ("map edge wide", "map edge tall")])
  assert (both == 32).sum() >= 6 and (both == 33).sum() >= 3
  giants = bc.binning_case("giants")
  ext, _ = bc.shim_extents(shim, _params(), giants)
  assert giants.M == 65 and (area(ext) > bc.MAP_TILES).all() and area(ext).max() >= 300
  needles = area(bc.shim_extents(shim, _params(), bc.binning_case("needles"))[0])
  assert (needles > bc.MAP_TILES).any() and ((needles > 0) & (needles <= bc.MAP_TILES)).any()
  grid = bc.binning_case("grid")
  op = grid.rows[:, 5]
  thr = np.float32(bc.PARAMS["alpha_threshold"])
  assert (op < thr).any() and (op == thr).any() and (op == np.float32(1)).any() and (op == np.float32(0.02)).any()
  assert grid.tiles_x * 16 > grid.W and grid.tiles_y * 16 > grid.H          # partial right and bottom tiles


# --------------------------------------------------------------------------------------- the comparator, planted defects
def _clean():
  case = bc.binning_case("grid")
  fh = case.ref.firm_hit.reshape(case.M, case.num_tiles, 2)
  masks = (fh[..., 0] | (fh[..., 1].astype(np.uint8) << 1)).astype(np.uint8)
  return case, masks, bc.emit(masks, case.order, case.M)


def _slot(case, out, want):
  """First (rank, slot) whose (splat, tile, mask) satisfies `want`."""
  fh = case.ref.firm_hit.reshape(case.M, case.num_tiles, 2)
  fm = case.ref.firm_miss.reshape(case.M, case.num_tiles, 2)
  for k in range(case.M):
    s = int(case.order[k])
    for i in range(int(out["offsets"][k]), int(out["offsets"][k] + out["count"][k])):
      t, mask = int(out["keys"][i]), int(out["inst"][i] >> 30)
      if want(fh[s, t], fm[s, t], mask):
        return k, i
  raise AssertionError("the case holds no such slot")


def _drop_firm_hit(case, out):
  _, i = _slot(case, out, lambda fh, fm, mask: mask == 3)
  out["inst"][i] &= np.uint32(~(1 << 30) & 0xFFFFFFFF)
  return "firm hit but was not emitted"


def _add_firm_miss(case, out):
  _, i = _slot(case, out, lambda fh, fm, mask: mask == 1 and fm[1])
  out["inst"][i] |= np.uint32(2 << 30)
  return "firm miss but was emitted"


def _swap_half_bits(case, out):
  _, i = _slot(case, out, lambda fh, fm, mask: mask == 2 and fm[0])
  out["inst"][i] ^= np.uint32(3 << 30)
  return "firm"


def _rotate_keys(case, out):
  k = int(np.flatnonzero(out["count"] >= 3)[0])
  b, n = int(out["offsets"][k]), int(out["count"][k])
  out["keys"][b:b + n], out["inst"][b:b + n] = np.roll(out["keys"][b:b + n], 1), np.roll(out["inst"][b:b + n], 1)
  return "ascending row-major order"


def _wrong_splat_id(case, out):
  i = int(out["total"]) // 2
  out["inst"][i] = (out["inst"][i] & np.uint32(0xC0000000)) | ((out["inst"][i] + np.uint32(1)) & np.uint32(0x3FFFFFFF))
  return "carries splat id"


def _count_off_by_one(case, out):
  out["count"][int(np.flatnonzero(out["count"])[3])] += 1
  return "exclusive scan"


def _write_beyond_capacity(case, out):
  out["keys"][out["capacity"]] = 0
  return "was written"


DEFECTS = [_drop_firm_hit, _add_firm_miss, _swap_half_bits, _rotate_keys, _wrong_splat_id, _count_off_by_one,
           _write_beyond_capacity]


def test_comparator_accepts_a_conforming_emission():
  case, masks, out = _clean()
  assert out["total"] > 1000
  assert bc.compare(case.ref, case.order, case.M, out, case.num_tiles) == []
  assert np.array_equal(bc.decode(case.order, case.M, out, case.num_tiles), masks)
  for live in bc.m_dev_values(case.M):
    assert bc.compare(case.ref, case.order, live, bc.emit(masks, case.order, live), case.num_tiles) == []
  for capacity in (0, 1, out["total"] // 2, out["total"] - 1):
    assert bc.compare(case.ref, case.order, case.M, bc.emit(masks, case.order, case.M, capacity), case.num_tiles) == []


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda f: f.__name__.strip("_"))
def test_comparator_reports_a_planted_defect(defect):
  case, masks, out = _clean()
  if defect is _write_beyond_capacity:
    out = bc.emit(masks, case.order, case.M, out["total"] // 2)
  words = defect(case, out)
  found = bc.compare(case.ref, case.order, case.M, out, case.num_tiles)
  assert any(words in line for line in found), found


# -------------------------------------------------------------------------- the project's tile maths through the contract
@pytest.mark.parametrize("name", CASES)
def test_host_tile_maths_meet_the_contract(built_libs, name):
  case = bc.binning_case(name)
  masks = bc.shim_masks(hostmath.load(built_libs), _params(), case)
  assert bc.compare(case.ref, case.order, case.M, bc.emit(masks, case.order, case.M), case.num_tiles) == []
  lost = case.need & ~_bits(masks, case)
  assert not lost.any(), np.argwhere(lost)[:5]


# ------------------------------------------------------------------------------------------------ the reduction model
def test_tree_is_the_balanced_pairwise_tree():
  x = (10.0 ** np.random.default_rng(1).uniform(-6, 3, 64)).astype(np.float32)
  rows = [x[16 * r:16 * r + 16] for r in range(4)]
  def row15(r):                                                # lane 15 after row_shr 1, 2, 4, 8: written out by hand
    p = [r[2 * i + 1] + r[2 * i] for i in range(8)]
    q = [p[2 * i + 1] + p[2 * i] for i in range(4)]
    return (q[3] + q[2]) + (q[1] + q[0])
  r = [row15(v) for v in rows]
  assert bc.tree64(x) == (r[3] + r[2]) + (r[1] + r[0])
  assert bc.model_sum(np.ones((65, 1), np.float32))[0] == 65


def test_reduction_cases_hold_every_placement():
  seen = set()
  for M in bc.REDUCTION_M:
    c = bc.reduction_case(M)
    seen |= c.features()
    assert set(np.unique(c.count)) <= set(bc.REDUCTION_COUNTS)
    assert 0.2 < (c.vis == 0).mean() < 0.4 or M == 1
    assert np.isnan(c.partial[c.vis == 0]).all() and np.isfinite(c.partial[c.vis > 0]).all()
  assert seen == bc.REDUCTION_FEATURES
  assert set(np.unique(np.concatenate([bc.reduction_case(M).count for M in bc.REDUCTION_M]))) == set(bc.REDUCTION_COUNTS)
  assert [bc.wide_cw(C) for C in bc.WIDE_C] == [4, 8, 8, 16]


@pytest.mark.parametrize("M", bc.REDUCTION_M)
def test_reduction_model_within_the_fp64_bound(M):
  c = bc.reduction_case(M)
  vis, sums = bc.reduction_model(M)
  assert np.isfinite(vis).all() and np.isfinite(sums).all()
  d_vis = bc.fp64_distance(c.vis[:, None], c.vis, c.offsets, c.count, False, vis[:, None])
  d_sum = bc.fp64_distance(c.partial, c.vis, c.offsets, c.count, True, sums)
  print(f"M={M}: slots {c.O}, model against fp64 relative to (n-1) u sum|x|: visibility {d_vis:.3f}, gradients {d_sum:.3f}")
  assert d_vis <= 1.0 and d_sum <= 1.0
  limit = c.O // 2
  cut = bc.reduction_model(M, limit)[0]
  whole = bc.model_reduce(np.where(np.arange(c.O) < limit, c.vis, 0)[:, None], c.vis, c.offsets, c.count, gate=False)[:, 0]
  assert np.array_equal(cut, whole)


def test_reversing_the_slot_order_changes_the_bits():
  c = bc.reduction_case(700)
  _, sums = bc.reduction_model(700)
  flipped = c.partial.copy()
  vis = c.vis.copy()
  for b, n in zip(c.offsets.astype(np.int64), c.count.astype(np.int64)):
    flipped[b:b + n], vis[b:b + n] = c.partial[b:b + n][::-1], c.vis[b:b + n][::-1]
  other = bc.model_reduce(flipped, vis, c.offsets, c.count, gate=True)
  serial, grouped = (c.count > 1) & (c.count <= bc.SERIAL), c.count > bc.SERIAL
  assert (other[serial] != sums[serial]).any() and (other[grouped] != sums[grouped]).any()
