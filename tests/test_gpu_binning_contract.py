"""K4 tile binning and the deterministic per-splat reductions on the GPU through the C ABI, against the stage contract of
tests/binning_contract.py: an fp64 reference with derived bands for the binning, a bit-exact numpy fp32 model for the
reductions.  Every figure is printed as a CONTRACT line (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import binning_contract as bc
import hostmath
from splat_trainer_amd import _lib

pytestmark = pytest.mark.gpu

CASES = [c.name for c in bc.binning_cases()]
CANARY_F = -77.25


def _ptr(t):
  return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
  a = np.ascontiguousarray(a)
  return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _canary(*shape):
  return _dev(np.full(shape, bc.CANARY, np.uint32))


def _u32(t):
  return t.cpu().numpy().view(np.uint32)


def _params():
  return _lib.GsrRasterParamsC(**bc.PARAMS)


def _count(case, m_dev=None, fused=True, rows=None, order=None, size=None):
  """gsr_tile_count_offsets (or gsr_tile_count + the scan): (count, offsets, total, hit records) with the inputs."""
  lib, params = _lib.load(), _params()
  W, H = size or (case.W, case.H)
  rows, order = _dev(case.rows if rows is None else rows), _dev(case.order if order is None else order)
  M = order.numel()
  count, offsets, hits, total = _canary(M), _canary(M), _canary(M, 4), _canary(1)
  flag = torch.zeros(1, dtype=torch.int32, device="cuda")
  md = _dev(np.array([m_dev], np.uint32)) if m_dev is not None else None
  if fused:
    nbytes = lib.gsr_tile_count_offsets_workspace_bytes(M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.gsr_tile_count_offsets(_ptr(rows), _ptr(order), M, W, H, C.byref(params), _ptr(count), _ptr(hits),
                                          _ptr(md), _ptr(offsets), _ptr(total), _ptr(flag), _ptr(ws), nbytes, _stream()),
               "tile_count_offsets")
  else:
    _lib.check(lib.gsr_tile_count(_ptr(rows), _ptr(order), M, W, H, C.byref(params), _ptr(count), _ptr(hits), _ptr(md),
                                  _stream()), "tile_count")
    nbytes = lib.gsr_scan_workspace_bytes(M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.gsr_exclusive_scan_u32_checked(_ptr(count), _ptr(offsets), M, _ptr(total), _ptr(flag), _ptr(ws), nbytes,
                                                  _stream()), "scan")
  assert flag.item() == 0
  return dict(rows=rows, order=order, md=md, M=M, W=W, H=H, d_count=count, d_offsets=offsets, d_hits=hits,
              count=_u32(count), offsets=_u32(offsets), hits=_u32(hits), total=int(_u32(total)[0]))


def _emit(c, capacity=None):
  """gsr_tile_emit into canary-filled buffers of 8 slots more than the total: the emission in the comparator's layout."""
  lib, params = _lib.load(), _params()
  slots = c["total"] + 8
  keys, inst = _canary(slots), _canary(slots)
  _lib.check(lib.gsr_tile_emit(_ptr(c["rows"]), _ptr(c["order"]), _ptr(c["d_offsets"]), _ptr(c["d_hits"]), c["M"], c["W"],
                               c["H"], C.byref(params), _ptr(keys), _ptr(inst), c["total"] if capacity is None else capacity,
                               _ptr(c["md"]), _stream()), "tile_emit")
  return dict(count=c["count"], offsets=c["offsets"], total=c["total"], keys=_u32(keys), inst=_u32(inst),
              capacity=capacity, d_keys=keys, d_inst=inst)


def _bits(masks, case):
  return np.stack([(masks & 1) != 0, (masks & 2) != 0], axis=-1).reshape(case.M, case.tiles_y, case.tiles_x, 2)


# ------------------------------------------------------------------------------------------------------------- binning
@pytest.mark.parametrize("name", CASES)
def test_count_and_emit_meet_the_contract(built_libs, name):
  case = bc.binning_case(name)
  c = _count(case)
  out = _emit(c)
  assert bc.compare(case.ref, case.order, case.M, out, case.num_tiles) == []
  masks = bc.decode(case.order, case.M, out, case.num_tiles)
  lost = case.need & ~_bits(masks, case)
  assert not lost.any(), np.argwhere(lost)[:5]
  # the count and the scan in separate launches: the same counts, offsets, total and hit records
  two = _count(case, fused=False)
  for key in ("count", "offsets", "hits", "total"):
    assert np.array_equal(two[key], c[key]), key
  again = _emit(_count(case))
  assert np.array_equal(again["keys"], out["keys"]) and np.array_equal(again["inst"], out["inst"])
  host = bc.shim_masks(hostmath.load(built_libs), _params(), case)
  differ = np.argwhere(host != masks)
  s = case.ref.stats()
  print(f"\nCONTRACT binning {name}: {case.M} ranks, {out['total']} tiles emitted, firm-hit halves {s['firm_hit']}, undecided "
        f"{s['undecided']} ({100 * s['share']:.4f} %), max rho {s['max_rho']:.3e}, undecided halves emitted "
        f"{int((_bits(masks, case) & case.ref.undecided).sum())}, host shim and device differ at {len(differ)} (splat, tile)"
        + (f": {differ[:4].tolist()}" if len(differ) else ""))


def test_undecided_share_stays_under_the_cap():
  for family, s in bc.family_stats(bc.binning_cases()).items():
    print(f"\nCONTRACT family {family}: firm-hit halves {s['firm_hit']}, undecided {s['undecided']} "
          f"({100 * s['share']:.4f} %), max rho {s['max_rho']:.3e}")
    assert s["share"] <= bc.UNDECIDED_CAP, (family, s)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
def test_ranks_behind_the_device_count(M):
  case = bc.binning_case(f"counts M={M}")
  whole = _count(case)
  full = _emit(whole)
  for m_dev in bc.m_dev_values(M):
    for fused in (True, False):
      c = _count(case, m_dev=m_dev, fused=fused)
      out = _emit(c)
      assert bc.compare(case.ref, case.order, m_dev, out, case.num_tiles) == [], (m_dev, fused)
      assert not c["count"][m_dev:].any() and np.array_equal(c["count"][:m_dev], whole["count"][:m_dev])
      assert (c["hits"][m_dev:] == bc.CANARY).all() and np.array_equal(c["hits"][:m_dev], whole["hits"][:m_dev])
      assert c["total"] == int(whole["count"][:m_dev].sum())
      assert np.array_equal(out["keys"][:c["total"]], full["keys"][:c["total"]])
      assert np.array_equal(out["inst"][:c["total"]], full["inst"][:c["total"]])


@pytest.mark.parametrize("name", ["grid", "needles", "giants", "map edge wide"])
def test_capacity_truncates_the_emit(name):
  case = bc.binning_case(name)
  c = _count(case)
  full = _emit(c)
  total = c["total"]
  assert total > 8
  for capacity in (0, 1, total // 2, total - 1, total):
    out = _emit(c, capacity)
    for key in ("keys", "inst"):
      assert np.array_equal(out[key][:capacity], full[key][:capacity]), (capacity, key)
      assert (out[key][capacity:] == bc.CANARY).all(), (capacity, key)
    assert bc.compare(case.ref, case.order, case.M, out, case.num_tiles) == []


def test_map_and_wave_paths_agree():
  """The same splat on 640 x 360, where its extent takes the wave path, and moved by whole tiles onto a 128 x 64 image whose
  8 x 4 tiles take the 64-bit map: every tile of the window gets the same half mask.  The means sit on a 1/256 px grid, so
  the move is exact in fp32 and both runs see the same pixel offsets."""
  rng = np.random.default_rng(3130)
  W, H, n = 640, 360, 24
  s1 = np.r_[bc._log_uniform(rng, 40.0, 300.0, n // 2), bc._log_uniform(rng, 60.0, 150.0, n // 2)]
  s2 = np.r_[bc._log_uniform(rng, 40.0, 300.0, n // 2), bc._log_uniform(rng, 0.55, 8.0, n // 2)]
  rows = bc.conic_rows(np.round(rng.uniform(0, W, n) * 256) / 256, np.round(rng.uniform(0, H, n) * 256) / 256, s1, s2,
                       rng.uniform(0, np.pi, n), rng.uniform(0.3, 1.0, n))
  big = bc.Case("paths", "paths", W, H, rows, np.arange(n))
  c = _count(big)
  wave = np.flatnonzero((c["hits"][:, 1] >> 16) != 0)             # the extents flagged for the wave path
  assert len(wave) >= 16
  full = bc.decode(big.order, n, _emit(c), big.num_tiles).reshape(n, big.tiles_y, big.tiles_x)
  moved, where = [], []
  for s in wave:
    ys, xs = np.nonzero(full[s])
    for wy in range(4 * (ys.min() // 4), ys.max() + 1, 4):
      for wx in range(8 * (xs.min() // 8), xs.max() + 1, 8):
        r = rows[s].copy()
        r[0], r[1] = r[0] - np.float32(16 * wx), r[1] - np.float32(16 * wy)
        assert float(r[0]) == float(rows[s, 0]) - 16 * wx and float(r[1]) == float(rows[s, 1]) - 16 * wy
        moved.append(r)
        where.append((s, wx, wy))
  keep = rng.permutation(len(moved))[:700]
  moved, where = np.stack(moved)[keep], [where[i] for i in keep]
  small = _count(None, rows=moved, order=np.arange(len(moved), dtype=np.uint32), size=(128, 64))
  assert ((small["hits"][:, 1] >> 16) == 0).all()                # ... and every window for the map
  got = bc.decode(np.arange(len(moved)), len(moved), _emit(small), 32).reshape(len(moved), 4, 8)
  compared = differing = 0
  for i, (s, wx, wy) in enumerate(where):
    want = full[s, wy:wy + 4, wx:wx + 8]
    window = got[i, :want.shape[0], :want.shape[1]]
    compared += int((want | window).astype(bool).sum())
    differing += int((want != window).sum())
  print(f"\nCONTRACT paths: {len(where)} windows of {len(wave)} splats, {compared} hit tiles compared, {differing} differ")
  assert compared > 5000 and differing == 0


@pytest.mark.parametrize("name", ["grid", "needles"])
def test_sort_and_ranges_give_each_tile_its_splats_in_depth_order(name):
  lib = _lib.load()
  case = bc.binning_case(name)
  out = _emit(_count(case))
  O = out["total"]
  ka, v2a = out["d_keys"][:O].clone(), out["d_inst"][:O].clone()
  va, kb, vb, v2b = (torch.zeros_like(ka) for _ in range(4))
  nbytes = lib.gsr_sort_workspace_bytes(O)
  ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
  bits = max(1, int(case.num_tiles - 1).bit_length())
  where = _lib.check(lib.gsr_sort_pairs2_u32(_ptr(ka), _ptr(va), _ptr(v2a), _ptr(kb), _ptr(vb), _ptr(v2b), O, 1, 0, bits,
                                             _ptr(ws), nbytes, None, _stream()), "sort2")
  k, v, v2 = (kb, vb, v2b) if where == 1 else (ka, va, v2a)
  ranges = torch.zeros(case.num_tiles, 2, dtype=torch.int32, device="cuda")
  _lib.check(lib.gsr_tile_ranges(_ptr(k), O, case.num_tiles, _ptr(ranges), None, _stream()), "ranges")
  k, v, v2, ranges = _u32(k), _u32(v), _u32(v2), _u32(ranges)
  perm = np.argsort(out["keys"][:O], kind="stable")
  assert np.array_equal(k, out["keys"][:O][perm]) and np.array_equal(v, perm.astype(np.uint32))
  assert np.array_equal(v2, out["inst"][:O][perm])
  rank = np.empty(case.M, np.int64)
  rank[case.order.astype(np.int64)] = np.arange(case.M)
  fh = case.ref.firm_hit.reshape(case.M, case.num_tiles, 2).any(axis=2)
  fm = case.ref.firm_miss.reshape(case.M, case.num_tiles, 2).all(axis=2)
  assert int(ranges[:, 1].astype(np.int64).sum() - ranges[:, 0].astype(np.int64).sum()) == O
  for t in range(case.num_tiles):
    ids = (v2[ranges[t, 0]:ranges[t, 1]] & np.uint32(0x3FFFFFFF)).astype(np.int64)
    assert (k[ranges[t, 0]:ranges[t, 1]] == t).all()
    assert (np.diff(rank[ids]) > 0).all(), t                    # depth-rank order, no splat twice
    listed = np.zeros(case.M, bool)
    listed[ids] = True
    assert not (fh[:, t] & ~listed).any() and not (fm[:, t] & listed).any(), t


# ---------------------------------------------------------------------------------------------------------- reductions
def _reduce_vis(c, order, m_dev=None, capacity=None, vis=None):
  lib = _lib.load()
  out = torch.full((c.M,), CANARY_F, device="cuda")
  d_vis, d_offsets, d_count = _dev(c.vis if vis is None else vis), _dev(c.offsets), _dev(c.count)
  d_order = _dev(order) if order is not None else None
  md = _dev(np.array([m_dev], np.uint32)) if m_dev is not None else None
  _lib.check(lib.gsr_reduce_visibility(_ptr(d_vis), _ptr(d_offsets), _ptr(d_count), _ptr(d_order), c.M, _ptr(out),
                                       c.O if capacity is None else capacity, _ptr(md), _stream()), "reduce_visibility")
  return out.cpu().numpy()


def _reduce_grad(c, order, C_wide=None):
  lib = _lib.load()
  rows = torch.full((c.M, 16), CANARY_F, device="cuda")
  d_vis, d_offsets, d_count = _dev(c.vis), _dev(c.offsets), _dev(c.count)     # (held: the calls take raw addresses)
  d_order = _dev(order) if order is not None else None
  args = (_ptr(d_vis), _ptr(d_offsets), _ptr(d_count), _ptr(d_order), c.M)
  if C_wide is None:
    partial = _dev(c.partial[:, :12])
    _lib.check(lib.gsr_reduce_gradients(_ptr(partial), *args, _ptr(rows), _stream()), "reduce_gradients")
    return rows.cpu().numpy(), None
  feat = torch.full((c.M, C_wide), CANARY_F, device="cuda")
  partial = _dev(c.partial[:, :8 + bc.wide_cw(C_wide)])
  _lib.check(lib.gsr_reduce_gradients_wide(_ptr(partial), *args, C_wide, _ptr(rows), _ptr(feat), _stream()),
             "reduce_gradients_wide")
  return rows.cpu().numpy(), feat.cpu().numpy()


def _same_bits(a, b):
  return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _by_splat(values, order):
  out = np.empty_like(values)
  out[np.arange(len(values)) if order is None else order.astype(np.int64)] = values
  return out


@pytest.mark.parametrize("M", bc.REDUCTION_M)
def test_reduce_visibility_equals_the_model(M):
  c = bc.reduction_case(M)
  model = bc.reduction_model(M)[0]
  for order in (c.order, None):
    got = _reduce_vis(c, order)
    assert np.isfinite(got).all() and _same_bits(got, _by_splat(model, order))
    assert _same_bits(_reduce_vis(c, order), got)                # two runs: equal bits
  for m_dev in bc.m_dev_values(M):
    got = _reduce_vis(c, c.order, m_dev=m_dev)
    want = np.full(M, CANARY_F, np.float32)
    want[c.order[:m_dev].astype(np.int64)] = model[:m_dev]
    assert _same_bits(got, want), m_dev
  # a speculative launch: the buffer holds `capacity` slots, NaN lies behind them
  for capacity in (0, 1, c.O // 2, c.O - 1):
    vis = c.vis.copy()
    vis[capacity:] = np.nan
    got = _reduce_vis(c, c.order, capacity=capacity, vis=vis)
    assert np.isfinite(got).all() and _same_bits(got, _by_splat(bc.reduction_model(M, capacity)[0], c.order)), capacity


@pytest.mark.parametrize("M", bc.REDUCTION_M)
def test_reduce_gradients_equals_the_model(M):
  c = bc.reduction_case(M)
  for order in (c.order, None):
    rows, _ = _reduce_grad(c, order)
    assert np.isfinite(rows).all() and _same_bits(rows, bc.narrow_rows(M, order))
    assert _same_bits(_reduce_grad(c, order)[0], rows)           # two runs: equal bits
    assert _same_bits(rows[:, 11], _reduce_vis(c, order))        # the visibility column: gsr_reduce_visibility's bits
  d = bc.fp64_distance(c.partial, c.vis, c.offsets, c.count, True, bc.reduction_model(M)[1])
  print(f"\nCONTRACT reductions M={M}: {c.O} slots, largest rank {int(c.count.max())}, device = model in every bit "
        f"(visibility, narrow); model against fp64 at {d:.3f} of (n-1) u sum|x|")


@pytest.mark.parametrize("C_wide", bc.WIDE_C)
@pytest.mark.parametrize("M", bc.REDUCTION_M)
def test_reduce_gradients_wide_equals_the_model(M, C_wide):
  c = bc.reduction_case(M)
  for order in (c.order, None):
    rows, feat = _reduce_grad(c, order, C_wide)
    want_rows, want_feat = bc.wide_rows(M, C_wide, order)
    assert np.isfinite(rows).all() and np.isfinite(feat).all()
    assert _same_bits(rows, want_rows) and _same_bits(feat, want_feat)
    again = _reduce_grad(c, order, C_wide)
    assert _same_bits(again[0], rows) and _same_bits(again[1], feat)
    narrow, _ = _reduce_grad(c, order)                           # columns 0-7 and the visibility: the narrow form's bits
    assert _same_bits(rows[:, :8], narrow[:, :8]) and _same_bits(rows[:, 11], narrow[:, 11])
    assert _same_bits(feat[:, :3], narrow[:, 8:11])
