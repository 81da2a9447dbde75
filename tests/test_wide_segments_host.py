"""Host side of segmented wide frames (no GPU: gsr_frame_plan only computes a layout): a wide frame reserves the segment
tables and the wide checkpoint planes whenever segmentation is on, none when it is off, and still needs feature_table."""
import ctypes as C

import splat_trainer_amd as sta
from splat_trainer_amd import _lib

OUT_FIELDS = ("prune_cost", "split_score", "counts", "tile_range", "vis_partial", "indexes", "rows", "screen_scale",
              "jacobian", "visibility", "image", "final_T", "last", "median", "count", "offsets", "vals_a", "vals_b",
              "tvals_a", "tvals_b", "trank_a", "trank_b", "pair_vis", "seg_tables", "seg_pix", "seg_last", "feat_rows",
              "seg_col")


def _plan(C_, seg_pairs, feature_table=1, cap=65_536, N=10_000, W=256, H=256, median=0):
  cfg = sta.RasterConfig()
  f = _lib.GsrFrameC(position=None, N=N, K=1, W=W, H=H, near_plane=0.1, far_plane=100.0, params=_lib.raster_params(cfg),
                     want_median=median, compute_visibility=1, needs_grad=1, seg_pairs=seg_pairs, seg_min_pairs=0,
                     pair_capacity=cap, gaussians2d=1, depth=1, features=1, C=C_, depth_order=None,
                     feature_table=feature_table)
  p = _lib.GsrFramePlanC()
  return _lib.load().gsr_frame_plan(C.byref(f), C.byref(p)), p


def _width(C_):
  return 4 if C_ <= 4 else 8 if C_ <= 8 else 16


def test_wide_frame_plans_segment_tables_and_checkpoint_planes(built_libs):
  for C_, median in ((8, 0), (4, 1), (16, 0), (13, 1)):
    rc, p = _plan(C_, -1, median=median)
    assert rc == 0
    assert p.seg_capacity > 0 and 0 < p.seg_heavy_capacity <= p.seg_capacity
    assert p.seg_tables >= 0 and p.seg_pix >= 0 and p.seg_last >= 0 and p.seg_col >= 0
    # every buffer has a 256-byte aligned range of its own: sorted by offset, each ends before the next begins
    offs = sorted((getattr(p, f), f) for f in OUT_FIELDS if getattr(p, f) >= 0)
    assert all(o % 256 == 0 for o, _ in offs) and len({o for o, _ in offs}) == len(offs)
    nxt = {name: (offs[i + 1][0] if i + 1 < len(offs) else p.out_bytes) for i, (_, name) in enumerate(offs)}
    slots = p.seg_capacity * 256
    assert nxt["seg_col"] - p.seg_col >= 4 * slots * _width(C_)         # CW colours per pixel slot ...
    assert nxt["seg_pix"] - p.seg_pix >= 4 * slots * (2 + median)       # ... next to T, the alpha products (and the median)
    assert nxt["seg_last"] - p.seg_last >= 4 * slots
    assert nxt["seg_col"] <= p.out_bytes
  # the plan does not depend on the channel count except through the colour planes
  a, b = _plan(4, -1)[1], _plan(8, -1)[1]
  assert (a.seg_capacity, a.seg_heavy_capacity) == (b.seg_capacity, b.seg_heavy_capacity)
  narrow = _plan(3, -1, feature_table=0)[1]
  assert narrow.seg_capacity > 0 and narrow.seg_col == -1


def test_wide_frame_without_segmentation_plans_no_segment_buffers(built_libs):
  rc, p = _plan(8, 0)
  assert rc == 0
  assert p.seg_capacity == 0 and p.seg_heavy_capacity == 0
  assert p.seg_tables == -1 and p.seg_pix == -1 and p.seg_last == -1 and p.seg_col == -1
  assert p.feat_rows >= 0
  rc, p = _plan(8, -1, cap=0)
  assert rc == 0 and p.seg_capacity == 0 and p.seg_col == -1


def test_wide_frame_still_needs_the_feature_table(built_libs):
  assert _plan(4, -1, feature_table=0)[0] < 0
  assert _plan(17, -1)[0] < 0


def test_wide_rule_is_the_narrow_one_except_for_the_automatic_length_with_gradients(built_libs):
  lib = _lib.load()

  def thresholds(seg, heavy, O, tiles, grads, wide):
    a, b = C.c_int32(0), C.c_int32(0)
    assert lib.gsr_segment_thresholds_wide(seg, heavy, O, tiles, grads, wide, C.byref(a), C.byref(b)) == 0
    return a.value, b.value

  for O, tiles in ((1_465_883, 8160), (6_593_876, 8160), (100, 12), (0, 100)):
    for grads in (0, 1):
      for seg, heavy in ((8, 8), (16, 32), (8, 10 ** 9), (40, 0), (-1, 900), (-1, 0)):
        narrow = thresholds(seg, heavy, O, tiles, grads, 0)
        a, b = C.c_int32(0), C.c_int32(0)
        assert lib.gsr_segment_thresholds(seg, heavy, O, tiles, grads, C.byref(a), C.byref(b)) == 0
        assert (a.value, b.value) == narrow                      # the entry point without the flag is the narrow rule
        wide = thresholds(seg, heavy, O, tiles, grads, 1)
        if seg > 0 or not grads:
          assert wide == narrow, (O, tiles, grads, seg, heavy)  # explicit values and evaluation frames: one rule
        else:
          assert wide == (256, max(narrow[1], 256)), (O, tiles, seg, heavy, wide)
  assert thresholds(-1, 0, 1_465_883, 8160, 1, 1) == (256, 625)
  # the bound for "at most O pairs" covers the exact bound of every smaller wide frame
  import random
  rnd = random.Random(2)
  for _ in range(1000):
    tiles = rnd.choice([1, 12, 300, 8160, 32400])
    bound = rnd.randint(1, 40_000_000)
    grads = rnd.randint(0, 1)
    seg_cfg, heavy_cfg = rnd.choice([(-1, 0), (-1, 0), (16, 64), (4, 0), (-1, 900)])
    cap_bound = lib.gsr_segment_capacity_wide(bound, 1, seg_cfg, heavy_cfg, tiles, grads, 1)
    hcap_bound = lib.gsr_segment_heavy_capacity_wide(bound, 1, seg_cfg, heavy_cfg, tiles, grads, 1)
    for O in (bound, bound // 2, bound // 7 + 1, rnd.randint(1, bound)):
      seg, heavy = thresholds(seg_cfg, heavy_cfg, O, tiles, grads, 1)
      worst = O // seg + min(tiles, O // (seg + 1))
      assert cap_bound >= min(worst, lib.gsr_segment_capacity_wide(O, 0, seg_cfg, heavy_cfg, tiles, grads, 1)), (tiles, bound, O)
      piece = max(seg, min(256, (heavy // 2) & ~3), 1)
      worst_heavy = O // piece + min(tiles, O // (heavy + 1))
      assert hcap_bound >= min(worst_heavy, lib.gsr_segment_heavy_capacity_wide(O, 0, seg_cfg, heavy_cfg, tiles, grads, 1)), (tiles, bound, O)
