"""The histogram's entry and bin rules (csrc/gsr_histogram.h) through the host shim -- the source the kernels compile --
against the fp64 oracle (tests/histogram_oracle.py), and ``Histogram`` / ``tensor_histogram`` on CPU tensors: the
numpy path against the shim (the same rule, so the same counts), against ``np.histogram(range=...)``, and the class's
algebra."""
import math

import numpy as np
import pytest
import torch

import histogram_oracle as ho
import hostmath
import splat_trainer_amd as sta
from splat_trainer_amd import _lib
from splat_trainer_amd.histogram import MAX_BINS, _host_histogram

BINS = [1, 10, 64, 256]


@pytest.fixture(scope="module")
def hm(built_libs):
  return hostmath.load(built_libs)


def _bin(hm, t, lo, hi, num_bins, trim):
  t = np.ascontiguousarray(t, np.float32)
  b, o = np.zeros(t.size, np.int32), np.zeros(t.size, np.int32)
  hm.hm_hist_bin(t, t.size, lo, hi, num_bins, int(trim), b, o)
  return b, o


def _shim_histogram(hm, v, rows=None, weight=None, eps=0.0, mode=0, min_value=0.0, range=None, num_bins=64, trim=True):
  counts, stats = np.zeros(num_bins, np.int64), np.zeros(8, np.float64)
  lo, hi = range or (0.0, 0.0)
  code = hm.hm_histogram(np.ascontiguousarray(v, np.float32), v.shape[0], v.shape[1], rows, 0 if rows is None else rows.size,
                         weight, eps, mode, min_value, lo, hi, num_bins, int(range is None), int(trim), counts, stats)
  assert code == 0
  return counts, stats


# --------------------------------------------------------------------------------------------------------- the bin rule
@pytest.mark.parametrize("num_bins", BINS)
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-7.5, 2.25), (1e-3, 1.7e-3), (-3e4, 5e4)])
def test_quarter_bin_offsets_land_in_their_bin(hm, num_bins, lo, hi):
  """Values at the bin centres and a quarter bin to either side: far from every edge, so the counts are exact."""
  width = (hi - lo) / num_bins
  centres = lo + (np.arange(num_bins) + 0.5) * width
  t = np.concatenate([centres - 0.25 * width, centres, centres + 0.25 * width])
  want = np.tile(np.arange(num_bins), 3)
  for trim in (True, False):
    b, o = _bin(hm, t, lo, hi, num_bins, trim)
    assert np.array_equal(b, want) and not o.any()


@pytest.mark.parametrize("num_bins", BINS)
def test_range_ends_and_outside(hm, num_bins):
  lo, hi = np.float32(-2.0), np.float32(3.0)
  below, above = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
  t = np.array([lo, hi, below, above, -1e30, 1e30], np.float32)
  b, o = _bin(hm, t, lo, hi, num_bins, True)
  assert b.tolist() == [0, num_bins - 1, -1, -1, -1, -1] and o.tolist() == [0, 0, 1, 1, 1, 1]     # t == hi: the last bin
  b, o = _bin(hm, t, lo, hi, num_bins, False)
  assert b.tolist() == [0, num_bins - 1, 0, num_bins - 1, 0, num_bins - 1] and o.tolist() == [0, 0, 1, 1, 1, 1]


@pytest.mark.parametrize("num_bins", BINS)
def test_an_empty_range_puts_everything_in_bin_zero(hm, num_bins):
  t = np.array([1.5, -4.0, 1e20, 0.0], np.float32)
  for trim in (True, False):
    b, o = _bin(hm, t, 1.5, 1.5, num_bins, trim)
    assert not b.any() and not o.any()


@pytest.mark.parametrize("num_bins", BINS)
def test_random_values_against_the_fp64_positions(hm, num_bins):
  rng = np.random.default_rng(num_bins)
  t = rng.normal(scale=2.0, size=20000).astype(np.float32)
  lo, hi = -3.0, 4.0
  for trim in (True, False):
    b, o = _bin(hm, t, lo, hi, num_bins, trim)
    counts = np.bincount(b[b >= 0], minlength=num_bins)
    share, worst = ho.compare_counts(counts, t.astype(np.float64), lo, hi, num_bins, trim, label=f"bins={num_bins} trim={trim}")
    print(f"bins={num_bins} trim={trim}: flagged share {share:.5f}, largest cumulative difference {worst}")
    p = (t.astype(np.float64) - lo) * (num_bins / (hi - lo))
    assert int(o.sum()) == int(((p < 0) | (p >= num_bins)).sum())                   # (no value sits on an end here)


# ------------------------------------------------------------------------------------------------------- the entry rule
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -1e-30, 1e-30, 1e-45, 1.0, 3.4e38, 1e-12, 2e-12], np.float32)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("min_value", [0.0, 1e-12])
def test_entry_classes(hm, mode, min_value):
  cls, t = np.zeros(SPECIAL.size, np.int32), np.zeros(SPECIAL.size, np.float32)
  hm.hm_hist_entry(SPECIAL, None, SPECIAL.size, 0.0, mode, min_value, cls, t)
  want_cls, want_t = ho.entries(SPECIAL[:, None], mode=mode, min_value=min_value)
  assert cls.tolist() == want_cls.tolist()
  kept = cls == ho.KEPT
  assert np.all(np.abs(t[kept].astype(np.float64) - want_t[kept]) <= ho.entry_bound(want_t[kept]))
  assert cls[:3].tolist() == [ho.NONFINITE] * 3                                      # NaN and both infinities, every mode
  if mode == 1:
    assert cls[3:7].tolist() == [ho.DROPPED] * 4                                     # zeros and negatives
  if mode == 2 and min_value == 0.0:
    assert cls[3:7].tolist() == [ho.NONFINITE] * 4                                   # log10(0) = -inf is not binned
  if mode == 2 and min_value > 0.0:
    want = math.log10(float(np.float32(min_value)))                                  # every clamped entry: the same value
    assert np.all(t[3:7] == t[3]) and abs(float(t[3]) - want) <= ho.entry_bound(want)


def test_weighted_entries(hm):
  v = np.array([1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
  w = np.array([0.0, 1.0, -1e-3, np.inf, np.nan], np.float32)
  cls, t = np.zeros(5, np.int32), np.zeros(5, np.float32)
  hm.hm_hist_entry(v, w, 5, 1e-3, 0, 0.0, cls, t)
  assert cls.tolist() == [0, 0, 2, 0, 2]                                             # 3 / 0 = inf; 4 / inf = 0; NaN weight
  assert t[0] == np.float32(1.0) / np.float32(1e-3) and t[1] == np.float32(2.0) / (np.float32(1e-3) + np.float32(1.0))
  assert t[3] == 0.0


def test_keys_order_floats(hm):
  x = np.array([-np.inf, -3.4e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.4e38, np.inf], np.float32)
  key, back = np.zeros(x.size, np.uint32), np.zeros(x.size, np.float32)
  hm.hm_hist_keys(x, x.size, key, back)
  assert np.all(np.diff(key.astype(np.int64)) > 0) and key.min() > 0
  assert np.array_equal(back.view(np.uint32), x.view(np.uint32))


# ------------------------------------------------------------------------------------ the whole call, host shim and numpy
def _inputs(n, c, seed):
  rng = np.random.default_rng(seed)
  v = np.exp(3.0 * rng.normal(size=(n, c)) - 6.0).astype(np.float32)
  v.reshape(-1)[::7] = 0.0
  if n > 12:
    v[3], v[5], v[9], v[11, 0] = np.nan, np.inf, -v[9], -np.inf
  w = rng.uniform(0.0, 2.0, n).astype(np.float32)
  w[::5] = 0.0
  rows = rng.integers(0, max(n, 1), n + 3).astype(np.int64) if n else np.zeros(0, np.int64)
  return v, w, rows


@pytest.mark.parametrize("n,c", [(0, 3), (1, 1), (65, 3), (1025, 4), (4099, 3)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_shim_histogram_against_the_oracle(hm, n, c, mode):
  v, w, rows = _inputs(n, c, 7 * n + c)
  min_value = 1e-10 if mode else 0.0
  for use_rows in (False, True):
    for use_weight in (False, True):
      kw = dict(rows=rows if use_rows else None, weight=w if use_weight else None, eps=1e-3, mode=mode, min_value=min_value)
      cls, t = ho.entries(v, **kw)
      kept = t[cls == ho.KEPT]
      for num_bins in BINS:
        for range_, trim in ((None, True), ((-6.0, 1.0), True), ((-6.0, 1.0), False)):
          label = f"n={n} c={c} mode={mode} rows={use_rows} weight={use_weight} bins={num_bins} range={range_} trim={trim}"
          counts, stats = _shim_histogram(hm, v, range=range_, num_bins=num_bins, trim=trim, **kw)
          assert stats[0] == kept.size and stats[5] == (cls == ho.DROPPED).sum() and stats[6] == (cls == ho.NONFINITE).sum(), label
          if kept.size == 0:
            assert not counts.any() and not stats.any() or stats[0] == 0, label
            continue
          assert abs(stats[3] - kept.min()) <= ho.entry_bound(kept.min()) and abs(stats[4] - kept.max()) <= ho.entry_bound(kept.max())
          lo, hi = range_ or (stats[3], stats[4])
          ho.compare_counts(counts, kept, lo, hi, num_bins, trim, ends=range_ is not None, label=label)
          if range_ is None:
            assert stats[7] == 0 and counts.sum() == kept.size, label
            tol_sum, tol_sq = ho.sum_bounds(kept)
            assert abs(stats[1] - kept.sum()) <= tol_sum and abs(stats[2] - (kept * kept).sum()) <= tol_sq, label
          # the numpy path of tensor_histogram states the same rule: the same counts and tallies
          py_counts, py_stats = _host_histogram(v, kw["rows"], kw["weight"], 1e-3, mode, min_value, range_, num_bins, trim)
          assert np.array_equal(py_counts, counts) and np.array_equal(py_stats[[0, 5, 6, 7]], stats[[0, 5, 6, 7]]), label


def test_shim_rejects_what_the_library_rejects(hm):
  v = np.ones((4, 1), np.float32)
  counts, stats = np.zeros(4, np.int64), np.zeros(8, np.float64)
  bad = lambda **kw: hm.hm_histogram(v, 4, 1, None, 0, None, 0.0, kw.get("mode", 0), 0.0, kw.get("lo", 0.0), kw.get("hi", 1.0),
                                     kw.get("num_bins", 4), 0, 1, counts, stats)
  assert bad() == 0
  assert bad(mode=3) == -1 and bad(num_bins=0) == -1 and bad(lo=1.0, hi=0.0) == -1 and bad(hi=float("inf")) == -1


# ------------------------------------------------------------------------------------------------- Histogram on CPU tensors
@pytest.mark.parametrize("num_bins", [1, 10, 64])
def test_cpu_path_equals_numpy_histogram(num_bins):
  gen = torch.Generator().manual_seed(num_bins)
  values = torch.randn(5000, 3, generator=gen)
  h = sta.tensor_histogram(values, num_bins=num_bins, range=(-1.5, 2.0))
  want, edges = np.histogram(values.numpy().ravel(), bins=num_bins, range=(-1.5, 2.0))
  assert h.counts.tolist() == want.tolist()
  assert h.range == (-1.5, 2.0) and h.num_bins == num_bins and h.bin_width == pytest.approx(3.5 / num_bins)
  assert np.allclose(h.bins.numpy(), edges)
  inside = values[(values >= -1.5) & (values <= 2.0)].double()
  assert h.sum == pytest.approx(float(inside.sum()), rel=1e-12) and h.mean == pytest.approx(float(inside.mean()), rel=1e-9)
  assert h.sum_squares == pytest.approx(float((inside ** 2).sum()), rel=1e-12)        # the sum of squares, not the norm
  assert h.std == pytest.approx(float(inside.std()), rel=1e-9)
  assert h.stats["outside"] == values.numel() - inside.numel()


def test_top_edge_is_inclusive_and_auto_range_spans_the_data():
  h = sta.tensor_histogram(torch.tensor([0.0, 0.5, 1.0]), num_bins=2, range=(0.0, 1.0))
  assert h.counts.tolist() == [1, 2]
  h = sta.tensor_histogram(torch.tensor([[3.0, -1.0], [7.0, float("nan")]]), num_bins=4)
  assert h.range == (-1.0, 7.0) and h.counts.tolist() == [1, 0, 1, 1] and h.stats["nonfinite"] == 1


def test_integer_and_half_inputs_and_log_modes():
  assert sta.tensor_histogram(torch.tensor([0, 1, 2, 2], dtype=torch.int16), num_bins=3, range=(0, 3)).counts.tolist() == [1, 1, 2]
  assert sta.tensor_histogram(torch.tensor([0.5, 0.25], dtype=torch.float16), num_bins=2, range=(0, 1)).counts.tolist() == [1, 1]
  v = torch.tensor([0.0, 2e-3, 1.5, 50.0])                                           # log10: -2.7, 0.18, 1.7
  drop = sta.tensor_histogram(v, num_bins=5, range=(-3, 2), log10="drop")
  assert drop.counts.tolist() == [1, 0, 0, 1, 1] and drop.stats["dropped"] == 1
  clamp = sta.tensor_histogram(v, num_bins=5, range=(-3, 2), log10="clamp", min_value=2e-3)
  assert clamp.counts.tolist() == [2, 0, 0, 1, 1]
  rows = sta.tensor_histogram(torch.tensor([[1.0], [2.0], [4.0]]), num_bins=4, range=(0, 4), rows=torch.tensor([2, 2, 0]),
                              weight=torch.tensor([1.0, 5.0, 3.0]), eps=1.0)
  assert rows.counts.tolist() == [1, 2, 0, 0]                                          # 4 / (1 + 3) twice, 1 / (1 + 1)
  with pytest.raises(ValueError):
    sta.tensor_histogram(v, log10="yes")
  with pytest.raises(ValueError):
    sta.tensor_histogram(v, num_bins=MAX_BINS + 1)
  with pytest.raises(ValueError):
    sta.tensor_histogram(v, range=(1, 0))


def test_histogram_algebra():
  a = sta.Histogram(torch.tensor([0.1, 0.2, 0.9]), range=(0, 1), num_bins=10)
  b = sta.Histogram(torch.tensor([0.25, 5.0]), range=(0, 1), num_bins=10)
  total = a + b
  assert total.counts.tolist() == [0, 1, 2, 0, 0, 0, 0, 0, 0, 1] and total.range == (0.0, 1.0)
  assert total.sum == pytest.approx(0.1 + 0.2 + 0.9 + 0.25, rel=1e-6)
  assert total.stats["outside"] == 1 and total.stats["min"] == pytest.approx(0.1) and total.stats["max"] == 5.0
  assert a.append(torch.tensor([0.25, 5.0])).counts.tolist() == total.counts.tolist()
  assert a.append(torch.tensor([5.0]), trim=False).counts.tolist()[-1] == 2
  empty = sta.Histogram.empty((0, 1), 10, device="cpu")
  assert empty.counts.tolist() == [0] * 10 and empty.mean == 0 and empty.std == 0 and (empty + a).counts.tolist() == a.counts.tolist()
  assert (empty + a).stats["min"] == pytest.approx(0.1)
  with pytest.raises(AssertionError):
    a + sta.Histogram(torch.tensor([0.5]), range=(0, 2), num_bins=10)
  assert a.mean == pytest.approx(0.4) and a.std == pytest.approx(float(torch.tensor([0.1, 0.2, 0.9]).std()), rel=1e-6)
  assert repr(a) == repr(a.counts.tolist()) and tuple(a.bin_ranges.shape) == (10, 2)
  assert math.isclose(a.bin_width, 0.1)


def test_the_header_declares_the_entry_point():
  assert "gsr_histogram" in _lib.FUNCTIONS and "gsr_histogram_workspace_bytes" in _lib.FUNCTIONS
  assert _lib.CONSTANTS["GSR_HISTOGRAM_MAX_BINS"] >= 256
