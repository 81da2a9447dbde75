"""The histogram kernels (csrc/histogram.hip) through ``tensor_histogram`` against the fp64 oracle
(tests/histogram_oracle.py, where the per-entry bound and the flip band are derived).

Shapes: N in {0, 1, 63, 64, 65, 257, 1023, 1024, 1025, 4099, 70001} -- the last runs many blocks and, with four channels
and a gather, the grid-stride tail -- C in {1, 3, 4} (C = 4 takes the 16-byte loads, the flat form takes them for every
C, with a scalar tail when N C is no multiple of four), num_bins in {1, 10, 64, 256}, with and without ``rows`` (repeated,
unsorted) and ``weight``.  Inputs: magnitudes exp(3 z - 6), every seventh entry zero, planted NaN / inf / negative rows.
One set of 70001 x 4 values serves every shape (a smaller one takes the leading rows and columns); the fp64 entries of a
(shape, rows, weight, mode) are computed once and serve every bin count and range.

The bound on log10f is the 2 ulp of the HIP math documentation (the ROCm installation's own tables state no other).

Asserted: kept / dropped / non-finite counts exact; with a found range nothing is outside and every kept entry is binned;
with a given range the outside count obeys the flip rule at the two ends; minimum and maximum within the per-entry bound;
sums of t within sum e_i + n 2^-52 sum |t_i| and of t^2 within sum 2 |t_i| e_i + n 2^-52 sum t_i^2; cumulative counts
under the flip rule with at most 1 % of the kept entries inside a band; two runs bit-identical; a found range
bit-identical to the given-range call with the (lo, hi) it reports."""
import numpy as np
import pytest
import torch

import histogram_oracle as ho
import splat_trainer_amd as sta

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257, 1023, 1024, 1025, 4099, 70001]
CHANNELS = [1, 3, 4]
BINS = [1, 10, 64, 256]
FULL = 70001
EPS = 1e-3
FIXED = (-6.0, 1.0)
MODES = {None: 0, "drop": 1, "clamp": 2}


@pytest.fixture(scope="module")
def data():
  """Host arrays, never modified: values (70001, 4), weight (70001,), and a gather list per N."""
  rng = np.random.default_rng(22)
  v = np.exp(3.0 * rng.normal(size=(FULL, 4)) - 6.0).astype(np.float32)
  v.reshape(-1)[::7] = 0.0
  v[3], v[17], v[40], v[41, 0], v[900] = np.nan, np.inf, -v[40], -np.inf, -1.0
  w = rng.uniform(0.0, 2.0, FULL).astype(np.float32)
  w[::5] = 0.0
  rows = {n: rng.integers(0, n, n + 3).astype(np.int64) if n else np.zeros(0, np.int64) for n in SIZES}
  return dict(v=v, w=w, rows=rows)


def _raw(h):
  return h._buffer.cpu().numpy().tobytes()


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("n", SIZES)
def test_histogram_against_the_oracle(data, n, c):
  v_host = np.ascontiguousarray(data["v"][:n, :c])
  v, w = torch.from_numpy(v_host).cuda(), torch.from_numpy(data["w"][:n].copy()).cuda()
  rows_host = data["rows"][n]
  rows = torch.from_numpy(rows_host).cuda()
  for use_rows in (False, True):
    for use_weight in (False, True):
      gather = dict(rows=rows if use_rows else None, weight=w if use_weight else None, eps=EPS)
      for log10, min_value, bins in (("drop", 1e-10, BINS), ("clamp", 1e-8, [64]), (None, 0.0, [10])):
        cls, t = ho.entries(v_host, rows_host if use_rows else None, data["w"][:n] if use_weight else None, EPS,
                            MODES[log10], min_value)
        kept = t[cls == ho.KEPT]
        for num_bins in bins:
          label = f"N={n} C={c} rows={use_rows} weight={use_weight} log10={log10} bins={num_bins}"
          call = lambda **kw: sta.tensor_histogram(v, num_bins=num_bins, log10=log10, min_value=min_value, **gather, **kw)
          found = call()
          ho.check_histogram(label + " found range", found, cls, kept, num_bins, None, True)
          assert _raw(call()) == _raw(found), label                                  # bit-identical from run to run
          if kept.size:
            again = call(range=found.range)
            assert again.range == found.range and _raw(again) == _raw(found), label  # ... and to the given-range call
          if num_bins in (10, 64):
            given = FIXED if log10 else (-0.001, 0.01)
            for trim in (True, False):
              h = call(range=given, trim=trim)
              ho.check_histogram(label + f" range={given} trim={trim}", h, cls, kept, num_bins, given, trim)
              assert _raw(call(range=given, trim=trim)) == _raw(h), label


def test_empty_inputs_launch_nothing_and_return_zeros():
  for h in (sta.tensor_histogram(torch.zeros(0, 3, device="cuda"), num_bins=10),
            sta.tensor_histogram(torch.ones(5, 3, device="cuda"), num_bins=10, rows=torch.zeros(0, dtype=torch.int64, device="cuda"))):
    assert h.counts.tolist() == [0] * 10 and h.range == (0.0, 0.0) and not any(h.stats.values())


def test_rows_outside_the_tensor_are_not_read():
  v = torch.ones(4, 3, device="cuda")
  h = sta.tensor_histogram(v, num_bins=2, range=(0, 2), rows=torch.tensor([0, 9, -1, 3], device="cuda"))
  assert h.counts.tolist() == [0, 6] and h.stats["nonfinite"] == 6


def test_integer_half_and_maximum_bins():
  h = sta.tensor_histogram(torch.arange(0, 2048, device="cuda", dtype=torch.int32) % 1024, num_bins=1024, range=(0, 1024))
  assert h.counts.tolist() == [2] * 1024                                             # the per-block counters above 256 bins
  h = sta.tensor_histogram(torch.tensor([0.5, 0.25, 0.75], device="cuda", dtype=torch.float16), num_bins=2, range=(0, 1))
  assert h.counts.tolist() == [1, 2]
  a = sta.Histogram(torch.tensor([0.1, 0.2, 0.9], device="cuda"), range=(0, 1), num_bins=10)
  total = a.append(torch.tensor([0.25, 5.0], device="cuda"))
  assert total.counts.tolist() == [0, 1, 2, 0, 0, 0, 0, 0, 0, 1] and total.stats["outside"] == 1 and total.device.type == "cuda"
