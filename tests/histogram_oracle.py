"""The fp64 statement of the histogram contract (include/gsplat_hip.h, csrc/gsr_histogram.h) in numpy, and the rule by
which a float32 histogram is compared with it.  Shared by test_histogram_host.py (the host shim, the numpy path) and
test_gpu_histogram.py (the kernels).

Per-entry bound.  The transformed value t of an entry differs from its fp64 value by at most
``e = 2^-23 (2 |t| + 1)``: log10f's documented 2 ulp (2 ulp(t) <= 2 * 2^-23 |t|) plus the roundings of its argument
(one for the tensor's own value; two more, the sum ``eps + w`` and the quotient, with a weight: each moves log10 by at
most 2^-24 / ln 10 = 0.43 * 2^-24, three of them 0.65 * 2^-23 < 2^-23).  In mode 0 the same bound holds with room.

Bin flips.  An entry's float32 position p32 = (t32 - lo) * scale32 differs from the fp64 position p = (t - lo) scale by
at most ``delta = scale (e + 2^-24 (|t| + |lo|)) + 3 * 2^-24 num_bins``: e moved t, the subtraction rounds once
(2^-24 (|t| + |lo|) bounds half an ulp of the difference), and the quotient num_bins / (hi - lo), its own denominator and
the product round once each (3 * 2^-24 relative, of a position that is at most num_bins).  Only an entry whose fp64
position lies within delta of an edge k can sit on the other side of k in float32, so cumulative counts at k may differ
by at most the number of such entries.
"""
import numpy as np

KEPT, DROPPED, NONFINITE = 0, 1, 2
FLT_MAX = float(np.finfo(np.float32).max)


def entries(values, rows=None, weight=None, eps=0.0, mode=0, min_value=0.0):
  """(cls int [E], t float64 [E]) of every gathered entry in row order; t is NaN where the entry is not kept.  The
  classes are decided in fp64 on the float32 inputs (an |x| above FLT_MAX counts as non-finite, as float32 sees it)."""
  v = np.asarray(values, np.float32)
  N, C = v.shape
  bad = 0
  if rows is not None:
    rows = np.asarray(rows, np.int64)
    inside = (rows >= 0) & (rows < N)
    bad = int((~inside).sum()) * C
    rows = rows[inside]
    v = v[rows]
  with np.errstate(all="ignore"):
    x = v.astype(np.float64)
    if weight is not None:
      w = np.asarray(weight, np.float32).astype(np.float64)
      w = w if rows is None else w[rows]
      x = x / (float(np.float32(eps)) + w)[:, None]
    x = x.reshape(-1)
    finite = np.isfinite(x) & (np.abs(x) <= FLT_MAX)
    cls = np.where(finite, KEPT, NONFINITE)
    mv = float(np.float32(min_value))
    t = x.copy()
    if mode == 1:
      cls = np.where(finite & ~(x > mv), DROPPED, cls)
      t = np.log10(np.where(cls == KEPT, x, 1.0))
    elif mode == 2:
      t = np.log10(np.maximum(np.where(finite, x, 1.0), mv))
    cls = np.where((cls == KEPT) & ~np.isfinite(t), NONFINITE, cls)
    t = np.where(cls == KEPT, t, np.nan)
  cls = np.concatenate([cls, np.full(bad, NONFINITE)])
  t = np.concatenate([t, np.full(bad, np.nan)])
  return cls, t


def entry_bound(t):
  return 2.0 ** -23 * (2.0 * np.abs(t) + 1.0)


def positions(t, lo, hi, num_bins):
  """fp64 positions of kept values t in a (lo, hi) given as float32 numbers, and each entry's flip band delta."""
  lo, hi = float(np.float32(lo)), float(np.float32(hi))
  scale = num_bins / (hi - lo)
  p = (t - lo) * scale
  delta = scale * (entry_bound(t) + 2.0 ** -24 * (np.abs(t) + abs(lo))) + 3.0 * 2.0 ** -24 * num_bins
  return p, delta


def compare_counts(counts, t, lo, hi, num_bins, trim, ends=True, label=""):
  """Asserts the cumulative rule on a float32 histogram's ``counts`` of the kept fp64 values ``t``.  ``ends``: the range
  was given (its two ends are edges like any other); False for a range the histogram found itself, whose ends hold its
  own minimum and maximum by construction and are not compared.  Returns (flagged share, largest cumulative
  difference).  Fails when more than 1 % of the kept entries lie inside a flip band."""
  counts = np.asarray(counts, np.int64)
  kept = t.size
  if float(np.float32(hi)) == float(np.float32(lo)):
    assert counts[0] == kept and counts[1:].sum() == 0, (label, counts.tolist(), kept)
    return 0.0, 0
  p, delta = positions(t, lo, hi, num_bins)
  edges = np.arange(0, num_bins + 1) if ends else np.arange(1, num_bins)
  first = np.clip(np.ceil(p - delta), 0, num_bins + 1).astype(np.int64)               # the edges k with |p - k| <= delta:
  last = np.clip(np.floor(p + delta), -1, num_bins).astype(np.int64)                  # first .. last (none when first > last)
  some = first <= last
  marks = np.bincount(first[some], minlength=num_bins + 2) - np.bincount(last[some] + 1, minlength=num_bins + 2)
  near = np.cumsum(marks)[:num_bins + 1]                                               # entries in the band of each edge
  flagged = int(some.sum()) if ends else int((np.maximum(first, 1) <= np.minimum(last, num_bins - 1)).sum())
  share = flagged / max(kept, 1)
  dev_cum = np.concatenate([[0], np.cumsum(counts)])
  sorted_p = np.sort(p)
  below = lambda k: int(np.searchsorted(sorted_p, k, side="left"))               # entries with p < k
  worst = 0
  for k in edges:
    if trim and ends:
      want, allowed = below(k) - below(0), near[k] + near[0]
    elif ends and k == num_bins:
      want, allowed = kept, 0                                                      # clamped: everything is binned
    elif ends and k == 0:
      want, allowed = 0, 0
    else:
      want, allowed = below(k), near[k]
    diff = abs(int(dev_cum[k]) - want)
    worst = max(worst, diff)
    assert diff <= allowed, (label, f"edge {k}: cumulative {int(dev_cum[k])} against {want}, {allowed} entries in the band")
  assert flagged <= 0.01 * kept, (label, f"{flagged} of {kept} kept entries lie inside a flip band")
  return share, worst


def sum_bounds(t):
  """(tolerance of sum t, tolerance of sum t^2) for kept fp64 values t: the float32 transform plus the fp64 summation."""
  n, e = t.size, entry_bound(t)
  return (float(e.sum() + n * 2.0 ** -52 * np.abs(t).sum()),
          float((2.0 * np.abs(t) * e).sum() + n * 2.0 ** -52 * (t * t).sum()))


def check_histogram(label, h, cls, kept, num_bins, given, trim):
  """Every assertion on a ``Histogram`` h of entries with the fp64 classes ``cls`` and kept values ``kept``: the tallies
  exact, minimum and maximum inside the per-entry bound, the cumulative rule, and -- ``given`` None, a range the histogram
  found itself -- nothing outside and the two sums inside ``sum_bounds``, or -- a given (lo, hi) -- the outside count
  under the flip rule at the two ends.  Each figure is printed before it is asserted."""
  counts, s = h.counts.cpu().numpy(), h.stats
  assert s["kept"] == kept.size and s["dropped"] == (cls == DROPPED).sum() and s["nonfinite"] == (cls == NONFINITE).sum(), (label, s)
  if kept.size == 0:
    assert not counts.any() and s["sum"] == 0 and s["outside"] == 0, (label, s)
    return
  lo_err, hi_err = abs(s["min"] - kept.min()), abs(s["max"] - kept.max())
  assert lo_err <= entry_bound(kept.min()) and hi_err <= entry_bound(kept.max()), (label, s)
  lo, hi = given or (s["min"], s["max"])
  share, worst = compare_counts(counts, kept, lo, hi, num_bins, trim, ends=given is not None, label=label)
  line = f"{label}: kept {kept.size}, flagged share {share:.5f}, largest cumulative difference {worst}, min/max error {lo_err:.2e} {hi_err:.2e}"
  if given is None:
    assert s["outside"] == 0 and counts.sum() == kept.size, (label, s)
    tol_sum, tol_sq = sum_bounds(kept)
    err_sum, err_sq = abs(s["sum"] - kept.sum()), abs(s["sum_squares"] - (kept * kept).sum())
    line += f", sum error {err_sum:.2e} (bound {tol_sum:.2e}), sum of squares error {err_sq:.2e} (bound {tol_sq:.2e})"
    print(line)
    assert err_sum <= tol_sum and err_sq <= tol_sq, line
  else:
    p, delta = positions(kept, lo, hi, num_bins)
    want = int(((p < 0) | (p >= num_bins)).sum())
    allowed = int((np.abs(p) <= delta).sum() + (np.abs(p - num_bins) <= delta).sum())
    print(line + f", outside {int(s['outside'])} against {want} ({allowed} entries in the end bands)")
    assert abs(s["outside"] - want) <= allowed, line
    assert counts.sum() == kept.size - (s["outside"] if trim else 0), line
