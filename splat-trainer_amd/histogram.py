"""The reference's ``Histogram`` (``splat_trainer.logger.histogram``) over the native histogram kernels
(csrc/histogram.hip; the contract is in include/gsplat_hip.h, the entry and bin rules in csrc/gsr_histogram.h).

``tensor_histogram`` does in one call what the reference's detailed logs do in a dozen torch launches and two host
waits per histogram: gather rows (``rows``), divide by a per-row weight (``weight``, ``eps``), take ``log10`` with the
small values dropped or clamped (``log10``, ``min_value``), find the range (``range=None``) and bin.  A device call
waits for nothing: the ``Histogram`` it returns holds device tensors and reads them the first time a number is asked
for (one copy for counts and statistics together).  CPU tensors take a numpy path with the same rule.

Deliberate deviations from the reference's class: ``sum_squares`` is the sum of squares (the reference stores the
2-norm, so its ``std`` is wrong); a value equal to the range's upper end is counted in the last bin (the reference
drops it); ``__truediv__``, which the reference cannot run, is left out.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._args import f32

MAX_BINS = _lib.CONSTANTS["GSR_HISTOGRAM_MAX_BINS"]
MODES = {None: 0, "drop": 1, "clamp": 2}
STATS = ("kept", "sum", "sum_squares", "min", "max", "dropped", "nonfinite", "outside")
_workspaces = {}


def _check_bins(num_bins) -> int:
  num_bins = int(num_bins)
  if not 1 <= num_bins <= MAX_BINS:
    raise ValueError(f"num_bins must be in 1..{MAX_BINS}, got {num_bins}")
  return num_bins


def _check_range(range) -> Optional[Tuple[float, float]]:
  if range is None:
    return None
  if len(range) != 2:
    raise ValueError(f"range must be None or (lower, upper), got {range!r}")
  lo, hi = float(np.float32(range[0])), float(np.float32(range[1]))
  if not (math.isfinite(lo) and math.isfinite(hi) and hi >= lo):
    raise ValueError(f"range must be finite in float32 with upper >= lower, got {range!r}")
  return lo, hi


def _rows_2d(values: torch.Tensor) -> torch.Tensor:
  """``values`` as float32 (N, C) contiguous: integer and half inputs are converted, 0-d and 1-d become one column."""
  v = f32(values)
  if v.dim() < 2:
    return v.reshape(-1, 1)
  return v.reshape(v.shape[0], -1) if v.dim() > 2 else v


def _host_histogram(v: np.ndarray, rows, weight, eps: float, mode: int, min_value: float, range, num_bins: int,
                    trim: bool):
  """The contract of gsr_histogram in numpy float32 (sums in float64): (counts int64 [num_bins], stats float64 [8])."""
  N = v.shape[0]
  bad_rows = 0
  if rows is not None:
    inside = (rows >= 0) & (rows < N)
    bad_rows = int((~inside).sum()) * v.shape[1]
    rows = rows[inside]
    v = v[rows]
  with np.errstate(all="ignore"):
    x = v if weight is None else v / (np.float32(eps) + (weight if rows is None else weight[rows])[:, None])
    x = x.astype(np.float32, copy=False).reshape(-1)
    finite = np.isfinite(x)
    passed = finite & (x > np.float32(min_value)) if mode == 1 else finite
    t = x[passed]
    if mode == 1:
      t = np.log10(t)
    elif mode == 2:
      t = np.log10(np.maximum(t, np.float32(min_value)))
    t = t.astype(np.float32, copy=False)
    t_finite = np.isfinite(t)
    t = t[t_finite]
    stats = np.zeros(8, np.float64)
    stats[0] = t.size
    stats[5] = int(finite.sum()) - int(passed.sum())
    stats[6] = int((~finite).sum()) + int((~t_finite).sum()) + bad_rows
    counts = np.zeros(num_bins, np.int64)
    if t.size == 0:
      return counts, stats
    stats[3], stats[4] = t.min(), t.max()
    lo, hi = (np.float32(stats[3]), np.float32(stats[4])) if range is None else map(np.float32, range)
    if hi == lo:
      b = np.zeros(t.shape, np.float32)
    else:
      b = np.floor((t - lo) * (np.float32(num_bins) / (hi - lo)))
      b = np.where(t == hi, np.float32(num_bins - 1), b)
    inside = (b >= 0) & (b < num_bins)
    stats[7] = int((~inside).sum())
    if trim:
      t, b = t[inside], b[inside]
    else:
      b = np.where(inside, b, np.where(b < 0, np.float32(0), np.float32(num_bins - 1)))
    counts += np.bincount(b.astype(np.int64), minlength=num_bins)
    t64 = t.astype(np.float64)
    stats[1], stats[2] = t64.sum(), (t64 * t64).sum()
  return counts, stats


def _workspace(device: torch.device, stream: int) -> torch.Tensor:
  key = (device.index, stream)
  if key not in _workspaces:
    _workspaces[key] = _lib.workspace(_lib.load().gsr_histogram_workspace_bytes(), device)
  return _workspaces[key]


class Histogram:
  """logger/histogram.py:7-110.  ``Histogram(values, range=(0, 1), num_bins=10, trim=True)`` bins ``values`` as the
  reference does; ``tensor_histogram`` is the full form.  ``counts`` is a tensor on the values' device; ``range``,
  ``sum``, ``sum_squares``, ``mean``, ``std`` and ``stats`` are host numbers, read from the device when first asked for."""

  def __init__(self, values: torch.Tensor, range=(0, 1), num_bins: int = 10, trim: bool = True):
    other = tensor_histogram(values, num_bins=num_bins, range=range, trim=trim)
    self._buffer, self._range, self._host = other._buffer, other._range, other._host

  @staticmethod
  def _of(buffer: torch.Tensor, range) -> "Histogram":
    """``buffer``: int64 [num_bins + 8], the counts and behind them the bits of the eight float64 statistics."""
    h = object.__new__(Histogram)
    h._buffer, h._range, h._host = buffer, range, None
    return h

  @staticmethod
  def empty(range, num_bins: int, device=None) -> "Histogram":
    return Histogram._of(torch.zeros(_check_bins(num_bins) + 8, dtype=torch.int64, device=device), _check_range(range))

  def _read(self):
    if self._host is None:
      host = self._buffer.cpu()                                          # the one wait
      self._host = (host[:-8].numpy(), host[-8:].view(torch.float64).numpy())
    return self._host

  @property
  def counts(self) -> torch.Tensor:
    return self._buffer[:-8]

  @property
  def num_bins(self) -> int:
    return self._buffer.shape[0] - 8

  @property
  def device(self):
    return self._buffer.device

  @property
  def stats(self) -> dict:
    """kept, sum, sum_squares, min, max, dropped, nonfinite, outside (STATS) as host floats."""
    return dict(zip(STATS, map(float, self._read()[1])))

  @property
  def range(self) -> Tuple[float, float]:
    if self._range is None:                                              # found on the device: the kept minimum and maximum
      s = self._read()[1]
      self._range = (float(s[3]), float(s[4]))
    return self._range

  @property
  def sum(self) -> float:
    return float(self._read()[1][1])

  @property
  def sum_squares(self) -> float:
    return float(self._read()[1][2])

  @property
  def total(self) -> int:
    return int(self._read()[0].sum())

  def __repr__(self):
    return self._read()[0].tolist().__repr__()

  @property
  def bins(self) -> torch.Tensor:
    lower, upper = self.range
    d = (upper - lower) / self.num_bins
    return torch.tensor([lower + i * d for i in np.arange(self.num_bins + 1)])

  @property
  def bin_width(self) -> float:
    lower, upper = self.range
    return (upper - lower) / self.num_bins

  @property
  def bin_ranges(self) -> torch.Tensor:
    bins = self.bins
    return torch.stack([bins[:-1], bins[1:]], dim=1)

  def __add__(self, other: "Histogram") -> "Histogram":
    assert isinstance(other, Histogram)
    assert other.num_bins == self.num_bins and other.range == self.range, "mismatched histogram sizes"
    a, b = self._buffer, other._buffer.to(self._buffer.device)
    total = torch.empty_like(a)
    total[:-8] = a[:-8] + b[:-8]
    sa, sb = a[-8:].view(torch.float64), b[-8:].view(torch.float64)
    s = sa + sb
    s[3] = torch.where(sa[0] == 0, sb[3], torch.where(sb[0] == 0, sa[3], torch.minimum(sa[3], sb[3])))
    s[4] = torch.where(sa[0] == 0, sb[4], torch.where(sb[0] == 0, sa[4], torch.maximum(sa[4], sb[4])))
    total[-8:] = s.view(torch.int64)
    return Histogram._of(total, self.range)

  def append(self, values: torch.Tensor, trim: bool = True) -> "Histogram":
    return self + tensor_histogram(values, num_bins=self.num_bins, range=self.range, trim=trim)

  @property
  def std(self) -> float:
    n = self.total
    if n > 1:
      sum_squares = self.sum_squares - (self.sum * self.sum / n)
      return math.sqrt(max(0.0, sum_squares / (n - 1)))
    return 0

  @property
  def mean(self) -> float:
    n = self.total
    return self.sum / n if n > 0 else 0


def tensor_histogram(values: torch.Tensor, num_bins: int = 64, range=None, rows: Optional[torch.Tensor] = None,
                     weight: Optional[torch.Tensor] = None, eps: float = 0., log10: Optional[str] = None,
                     min_value: float = 0., trim: bool = True) -> Histogram:
  """The histogram of the entries of ``values`` (any shape; rows are its first dimension).

  ``rows``: int64 indices of the rows to take (repeats and any order allowed), None for all.  ``weight``: one value per
  row of ``values``; an entry ``v`` of row ``r`` becomes ``v / (eps + weight[r])``.  ``log10``: None bins the entries as
  they are, ``"drop"`` bins ``log10(v)`` of the entries ``v > min_value`` and drops the others (the reference's
  ``hist_log_nonzero`` / ``log_scale_histogram``), ``"clamp"`` bins ``log10(max(v, min_value))`` (its
  ``point_state.log_histograms``).  ``range``: (lower, upper), or None for the minimum and maximum of what is kept.
  Non-finite entries are never binned; ``Histogram.stats`` counts them.  With ``trim`` an entry outside the range is
  left out, without it it goes to the nearest bin.  On a device tensor this is the native kernel family and waits for
  nothing; on a CPU tensor it is numpy with the same rule."""
  if log10 not in MODES:
    raise ValueError(f"log10 must be None, 'drop' or 'clamp', got {log10!r}")
  num_bins, fixed, mode = _check_bins(num_bins), _check_range(range), MODES[log10]
  v = _rows_2d(values)
  N, C = v.shape
  if rows is not None:
    if rows.dtype is not torch.int64 or rows.dim() != 1:
      raise ValueError(f"rows must be a 1-d int64 tensor, got {rows.dtype} {tuple(rows.shape)}")
    rows = rows.to(v.device).contiguous()
  if weight is not None:
    if weight.numel() != N:
      raise ValueError(f"weight must hold one value per row of values ({N}), got {tuple(weight.shape)}")
    weight = weight.detach().to(device=v.device, dtype=torch.float32).reshape(N).contiguous()
  if N == 0 or C == 0 or (rows is not None and rows.shape[0] == 0):          # nothing to launch
    return Histogram.empty(fixed or (0., 0.), num_bins, v.device)
  if not v.is_cuda:
    counts, stats = _host_histogram(v.numpy(), None if rows is None else rows.numpy(),
                                    None if weight is None else weight.numpy(), float(eps), mode, float(min_value), fixed,
                                    num_bins, bool(trim))
    buffer = torch.from_numpy(np.concatenate([counts, stats.view(np.int64)]))
    return Histogram._of(buffer, fixed)
  with _lib.on_device(v.device) as stream:
    workspace = _workspace(v.device, stream)
    buffer = torch.empty(num_bins + 8, dtype=torch.int64, device=v.device)
    lo, hi = fixed or (0., 0.)
    _lib.call("gsr_histogram", _lib.ptr(v), N, C, None if rows is None else rows.data_ptr(),
              0 if rows is None else rows.shape[0], _lib.ptr(weight), float(eps), mode, float(min_value), lo, hi, num_bins,
              int(fixed is None), int(bool(trim)), buffer.data_ptr(), buffer.data_ptr() + 8 * num_bins,
              workspace.data_ptr(), workspace.numel(), stream)
  return Histogram._of(buffer, fixed)
