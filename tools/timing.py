"""The one timing loop of the benchmark tools under tools/, its two clocks and the summaries the tools report.

    from timing import repetitions, lower_median, spread            # a tool next to this file

``repetitions`` runs named forms (callables) for a warm-up and then ``reps`` repetitions, each form in a timed window of
its own, and returns every window's milliseconds per call in the order measured.  What a tool reports from those lists --
which median, which unit, which rounding -- is the tool's business and is fixed by the JSON it has filed; the helpers
below are the statistics the tools share.  A tool states its parameters (warm-up count and form, repetitions, calls per
window, order, clock, fresh or reused events, statistic) in its own docstring.

A measurement path that finds no GPU fails: both clocks raise at construction without one.  Nothing here touches the
device when the module is imported, and nothing depends on the package.
"""
from __future__ import annotations

import inspect
import statistics
import time

import torch


def _need_gpu(who: str):
  if not torch.cuda.is_available():
    raise RuntimeError(f"{who} needs a GPU: a timing without one is no measurement, and there is no fallback")


class DeviceEvents:
  """A window between two ``torch.cuda.Event`` records on the current stream; ``stop`` waits on the end event.
  ``fresh=False`` (the default) creates one pair at the first window and records into it again every window;
  ``fresh=True`` creates a new pair per window.  Both measure the same interval; each tool keeps the one it had."""

  def __init__(self, fresh: bool = False):
    _need_gpu("DeviceEvents")
    self._fresh, self._pair = fresh, None

  def synchronize(self):
    torch.cuda.synchronize()

  def start(self):
    if self._fresh or self._pair is None:
      self._pair = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    self._pair[0].record()

  def stop(self) -> float:
    a, b = self._pair
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class HostClock:
  """``time.perf_counter`` around a window that ends in ``torch.cuda.synchronize()``: host work and launches included."""

  def __init__(self):
    _need_gpu("HostClock")

  def synchronize(self):
    torch.cuda.synchronize()

  def start(self):
    self._t0 = time.perf_counter()

  def stop(self) -> float:
    torch.cuda.synchronize()
    return (time.perf_counter() - self._t0) * 1e3


def _caller(fn):
  """``fn`` as a function of the call index: it is handed ``k`` when it has a required positional parameter (a
  parameter with a default, such as a loop variable bound with ``lambda n=n: ...``, does not count) and nothing
  otherwise.  Decided here, once, from the signature."""
  positional = (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)
  takes_k = any(p.kind in positional and p.default is p.empty for p in inspect.signature(fn).parameters.values())
  return fn if takes_k else (lambda k: fn())


def repetitions(forms, reps, warmup, calls=1, order="fixed", clock=None, fresh_events=False, warmup_form="interleaved"):
  """``{name: [milliseconds per call of each window, in the order measured]}``; neither sorted nor summarised.

  forms         an ordered mapping name -> fn or a sequence of (name, fn); fn takes the call index k or nothing
  reps          timed repetitions; in each, every form gets one window
  warmup        untimed rounds before the first window; fn(k) is handed the round, 0..warmup-1
  warmup_form   "interleaved": one call of every form per round; "per_form": all rounds of one form, then the next
  calls         calls of one form inside one window (k = 0..calls-1); the window's time is divided by it
  order         "fixed", or "mirrored": the forms reversed on odd repetitions
  clock         DeviceEvents by default; an object with synchronize(), start() and stop() -> ms otherwise
  fresh_events  the default clock's ``fresh``: False records into one reused event pair, True creates a pair per window

  One ``clock.synchronize()`` follows the warm-up; every window ends in the clock's own wait."""
  if order not in ("fixed", "mirrored") or warmup_form not in ("interleaved", "per_form"):
    raise ValueError(f"order={order!r}, warmup_form={warmup_form!r}")
  forms = [(name, _caller(fn)) for name, fn in (forms.items() if hasattr(forms, "items") else forms)]
  clock = DeviceEvents(fresh=fresh_events) if clock is None else clock
  if warmup_form == "interleaved":
    for k in range(warmup):
      for _, call in forms:
        call(k)
  else:
    for _, call in forms:
      for k in range(warmup):
        call(k)
  clock.synchronize()
  times = {name: [] for name, _ in forms}
  for rep in range(reps):
    for name, call in (forms[::-1] if order == "mirrored" and rep % 2 else forms):
      clock.start()
      for k in range(calls):
        call(k)
      times[name].append(clock.stop() / calls)
  return times


def single_window(fn, reps, warmup, clock=None) -> float:
  """Mean milliseconds per call of ``reps`` calls in one window, after ``warmup`` calls and a synchronise."""
  return repetitions([("fn", fn)], 1, warmup, calls=reps, clock=clock)["fn"][0]


def lower_median(ts):
  """``sorted(ts)[len(ts) // 2]``: the upper of the two middles on an even count."""
  return sorted(ts)[len(ts) // 2]


def mid_median(ts):
  """``statistics.median``: the mean of the two middles on an even count."""
  return statistics.median(ts)


def spread(ts):
  return [min(ts), max(ts)]


def clear(a, b) -> bool:
  """``a`` counts as faster than ``b`` only when its slowest repetition beats the other's fastest."""
  return max(a) < min(b)


def comparison_row(name, native, reference, digits=(4, 3)):
  """The row of a native form beside its torch form: lower median and [min, max] of each in ms, rounded to
  ``digits`` (native, torch), the ratio of the medians to one digit and the ``clear`` rule."""
  dn, dr = digits
  n, r = lower_median(native), lower_median(reference)
  return dict(case=name, native_ms=round(n, dn), native_range=[round(t, dn) for t in spread(native)],
              torch_ms=round(r, dr), torch_range=[round(t, dr) for t in spread(reference)],
              speedup=round(r / n, 1), clear=clear(native, reference))
