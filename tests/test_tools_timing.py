"""tools/timing.py, the one timing loop of the benchmark tools, on the CPU: the exact sequence of calls, synchronises
and windows of every warm-up form, order and call count under a scripted clock, the summaries, the row of a comparison
against the row tools/visibility_bench.py gave before the loop moved, and that no converted tool times by hand."""
import ast
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("timing", os.path.join(ROOT, "tools", "timing.py"))
timing = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(timing)


class ScriptedClock:
  """Writes its own calls into the trace the forms write into; window i lasts ``script[i]`` milliseconds."""

  def __init__(self, trace, script):
    self.trace, self.script = trace, list(script)

  def synchronize(self):
    self.trace.append("sync")

  def start(self):
    self.trace.append("start")

  def stop(self):
    self.trace.append("stop")
    return self.script.pop(0)


def stubs(trace):
  """Form a takes the call index, form b takes nothing (its trace entry holds the arguments it got: none)."""
  def a(k):
    trace.append(("a", k))

  def b(*args):
    trace.append(("b", args))

  return (("a", a), ("b", b))


# 2 forms, reps=3, warmup=2: the warm-up calls of each form and the form of each of the six windows, written out.
WARMUP = {"interleaved": [("a", 0), ("b", ()), ("a", 1), ("b", ())],
          "per_form": [("a", 0), ("a", 1), ("b", ()), ("b", ())]}
WINDOWS = {"fixed": ["a", "b", "a", "b", "a", "b"],
           "mirrored": ["a", "b", "b", "a", "a", "b"]}
SCRIPT = [6.0, 9.0, 3.0, 12.0, 1.5, 0.75]


@pytest.mark.parametrize("calls", [1, 3])
@pytest.mark.parametrize("order", ["fixed", "mirrored"])
@pytest.mark.parametrize("warmup_form", ["interleaved", "per_form"])
def test_call_trace_and_times(warmup_form, order, calls):
  trace = []
  times = timing.repetitions(stubs(trace), 3, 2, calls=calls, order=order, warmup_form=warmup_form,
                             clock=ScriptedClock(trace, SCRIPT))
  expected = WARMUP[warmup_form] + ["sync"]
  for name in WINDOWS[order]:
    expected += ["start"] + [("a", k) if name == "a" else ("b", ()) for k in range(calls)] + ["stop"]
  assert trace == expected
  assert trace.count("sync") == 1 and trace.index("sync") < trace.index("start")
  per_form = {"a": [], "b": []}
  for name, ms in zip(WINDOWS[order], SCRIPT):
    per_form[name].append(ms / calls)
  assert times == per_form                                   # measured order, unsorted: a's list is not monotonic
  assert list(times) == ["a", "b"]


def test_one_trace_spelled_out():
  """2 forms, reps=3, warmup=2 interleaved, calls=2, mirrored: every entry."""
  trace = []
  times = timing.repetitions(stubs(trace), 3, 2, calls=2, order="mirrored", clock=ScriptedClock(trace, SCRIPT))
  assert trace == [("a", 0), ("b", ()), ("a", 1), ("b", ()), "sync",
                   "start", ("a", 0), ("a", 1), "stop", "start", ("b", ()), ("b", ()), "stop",
                   "start", ("b", ()), ("b", ()), "stop", "start", ("a", 0), ("a", 1), "stop",
                   "start", ("a", 0), ("a", 1), "stop", "start", ("b", ()), ("b", ()), "stop"]
  assert times == {"a": [3.0, 6.0, 0.75], "b": [4.5, 1.5, 0.375]}


def test_forms_as_a_mapping_and_no_warmup():
  trace = []
  forms = dict(stubs(trace))
  times = timing.repetitions(forms, 1, 0, clock=ScriptedClock(trace, [2.0, 4.0]))
  assert trace == ["sync", "start", ("a", 0), "stop", "start", ("b", ()), "stop"]
  assert times == {"a": [2.0], "b": [4.0]}


def test_a_parameter_with_a_default_is_not_the_call_index():
  seen = []
  timing.repetitions([("f", lambda n=7: seen.append(n))], 2, 1, clock=ScriptedClock([], [1.0, 1.0]))
  assert seen == [7, 7, 7]


def test_unknown_options_raise():
  with pytest.raises(ValueError):
    timing.repetitions(stubs([]), 1, 0, order="random", clock=ScriptedClock([], [1.0]))
  with pytest.raises(ValueError):
    timing.repetitions(stubs([]), 1, 0, warmup_form="none", clock=ScriptedClock([], [1.0]))


def test_single_window():
  """optim_bench's form: warm-up calls, one synchronise, all the calls in one window, the window divided by them."""
  trace = []
  ms = timing.single_window(lambda: trace.append("f"), 4, 3, clock=ScriptedClock(trace, [10.0]))
  assert trace == ["f", "f", "f", "sync", "start", "f", "f", "f", "f", "stop"]
  assert ms == 2.5


def test_summaries():
  assert timing.lower_median([4, 1, 3, 2]) == 3 and timing.mid_median([4, 1, 3, 2]) == 2.5
  assert timing.lower_median([5, 1, 3]) == timing.mid_median([5, 1, 3]) == 3
  assert timing.lower_median([2]) == timing.mid_median([2]) == 2
  assert timing.spread([3, 1, 2]) == [1, 3]
  assert timing.clear([1, 2], [3, 4]) is True
  assert timing.clear([1, 3], [3, 4]) is False               # equality is not clear
  assert timing.clear([1, 3.5], [3, 4]) is False
  assert timing.clear([2, 1], [4, 3]) is True                # unsorted lists, as the loop returns them


def test_comparison_row_is_the_parent_row():
  """The expected dictionaries are what visibility_bench.row returned for these lists (sorted, as its loop handed them
  over) before the loop moved to tools/timing.py; here the lists come unsorted, as the loop returns them now."""
  row = timing.comparison_row("a case", [0.12345, 0.11111, 0.13579, 0.12001], [1.23456, 1.5, 1.11119, 1.3])
  assert row == {"case": "a case", "native_ms": 0.1235, "native_range": [0.1111, 0.1358], "torch_ms": 1.3,
                 "torch_range": [1.111, 1.5], "speedup": 10.5, "clear": True}
  assert list(row) == ["case", "native_ms", "native_range", "torch_ms", "torch_range", "speedup", "clear"]
  row = timing.comparison_row("overlap", [0.5, 1.11119, 0.25], [1.23456, 1.11119, 1.3])
  assert row == {"case": "overlap", "native_ms": 0.5, "native_range": [0.25, 1.1112], "torch_ms": 1.235,
                 "torch_range": [1.111, 1.3], "speedup": 2.5, "clear": False}


@pytest.mark.parametrize("clock", ["DeviceEvents", "HostClock"])
def test_default_clocks_need_a_gpu(clock):
  if torch.cuda.is_available():
    pytest.skip("a device is present: the clocks construct")
  with pytest.raises(RuntimeError, match="needs a GPU"):
    getattr(timing, clock)()
  with pytest.raises(RuntimeError, match="needs a GPU"):
    timing.repetitions(stubs([]), 1, 0)                      # no injected clock: the default one, which refuses


CONVERTED = ["visibility_bench", "filter3d_bench", "controller_bench", "relocate_bench", "undistort_bench", "dataset_bench",
             "camera_table_bench", "neighbours_bench", "color_model_bench", "mlp_scene_bench", "bilagrid_bench",
             "sh_fit_bench", "eval_bench", "optim_bench", "camera_grad_bench", "wide_bench", "large_splat_bench"]
# Clock calls a converted tool may keep, with the reason: host-side phases that are no device timing.
KEPT = {"dataset_bench": {"perf_counter": "bench_load times JPEG decoding and load_images() on the host, seconds per phase"}}


def _dotted(node):
  parts = []
  while isinstance(node, ast.Attribute):
    parts.append(node.attr)
    node = node.value
  return ".".join(reversed(parts + [node.id])) if isinstance(node, ast.Name) else ""


@pytest.mark.parametrize("tool", CONVERTED)
def test_converted_tool_has_no_loop_of_its_own(tool):
  with open(os.path.join(ROOT, "tools", tool + ".py")) as f:
    tree = ast.parse(f.read())
  called = {_dotted(n.func) for n in ast.walk(tree) if isinstance(n, ast.Call)}
  imports = [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
  kept = KEPT.get(tool, {})
  assert not any(c.split(".")[-1] == "Event" for c in called), "records device events itself"
  if "perf_counter" not in kept:
    assert not any(c.split(".")[-1] == "perf_counter" for c in called), "reads the host clock itself"
  assert not any(a.name == "alternated" for n in imports for a in n.names), "takes a sibling tool's loop"
  assert any(n.module == "timing" for n in imports), "does not use tools/timing.py"
