"""tools/timing.py on the device: both clocks give one positive finite time per window, and the loop makes exactly the
calls it is asked for (counted by the device itself).  Nothing is asserted about magnitudes."""
import importlib.util
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("timing", os.path.join(ROOT, "tools", "timing.py"))
timing = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(timing)


@pytest.mark.gpu
def test_loop_on_the_device():
  for clock in (timing.DeviceEvents(), timing.HostClock()):
    x = torch.zeros(1024, device="cuda")
    forms = (("first", lambda: x.add_(1)), ("second", lambda k: x.add_(1)))
    times = timing.repetitions(forms, 3, 1, calls=2, warmup_form="interleaved", clock=clock)
    assert list(times) == ["first", "second"]
    for ts in times.values():
      assert len(ts) == 3 and all(math.isfinite(t) and t > 0 for t in ts)
    assert torch.equal(x, torch.full_like(x, 2 * (1 + 3 * 2)))
