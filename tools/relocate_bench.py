"""Times one relocation round of the MCMC controller (splat_trainer_amd.controller.relocate_points, csrc/relocate.hip)
against its torch form written out below, on the same GPU in the same process: the two are alternated repetition by
repetition after a warm-up, timed with device events, and reported as median and [min, max] (tools/timing.py's loop:
2 interleaved warm-up rounds, 9 repetitions, one call per window, fixed order, one reused event pair, lower median).
It runs no reference code.

    python tools/relocate_bench.py [--quick] [--json out.json]

The point table is an ``MLPScene``'s: position, log_scaling, rotation, alpha_logit, 8 feature channels and ``visible``,
with Adam state for the five parameter groups; 5 % of the rows are dead.  The torch form: ``torch.multinomial`` over the
live rows' opacities, ``bincount``, the correction in fp64 on the drawn sources (the 51-term sum as a masked loop),
indexed copies of every column and indexed zero-fills of the optimizer state.  Both forms end with the state zeroing of
the dead rows and make one host read.

The second part records what one draw does at N = 2^24 + 1 rows, where ``torch.multinomial`` refuses the category count.

Written down before the first run.  Native: some fifteen launches of which none moves more than 12 MB at 3 M rows, and
one host read -- launch-bound, 0.2 to 0.5 ms at both sizes.  Torch: the multinomial's cumsum and search, a nonzero (a
second host read), some 51 x 6 element-wise fp64 launches over the sources and two indexed launches per column -- 3 to
8 ms at both sizes, launch-bound too.  So x10, and no change with N until the rows' traffic passes the launches.

A native round counts as faster only when its slowest repetition beats torch's fastest (``clear``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import controller as ctl  # noqa: E402
from splat_trainer_amd.controller_math import PointState  # noqa: E402
from splat_trainer_amd.optim import ParameterClass  # noqa: E402
from timing import comparison_row, repetitions  # noqa: E402

PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))
O_FLOOR, MAX_COPIES = 0.1, 51


def make_points(n, g):
  logit = torch.where(torch.rand(n, 1, generator=g) < 0.05, torch.tensor(-4.0), torch.randn(n, 1, generator=g) * 2 + 1)
  tensors = dict(position=torch.randn(n, 3, generator=g), log_scaling=torch.randn(n, 3, generator=g) - 4,
                 rotation=torch.randn(n, 4, generator=g), alpha_logit=logit, feature=torch.randn(n, 8, generator=g),
                 visible=torch.zeros(n))
  points = ParameterClass({k: v.cuda() for k, v in tensors.items()}, PARAMETERS)
  return points, PointState.new_zeros(n, "cuda"), (logit.squeeze(1) < -3.0).cuda()


def torch_correction(alpha_logit, log_scaling, rows, copies):
  """Eq. 9 on the rows ``rows`` with ``copies`` copies each, fp64, in place."""
  n = torch.clamp(copies + 1, max=MAX_COPIES).to(torch.float64)
  o = torch.sigmoid(alpha_logit[rows, 0].double())
  op = -torch.expm1(torch.log1p(-o) / n)
  D, binom, power = torch.zeros_like(o), n.clone(), op.clone()
  for k in range(MAX_COPIES):
    term = torch.where(n > k, binom * power / (k + 1) ** 0.5, torch.zeros_like(o))
    D = D - term if k & 1 else D + term
    binom = binom * (n - k - 1) / (k + 2)
    power = power * op
  p = torch.clamp(op, O_FLOOR, 1 - 2.0 ** -24)
  alpha_logit[rows, 0] = torch.log(p / (1 - p)).float()
  log_scaling[rows] = (log_scaling[rows].double() + torch.log(o / D)[:, None]).float()


@torch.no_grad()
def torch_round(points, state, dead):
  dead_rows = dead.nonzero().squeeze(1)                                        # (host read: the dead count)
  live_rows = (~dead).nonzero().squeeze(1)
  opacity = torch.sigmoid(points.alpha_logit.detach()[live_rows, 0])
  sources = live_rows[torch.multinomial(opacity, dead_rows.shape[0], replacement=True)]
  counts = torch.bincount(sources, minlength=dead.shape[0])
  drawn = counts.nonzero().squeeze(1)                                          # (a second host read)
  torch_correction(points.alpha_logit.detach(), points.log_scaling.detach(), drawn, counts[drawn])
  for t in points.tensors.values():
    t.detach()[dead_rows] = t.detach()[sources]
  for t in ctl._optimizer_columns(points):
    t[dead_rows] = 0
    t[sources] = 0
  for v in vars(state).values():
    v.masked_fill_(dead, 0)


def one_draw(n):
  """What one draw over n equal weights does, natively and with torch.multinomial."""
  out = {}
  weights = torch.ones(n, dtype=torch.int32, device="cuda")
  sources, counts, total = sta.weighted_draws(weights, 1, 3, 4, 1)
  out["native"] = dict(source=int(sources.item()), total=int(total.item()), counted=int(counts.sum().item()))
  try:
    out["torch"] = dict(source=int(torch.multinomial(torch.ones(n, device="cuda"), 1).item()))
  except RuntimeError as e:
    out["torch"] = dict(raised=str(e).splitlines()[0][:160])
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--quick", action="store_true", help="small sizes (a functional run)")
  ap.add_argument("--json", default=None)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  g = torch.Generator().manual_seed(0)
  rows = []
  for n in ((20_000, 100_000) if args.quick else (500_000, 3_000_000)):
    points, state, dead = make_points(n, g)
    twin = ParameterClass({k: t.detach().clone() for k, t in points.tensors.items()}, PARAMETERS)
    twin_state = PointState.new_zeros(n, "cuda")
    step = [0]

    def native():
      step[0] += 1
      sta.relocate_points(points, state, dead, O_FLOOR, 0, step[0])

    ms = repetitions(dict(native=native, torch=lambda: torch_round(twin, twin_state, dead)), 9, warmup=2)
    r = comparison_row(f"relocation round N={n}, {int(dead.sum())} dead", ms["native"], ms["torch"])
    for k, t in points.tensors.items():
      assert torch.isfinite(t).all() and torch.isfinite(twin.tensors[k]).all(), k
    rows.append(r)
    print(f"{r['case']:46s} native {r['native_ms']} {r['native_range']}  torch {r['torch_ms']} {r['torch_range']}  "
          f"x{r['speedup']}  clear {r['clear']}", flush=True)
  for n in ((2 ** 16 + 1,) if args.quick else (2 ** 24, 2 ** 24 + 1)):
    r = dict(case=f"one draw over N={n} equal weights", **one_draw(n))
    rows.append(r)
    print(r, flush=True)
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
