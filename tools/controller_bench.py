"""Times one noise step of the MCMC controller (splat_trainer_amd.controller.mcmc_noise, csrc/controller.hip) against the
torch form of the reference's mcmc_controller.py:93-100 written out below and made to hit the scene (the reference's own
lines perturb a copy), on the same GPU in the same process: the two are alternated repetition by repetition after a
warm-up, timed with device events, and reported as median and [min, max] (tools/timing.py's loop: 2 interleaved warm-up
rounds, 9 repetitions, one call per window, fixed order, one reused event pair, lower median).

    python tools/controller_bench.py [--quick] [--json out.json]

The torch form is eager: a bool-mask gather of every column of the point table (the 8 feature channels included, as
``points.tensors[enough_views]`` does), ``randn_like``, ``point_basis`` (exp, clamp, normalize, quaternion to matrix,
scale) -- the reference compiles that one function with torch.compile, here it is its eager ops --, a batched mat-vec and
the masked write back.  Two opacity mixes: every point nearly transparent (alpha_logit -4: every eligible row is
perturbed) and 5 % nearly transparent (the rest at +3: an opaque row costs the kernel its view count and its logit).
The kernel alone is timed through the C ABI, twenty launches between two events (1 warm-up launch, 5 windows, a fresh
event pair per window, every launch at the next step number).  It runs no reference code.

A native call counts as faster only when its slowest repetition beats torch's fastest (``clear``).
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import _lib  # noqa: E402
from timing import comparison_row, lower_median, repetitions, spread  # noqa: E402

MIN_VIEWS, THRESHOLD, NOISE, MARGIN, EPS = 5, 0.1, 1e-3, 16.0, 1e-4


def quat_to_rotmat(q):
  x, y, z, w = q.unbind(-1)
  return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                      2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                      2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def torch_noise(table, views):
  """mcmc_controller.py:93-100 in eager torch, with the write back the reference lacks."""
  enough = views > MIN_VIEWS
  opacity = torch.sigmoid(table["alpha_logit"]).squeeze(1)
  h = THRESHOLD / 2
  target = 1 - torch.sigmoid((opacity - h) * MARGIN / h)
  points = {k: v[enough] for k, v in table.items()}                        # every column, as tensors[enough_views]
  position = points["position"]
  noise = torch.randn_like(position) * (target[enough] * NOISE).unsqueeze(1)
  scale = torch.clamp_min(torch.exp(points["log_scaling"]), EPS)
  basis = quat_to_rotmat(F.normalize(points["rotation"], dim=1)) * scale.unsqueeze(-2)
  position += (basis @ noise.unsqueeze(-1)).squeeze(-1)
  table["position"][enough] = position


def kernel_alone(table, views, launches=20):
  lib, n, stream = _lib.load(), views.shape[0], _lib.current_stream_ptr()
  p = lambda t: t.data_ptr()
  steps = itertools.count()                                   # the warm-up launch is step 0, the timed ones follow on
  fn = lambda: _lib.check(lib.gsr_mcmc_noise(p(table["position"]), p(table["log_scaling"]), p(table["rotation"]),
                                             p(table["alpha_logit"]), p(views), n, MIN_VIEWS, THRESHOLD, MARGIN, NOISE,
                                             EPS, 0, next(steps), stream), "gsr_mcmc_noise")
  times = repetitions({"kernel": fn}, 5, warmup=1, calls=launches, fresh_events=True)["kernel"]
  return [round(t, 4) for t in (lower_median(times), *spread(times))]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--quick", action="store_true", help="small sizes (a functional run)")
  ap.add_argument("--json", default=None)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  g = torch.Generator().manual_seed(0)
  rows = []
  for n in ((20_000, 100_000) if args.quick else (500_000, 3_000_000)):
    for mix, share in (("all nearly transparent", 1.0), ("5 % nearly transparent", 0.05)):
      logit = torch.where(torch.rand(n, 1, generator=g) < share, torch.tensor(-4.0), torch.tensor(3.0))
      table = dict(position=torch.randn(n, 3, generator=g), log_scaling=torch.randn(n, 3, generator=g) - 4,
                   rotation=F.normalize(torch.randn(n, 4, generator=g), dim=1), alpha_logit=logit,
                   feature=torch.randn(n, 8, generator=g))
      table = {k: v.cuda() for k, v in table.items()}
      views = torch.randint(0, 40, (n,), generator=g).to(torch.int16).cuda()      # 85 % of the rows have enough views
      step = [0]

      def native():
        step[0] += 1
        sta.mcmc_noise(table["position"], table["log_scaling"], table["rotation"], table["alpha_logit"], views,
                       min_views=MIN_VIEWS, opacity_threshold=THRESHOLD, noise_level=NOISE, seed=0, step=step[0])

      ms = repetitions(dict(native=native, torch=lambda: torch_noise(table, views)), 9, warmup=2)
      r = comparison_row(f"noise step N={n} {mix}", ms["native"], ms["torch"])
      r["kernel_alone_ms"] = kernel_alone(table, views)
      live = int(((views > MIN_VIEWS) & (table["alpha_logit"].squeeze(1) < 0)).sum())
      r["perturbed_rows"] = live
      r["kernel_bytes"] = 6 * n + 52 * live                                        # 58 B per perturbed row, 6 per other
      r["kernel_GBps"] = round(r["kernel_bytes"] / (r["kernel_alone_ms"][0] * 1e-3) / 1e9, 1)
      assert torch.isfinite(table["position"]).all()
      rows.append(r)
      print(f"{r['case']:46s} native {r['native_ms']} {r['native_range']}  torch {r['torch_ms']} {r['torch_range']}  "
            f"x{r['speedup']}  clear {r['clear']}\n{'':46s} kernel alone {r['kernel_alone_ms'][0]} "
            f"[{r['kernel_alone_ms'][1]}, {r['kernel_alone_ms'][2]}] ms, {live} rows perturbed, "
            f"{r['kernel_bytes'] / 1e6:.1f} MB by the row count: {r['kernel_GBps']} GB/s", flush=True)
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
