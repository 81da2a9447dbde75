"""One fwd+bwd step of render_projected on c2 geometry (500k splats, 1920x1080) for C in {3, 4, 8, 16}, and for the
workaround the wide path replaces: a C = 3 render plus a C = 1 render of the same splats.

    python tools/wide_bench.py [--reps 20] [--warmup 5] [--n 500000]

Device-event timing of whole steps (projection excluded: it is shared by every variant), warm-up first, then the variants
run in alternating order `reps` times; prints the median milliseconds per step.  Per-kernel times come from a run of its
own under `rocprofv3 --kernel-trace --stats -- python tools/wide_bench.py --reps 5`.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import synthetic  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--n", type=int, default=500_000)
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  g, cam = synthetic.scene_a(args.n, 1920, 1080, sh_degree=0, seed=0)
  cfg = sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True)
  cam = cam.to("cuda")
  gd = sta.Gaussians3D(*(t.cuda() for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
  with torch.no_grad():
    g2d, depth, idx = sta.project_to_image(gd, cam, cfg)
  M = idx.shape[0]
  torch.manual_seed(0)
  feats = {c: torch.rand(M, c, device="cuda") for c in (1, 3, 4, 8, 16)}
  grads = {c: torch.rand(1080, 1920, c, device="cuda") for c in (1, 3, 4, 8, 16)}
  g2 = g2d.detach().clone().requires_grad_(True)

  def step(channels):
    for c in channels:
      f = feats[c].requires_grad_(True)
      r = sta.render_projected(idx, g2, f, depth, cam, cfg)
      r.image.backward(grads[c])
      f.grad = None
    g2.grad = None

  variants = {"C=3": (3,), "C=4": (4,), "C=8": (8,), "C=16": (16,), "C=3 + C=1": (3, 1)}
  times = {k: [] for k in variants}
  for _ in range(args.warmup):
    for v in variants.values():
      step(v)
  torch.cuda.synchronize()
  for rep in range(args.reps):
    order = list(variants) if rep % 2 == 0 else list(reversed(variants))
    for k in order:
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      step(variants[k])
      b.record()
      b.synchronize()
      times[k].append(a.elapsed_time(b))
  med = {k: statistics.median(v) for k, v in times.items()}
  print(f"c2 geometry: M={M} visible splats, 1920x1080; median ms per fwd+bwd step over {args.reps} alternating runs")
  for k, v in med.items():
    print(f"  {k:10s} {v:8.3f} ms   (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
  print(json.dumps({"M": M, "median_ms": med}))


if __name__ == "__main__":
  main()
