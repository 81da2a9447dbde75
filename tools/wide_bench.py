"""One fwd+bwd step of render_projected on c2 geometry (500k splats, 1920x1080) for C in {3, 4, 8, 16}, and for the
workaround the wide path replaces: a C = 3 render plus a C = 1 render of the same splats.

    python tools/wide_bench.py [--reps 20] [--warmup 5] [--n 500000]
    python tools/wide_bench.py --clustered [--segments -1 0] [--channels 4 8 16]

Device-event timing of whole steps (projection excluded: it is shared by every variant), warm-up first, then the variants
run in alternating order `reps` times; prints the median milliseconds per step (tools/timing.py's loop: --warmup
interleaved rounds, one call per window, mirrored order, a fresh event pair per window, the mean-of-middles median).
Per-kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/wide_bench.py --reps 5`.

--clustered: the wide path on the uniform scene and on the clustered one (half of the splats in the central 10 % x 10 %
of the frame: the construction of tests/test_gpu_segments.py) under every RasterConfig.segment_pairs value of --segments
(-1: the automatic rule, 0: no segmentation, n: n-pair segments with the automatic heavy threshold), all variants
alternating in one process: the step by device events, then composite_forward + composite_backward (K6 + K7) by
renderer.KernelTimer, and the clustered / uniform ratio of K6 + K7 per width and segment setting.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import renderer, synthetic  # noqa: E402
from timing import mid_median, repetitions  # noqa: E402


def clustered_scene(n, w, h, frac, region, seed=0):
  """`frac` of the splats moved into the central `region` x `region` of the image (tests/test_gpu_segments.py)."""
  g, cam = synthetic.scene_a(n, w, h, sh_degree=0, seed=seed)
  k = int(frac * n)
  gen = torch.Generator().manual_seed(1)
  fx = w / (2.0 * math.tan(math.radians(30.0)))
  z = g.position[:k, 2]
  u = (0.5 + region * (torch.rand(k, generator=gen) - 0.5)) * w
  v = (0.5 + region * (torch.rand(k, generator=gen) - 0.5)) * h
  g.position[:k, 0] = (u - w / 2) * z / fx
  g.position[:k, 1] = (v - h / 2) * z / fx
  return g, cam


def clustered_main(args):
  W, H = 1920, 1080
  scenes = {}
  for name, frac, region in (("uniform", 0.0, 1.0), ("clustered", 0.5, 0.1)):
    if name not in args.scenes:
      continue
    g, cam = clustered_scene(args.n, W, H, frac, region)
    cam = cam.to("cuda")
    gd = sta.Gaussians3D(*(t.cuda() for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
    with torch.no_grad():
      g2d, depth, idx = sta.project_to_image(gd, cam, sta.RasterConfig())
    scenes[name] = (cam, idx, g2d.detach().clone().requires_grad_(True), depth)
  torch.manual_seed(0)
  feats = {(s, c): torch.rand(scenes[s][1].shape[0], c, device="cuda") for s in scenes for c in args.channels}
  grads = {c: torch.rand(H, W, c, device="cuda") for c in args.channels}
  cfgs = {seg: sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True, segment_pairs=seg)
          for seg in args.segments}
  variants = [(s, seg, c) for c in args.channels for seg in args.segments for s in scenes]

  def step(v):
    s, seg, c = v
    cam, idx, g2, depth = scenes[s]
    f = feats[(s, c)].requires_grad_(True)
    r = sta.render_projected(idx, g2, f, depth, cam, cfgs[seg])
    r.image.backward(grads[c])
    f.grad = None
    g2.grad = None
    return r

  overlaps = {}

  def counted(v):                                              # every call notes its scene's pair count
    overlaps[v[0]] = step(v).num_overlaps

  steps = repetitions([(v, lambda v=v: counted(v)) for v in variants], args.reps, args.warmup, order="mirrored",
                      fresh_events=True)
  k67 = {v: [] for v in variants}
  for rep in range(args.reps):
    for v in (variants if rep % 2 == 0 else list(reversed(variants))):
      timer = renderer.KernelTimer()
      renderer.KERNEL_TIMER = timer
      try:
        step(v)
        ks = timer.summary()
      finally:
        renderer.KERNEL_TIMER = None
      k67[v].append((ks["composite_forward"][1], ks["composite_backward"][1]))
  print(f"{args.n} splats, {W}x{H}; pairs: " + ", ".join(f"{s} {o}" for s, o in overlaps.items()) +
        f"; medians over {args.reps} alternating runs")
  out = {}
  for c in args.channels:
    for seg in args.segments:
      row = {}
      for s in scenes:
        v = (s, seg, c)
        k6 = statistics.median(t[0] for t in k67[v])
        k7 = statistics.median(t[1] for t in k67[v])
        row[s] = dict(step_ms=mid_median(steps[v]), step_min=min(steps[v]), step_max=max(steps[v]), k6_ms=k6, k7_ms=k7)
        print(f"  C={c:2d} segment_pairs={seg:4d} {s:9s}  step {row[s]['step_ms']:8.3f} ms (min {row[s]['step_min']:.3f}, "
              f"max {row[s]['step_max']:.3f})   K6 {k6 * 1e3:7.0f} us  K7 {k7 * 1e3:7.0f} us")
      if len(row) == 2:
        ratio = (row["clustered"]["k6_ms"] + row["clustered"]["k7_ms"]) / (row["uniform"]["k6_ms"] + row["uniform"]["k7_ms"])
        row["k67_clustered_over_uniform"] = ratio
        print(f"  C={c:2d} segment_pairs={seg:4d} K6 + K7 clustered / uniform = {ratio:.2f}")
      out[f"C={c} seg={seg}"] = row
  print(json.dumps(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--n", type=int, default=500_000)
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--clustered", action="store_true", help="uniform and clustered scene, every --segments value")
  ap.add_argument("--segments", type=int, nargs="+", default=[-1, 0], help="RasterConfig.segment_pairs values (--clustered)")
  ap.add_argument("--channels", type=int, nargs="+", default=[4, 8, 16], help="channel counts (--clustered)")
  ap.add_argument("--scenes", nargs="+", default=["uniform", "clustered"], choices=["uniform", "clustered"],
                  help="scenes of --clustered (one alone: for a profiler run)")
  args = ap.parse_args()
  torch.cuda.set_device(0)
  if args.clustered:
    return clustered_main(args)
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
  times = repetitions([(k, lambda v=v: step(v)) for k, v in variants.items()], args.reps, args.warmup, order="mirrored",
                      fresh_events=True)
  med = {k: mid_median(v) for k, v in times.items()}
  print(f"c2 geometry: M={M} visible splats, 1920x1080; median ms per fwd+bwd step over {args.reps} alternating runs")
  for k, v in med.items():
    print(f"  {k:10s} {v:8.3f} ms   (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
  print(json.dumps({"M": M, "median_ms": med}))


if __name__ == "__main__":
  main()
