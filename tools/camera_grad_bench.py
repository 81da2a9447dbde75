"""Cost of the camera gradient: one-call fwd+bwd steps (render_gaussians(use_sh=True) + clamped MSE + backward) on c2 and
c3 with and without T_camera_world / projection requiring grad, in the same process.

    python tools/camera_grad_bench.py [--workloads c2,c3] [--reps 30] [--warmup 5] [--only base|camera]

Device-event timing of whole steps, warm-up first, then the two variants alternate (order flipped every repetition);
prints the median ms per step of each and the difference (tools/timing.py's loop: --warmup interleaved rounds, one call
per window, mirrored order, a fresh event pair per window, the mean-of-middles median).  ``--only``: one variant alone, for a
`rocprofv3 --kernel-trace --stats -- python tools/camera_grad_bench.py --only camera --reps 5` run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import synthetic  # noqa: E402
from timing import mid_median, repetitions  # noqa: E402

SCENES = {"c2": lambda: synthetic.scene_a(500_000, 1920, 1080, sh_degree=3, seed=0),
          "c3": lambda: (lambda g, cams: (g, cams[0]))(*synthetic.scene_b(3_000_000, 1920, 1080, sh_degree=3, seed=1))}


def measure(name: str, reps: int, warmup: int, only=None) -> dict:
  g, cam = SCENES[name]()
  cfg = sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True)
  params = [t.cuda().requires_grad_(True) for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)]
  gd = sta.Gaussians3D(*params)
  T, proj = cam.T_camera_world.cuda(), cam.projection.cuda()
  Tg, pg = T.clone().requires_grad_(True), proj.clone().requires_grad_(True)
  cams = {"base": sta.CameraParams(T, proj, cam.image_size, cam.near_plane, cam.far_plane),
          "camera": sta.CameraParams(Tg, pg, cam.image_size, cam.near_plane, cam.far_plane)}
  variants = [only] if only else ["base", "camera"]

  def step(v):
    r = sta.render_gaussians(gd, cams[v], cfg, use_sh=True)
    ((r.image.clamp(0, 1) - 0.5) ** 2).mean().backward()
    for p in params + [Tg, pg]:
      p.grad = None

  times = repetitions([(v, lambda v=v: step(v)) for v in variants], reps, warmup, order="mirrored", fresh_events=True)
  out = {v: dict(median_ms=mid_median(t), min_ms=min(t), max_ms=max(t)) for v, t in times.items()}
  if not only:
    out["camera_minus_base_ms"] = out["camera"]["median_ms"] - out["base"]["median_ms"]
    out["overhead_pct"] = 100.0 * out["camera_minus_base_ms"] / out["base"]["median_ms"]
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--workloads", default="c2,c3")
  ap.add_argument("--reps", type=int, default=30)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--only", choices=["base", "camera"], default=None)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  res = {}
  for name in args.workloads.split(","):
    res[name] = measure(name, args.reps, args.warmup, args.only)
    r = res[name]
    line = "  ".join(f"{v} {r[v]['median_ms']:.3f} ms" for v in ("base", "camera") if v in r)
    if "overhead_pct" in r:
      line += f"  difference {r['camera_minus_base_ms'] * 1000:.1f} us ({r['overhead_pct']:+.2f} %)"
    print(f"{name}: median per one-call fwd+bwd step over {args.reps} alternating runs: {line}", flush=True)
  print(json.dumps(res))


if __name__ == "__main__":
  main()
