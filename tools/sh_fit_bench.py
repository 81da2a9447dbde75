"""Times the direct SH export fit (splat_trainer_amd.sh_fit) on the synthetic scenes, 32 cameras:

    python tools/sh_fit_bench.py [--quick] [--json out.json]

kernels alone    ``gsr_sh_fit_accumulate`` over every row (M = N) and over a sorted random quarter of them, and
                 ``gsr_sh_fit_solve``, through the C ABI between two device events, median and [min, max] of 5 timings;
                 bytes moved per row (accumulate: the row read and written, 2 x 8 R(K); solve: the row read, 3 K + 1
                 floats written) and the rate that makes;
export           a whole ``MLPScene.to_sh_gaussians(method="lstsq")`` against ``method="adam", epochs=1`` on the same
                 scene and cameras, alternated repetition by repetition, wall clock around a device synchronisation
                 (both spend most of their time in the per-camera visibility query and colour model, which they share);
quality          both exports' visibility-weighted colour MSE, prediction clamped to [0, 1], on the 32 fitted views and on
                 8 held-out views of the same ring.

The loops are tools/timing.py's.  Kernels alone: 1 warm-up launch, 5 windows of 4 launches, a fresh event pair per window,
lower median.  Export: 1 warm-up call of each form, 3 repetitions of one call, fixed order, host clock, lower median.
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
from splat_trainer_amd import _lib, mlp_scene, sh_fit, synthetic  # noqa: E402
from timing import HostClock, clear, lower_median, repetitions, spread  # noqa: E402

PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))


def timed(fn, launches, reps=5):
  times = repetitions({"fn": fn}, reps, warmup=1, calls=launches, fresh_events=True)["fn"]
  return lower_median(times), [round(t, 4) for t in spread(times)]


def kernels_alone(N, degree, gen):
  lib, K = _lib.load(), (degree + 1) ** 2
  R = lib.gsr_sh_fit_row_doubles(K)
  positions = torch.randn(N, 3, generator=gen).cuda()
  fit = sta.ShFit(positions, degree)
  cam = torch.tensor([0.0, 0.0, 4.0]).cuda()
  p, stream = (lambda t: t.data_ptr()), _lib.current_stream_ptr()
  rows = []
  for label, M in (("every row", N), ("a sorted random quarter", N // 4)):
    idx = torch.randperm(N, generator=gen)[:M].sort().values.cuda() if M < N else torch.arange(N).cuda()
    col, w = torch.rand(M, 3, generator=gen).cuda(), (0.1 + 0.9 * torch.rand(M, generator=gen)).cuda()
    run = lambda: _lib.check(lib.gsr_sh_fit_accumulate(p(positions), N, p(idx), M, p(col), p(w), p(cam), K, p(fit.acc),
                                                       stream), "gsr_sh_fit_accumulate")
    ms, span = timed(run, launches=4)
    moved = 2 * 8 * R
    rows.append(dict(what=f"accumulate N={N} degree={degree} {label}", M=M, ms=round(ms, 4), range=span,
                     bytes_per_row=moved, TB_per_s=round(M * moved / ms / 1e9, 3)))
  sh, weight = torch.empty(N, 3, K, device="cuda"), torch.empty(N, device="cuda")
  run = lambda: _lib.check(lib.gsr_sh_fit_solve(p(fit.acc), N, K, sh_fit.DEFAULT_RIDGE, p(sh), p(weight), stream),
                           "gsr_sh_fit_solve")
  ms, span = timed(run, launches=4)
  moved = 8 * R + 4 * (3 * K + 1)
  rows.append(dict(what=f"solve N={N} degree={degree}", ms=round(ms, 4), range=span, bytes_per_row=moved,
                   TB_per_s=round(N * moved / ms / 1e9, 3)))
  return rows


def make_scene(N, width, height, cameras):
  g, cams = synthetic.scene_b(N, width, height, sh_degree=0, seed=9, num_cameras=cameras)
  config = sta.MLPSceneConfig(parameters=PARAMETERS, reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
                              color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=3), image_features=8,
                              point_features=8)
  torch.manual_seed(5)
  scene = config.from_color_gaussians(g, cameras, "cuda", seed=5)
  return scene, [c.to("cuda") for c in cams]


def weighted_mse(scene, feature, cams, image_indexes):
  positions, total = scene.points.position.detach(), []
  with torch.no_grad():
    for cam, i in zip(cams, image_indexes):
      half = mlp_scene.resized_camera(cam, 0.5)
      idx, vis = scene.query_visibility(half)
      if idx.shape[0] == 0:
        continue
      want = scene.color_model.post_activation(scene.eval_colors(idx, half, i).total())
      got = sta.evaluate_sh_at(feature, positions, idx, half.camera_position).clamp(0, 1)
      total.append((((got - want) ** 2).mean(dim=1) * vis).sum().item() / vis.sum().item())
  return sum(total) / max(len(total), 1)


def export(N, width, height, reps):
  scene, cams = make_scene(N, width, height, 40)
  held = list(range(0, 40, 5))
  fitted = [i for i in range(40) if i not in held]
  fit_cams, held_cams = [cams[i] for i in fitted], [cams[i] for i in held]

  features = {}                                             # each form's last result, for the quality figures

  def lstsq():
    features["lstsq"] = scene.to_sh_gaussians(fit_cams, fitted, sh_degree=2, method="lstsq").feature

  def adam():
    features["adam"] = scene.to_sh_gaussians(fit_cams, fitted, epochs=1, sh_degree=2,
                                             generator=torch.Generator().manual_seed(0)).feature

  times = repetitions(dict(lstsq=lstsq, adam=adam), reps, warmup=1, clock=HostClock())
  out = dict(what=f"to_sh_gaussians N={N} cameras={len(fitted)} at {width // 2}x{height // 2} degree=2")
  for name, ts in times.items():
    out[f"{name}_ms"] = round(lower_median(ts), 2)
    out[f"{name}_range"] = [round(t, 2) for t in spread(ts)]
    out[f"{name}_mse_fitted"] = float(f"{weighted_mse(scene, features[name], fit_cams, fitted):.4e}")
    out[f"{name}_mse_held_out"] = float(f"{weighted_mse(scene, features[name], held_cams, held):.4e}")
  out["adam_over_lstsq"] = round(out["adam_ms"] / out["lstsq_ms"], 2)
  out["lstsq_faster_every_repetition"] = clear(times["lstsq"], times["adam"])
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--quick", action="store_true", help="small sizes (a functional run)")
  ap.add_argument("--json", default=None)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  gen = torch.Generator().manual_seed(0)
  sizes = (20_000, 50_000) if args.quick else (500_000, 3_000_000)
  rows = []

  def report(new_rows):
    for r in new_rows:
      print(json.dumps(r), flush=True)
    rows.extend(new_rows)

  for N in sizes:
    for degree in (2, 3):
      report(kernels_alone(N, degree, gen))
  width, height = (320, 240) if args.quick else (1280, 960)
  for N in sizes:
    report([export(N, width, height, reps=3)])
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
