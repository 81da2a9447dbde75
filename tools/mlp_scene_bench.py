"""Times the native scene regulariser and post-step projection (splat_trainer_amd.reg, csrc/reg.hip) and the whole
``MLPScene`` training step at the size of workload c2 (scene A, 500 000 points, 1920 x 1080), next to the torch form a
user wrote before (tests/test_gpu_dropin_flow.py:38-46 through ``points.visible``).  HIP-event medians after warm-up,
the two forms alternated in the same process; host synchronisations per call counted with torch's sync debug mode.
The loop is tools/timing.py's: 3 interleaved warm-up rounds (2 for the whole step), --reps repetitions of one call, fixed
order, one reused event pair, lower median and minimum in microseconds.

    python tools/mlp_scene_bench.py [--points 500000] [--reps 30] [--parts reg post step]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/mlp_scene_bench.py --trace native --calls 40
    python tools/mlp_scene_bench.py --launches OUT --calls 40 [--setup OUT0]

``--trace native|torch|none`` only runs ``--calls`` forward + backward calls of that form on seeded rows (``none``: the
set-up alone), for a kernel-trace run of its own; ``--launches`` then prints the kernel launches per call of such a run,
less the launches of a ``--trace none`` run.  The only assertion: the native form is not slower than the torch form.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import sys
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import reg, synthetic  # noqa: E402
from timing import lower_median, repetitions  # noqa: E402

WEIGHTS = dict(scale=0.01, opacity=1.0, aspect=1e-4, specular=1e-5)          # config/scene/mlp.yaml:16-20 at t = 0
PARAMETERS = dict(position=dict(lr=0.3, type="local_vector"), log_scaling=dict(lr=0.08),
                  rotation=dict(lr=0.01, type="vector"), alpha_logit=dict(lr=0.1), feature=dict(lr=5.0, type="vector"))


def saturate(t, gain=4.0, k=2.0):
  return (1 - 1 / torch.exp(gain * t)).pow(k)


def torch_reg(points, log_scaling, weights=WEIGHTS):
  """mlp_scene.py:246-288 as torch ops through ``points.visible`` (nonzero: a host wait) -- the path before this kernel."""
  pv = points.visible
  scale = torch.exp(log_scaling[pv.idx])
  norm_scale = scale.pow(2).sum(1) / pv.depths.pow(2).squeeze(-1)
  opacity_term = saturate(pv.opacity) * norm_scale
  aspect = scale.max(1).values / scale.min(1).values
  spec = pv.attributes.specular.abs().sum(1)
  w = pv.visibility
  return (weights["scale"] * (norm_scale * w).mean() + weights["opacity"] * (opacity_term * w).mean() +
          weights["aspect"] * (aspect * w).mean() + weights["specular"] * (spec * w).mean())


def timed_pair(fns: dict, reps: int, warmup: int = 3) -> dict:
  """Median us per call of each function, the functions alternated call by call."""
  return {k: (lower_median(v) * 1e3, min(v) * 1e3) for k, v in repetitions(fns, reps, warmup).items()}


def count_syncs(fn) -> int:
  torch.cuda.synchronize()
  previous = torch.cuda.get_sync_debug_mode()
  with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter("always")
    torch.cuda.set_sync_debug_mode("warn")
    try:
      fn()
    finally:
      torch.cuda.set_sync_debug_mode(previous)
  return sum(1 for w in caught if "called a synchronizing" in str(w.message))


def seeded_rows(M: int, N: int, hidden: float = 0.3):
  """Rows as a frame would hand them over, ``hidden`` of them with visibility 0."""
  gen = torch.Generator(device="cuda").manual_seed(0)
  r = lambda *s: torch.rand(*s, device="cuda", generator=gen)
  idx = torch.randperm(N, device="cuda", generator=gen)[:M].sort().values
  vis = r(M) * (r(M) > hidden)
  opacity, depths = r(M).requires_grad_(True), (2 + 8 * r(M, 1)).requires_grad_(True)
  specular = (r(M, 3) - 0.5).requires_grad_(True)
  log_scaling = (-4 + r(N, 3)).requires_grad_(True)
  z = torch.zeros(M, device="cuda")
  points = sta.RenderedPoints(idx=idx, depths=depths, opacity=opacity, screen_scale=torch.zeros(M, 2, device="cuda"),
                              visibility=vis, prune_cost=z, split_score=z,
                              attributes=sta.Colors(torch.zeros_like(specular), specular))
  return points, [opacity, depths, specular, log_scaling]


def reg_calls(points, leaves):
  def native():
    torch.autograd.grad(sta.reg_loss(points, leaves[-1], WEIGHTS), leaves)

  def torch_form():
    torch.autograd.grad(torch_reg(points, leaves[-1]), leaves)

  return dict(native=native, torch=torch_form)


def bench_reg(scene, cam, reps):
  with torch.no_grad():
    r = scene.render(cam, image_idx=0, compute_visibility=True)
  p = r.points
  leaves = [p.opacity.detach().clone().requires_grad_(True), p.depths.detach().clone().requires_grad_(True),
            p.attributes.specular.detach().clone().requires_grad_(True),
            scene.points.log_scaling.detach().clone().requires_grad_(True)]
  points = p.replace(opacity=leaves[0], depths=leaves[1], attributes=sta.Colors(p.attributes.diffuse.detach(), leaves[2]))
  M, N = int(p.idx.shape[0]), scene.num_points
  calls = reg_calls(points, leaves)
  a = sta.reg_loss(points, leaves[-1], WEIGHTS).item()
  b = torch_reg(points, leaves[-1]).item()
  t = timed_pair(calls, reps)
  syncs = {k: count_syncs(fn) for k, fn in calls.items()}
  print(f"reg_loss forward + backward, M = {M} of N = {N} rows, {int((p.visibility > 0).sum())} visible: "
        f"loss native {a:.6e} torch {b:.6e}")
  for k in ("native", "torch"):
    print(f"  {k:6s} median {t[k][0]:8.1f} us  min {t[k][1]:8.1f} us  host syncs per call {syncs[k]}")
  print(f"  torch / native = x{t['torch'][0] / t['native'][0]:.1f}")
  assert t["native"][0] <= t["torch"][0], "the native regulariser is slower than the torch form"


def bench_post(scene, reps):
  pts = scene.points
  rot, ls = pts.rotation.detach().clone(), pts.log_scaling.detach().clone()

  def native():
    reg.scene_post_step(rot, ls)

  def torch_form():
    rot.copy_(F.normalize(rot, dim=1))          # (the reference rebinds .data; the copy keeps both forms on one buffer)
    ls.clamp_(min=-8, max=8)

  def torch_rebind():
    pts.rotation.data = F.normalize(pts.rotation.data, dim=1)
    pts.log_scaling.data.clamp_(min=-8, max=8)

  t = timed_pair(dict(native=native, torch=torch_form, torch_rebind=torch_rebind), reps)
  print(f"post-step projection over N = {scene.num_points} rows:")
  for k, (med, mn) in t.items():
    print(f"  {k:12s} median {med:8.1f} us  min {mn:8.1f} us")


def bench_step(scene, cam, target, reps):
  def step_with(reg_fn):
    def step():
      r = scene.render(cam, image_idx=0, compute_visibility=True, compute_point_heuristic=True)
      loss = sta.reference_loss(r.image, target) + reg_fn(r)
      loss.backward()
      scene.add_rendering(0, r)
      scene.step()
    return step

  fns = dict(native=step_with(lambda r: scene.reg_loss(r, WEIGHTS)),
             torch=step_with(lambda r: torch_reg(r.points, scene.points.log_scaling)))
  t = timed_pair(fns, reps, warmup=2)
  syncs = {k: count_syncs(fn) for k, fn in fns.items()}
  print(f"MLPScene training step (render + reference_loss + reg_loss + backward + add_rendering + step), "
        f"N = {scene.num_points}, {cam.image_size[0]} x {cam.image_size[1]}:")
  for k in ("native", "torch"):
    print(f"  reg_loss {k:6s} median {t[k][0] / 1e3:8.2f} ms  min {t[k][1] / 1e3:8.2f} ms  host syncs per step {syncs[k]}")


def launches(directory: str) -> int:
  hits = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
  if not hits:
    raise SystemExit(f"no *kernel_stats.csv under {directory}")
  return sum(int(r["Calls"]) for r in csv.DictReader(open(hits[-1])))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--points", type=int, default=500_000)
  ap.add_argument("--size", type=int, nargs=2, default=[1920, 1080])
  ap.add_argument("--reps", type=int, default=30)
  ap.add_argument("--parts", nargs="+", default=["reg", "post", "step"], choices=["reg", "post", "step"])
  ap.add_argument("--trace", choices=["native", "torch", "none"], default=None)
  ap.add_argument("--calls", type=int, default=40)
  ap.add_argument("--launches", default=None)
  ap.add_argument("--setup", default=None)
  args = ap.parse_args()
  if args.launches:
    total, setup = launches(args.launches), launches(args.setup) if args.setup else 0
    print(f"{args.launches}: {total} kernel launches, set-up {setup}, {args.calls} calls: "
          f"{(total - setup) / args.calls:.1f} launches per forward + backward call")
    return
  if not torch.cuda.is_available():
    raise SystemExit("no GPU: this benchmark measures on the device only")
  if args.trace:
    points, leaves = seeded_rows(args.points, args.points)
    if args.trace != "none":
      fn = reg_calls(points, leaves)[args.trace]
      for _ in range(args.calls):
        fn()
    torch.cuda.synchronize()
    return
  W, H = args.size
  g, cam = synthetic.scene_a(args.points, W, H, sh_degree=0, seed=0)
  cam = cam.to("cuda")
  torch.manual_seed(0)
  config = sta.MLPSceneConfig(parameters=PARAMETERS, reg_weight=WEIGHTS,
                              color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=5, lr_diffuse=1e-2, lr_specular=1e-2),
                              lr_glo_feature=2.0, beta2=0.95, vis_beta=0.999, vis_smooth=0.01, image_features=32,
                              point_features=16)                                # config/scene/mlp.yaml
  scene = config.from_color_gaussians(g, 1, "cuda", seed=0)
  if "reg" in args.parts:
    bench_reg(scene, cam, args.reps)
  if "post" in args.parts:
    bench_post(scene, args.reps)
  if "step" in args.parts:
    target = torch.rand(H, W, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    bench_step(scene, cam, target, max(5, args.reps // 3))


if __name__ == "__main__":
  main()
