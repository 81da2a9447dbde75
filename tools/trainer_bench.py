"""Two measurements of the trainer layer on one GPU, in one process.

    python tools/trainer_bench.py [--quick] [--json out.json]

(a) All histograms of one ``log_details`` step -- 10 of gradients (gathered by the visible rows, raw and divided by the
    visibility), 10 of optimizer state, 6 of parameters, 4 of a rendering's per-point outputs: 30 -- on a point table of
    0.5 M and 3 M rows, native (``tensor_histogram``, csrc/histogram.hip) against the torch form of the reference written
    out below: boolean-mask index, ``log10``, ``min`` / ``max`` with their two ``.item()`` waits for the range, then the
    reference's ``Histogram`` (bin computation, ``.long()``, a second mask index for ``trim``, ``sum().item()``,
    ``norm().item()``, ``bincount``).  Both are timed wall-clock from a drained device to a drained device, after every
    native histogram has been read on the host (one copy each), alternated repetition by repetition after a warm-up;
    median [min, max] ms.  Launches are counted with torch's profiler (device kernels and memsets of one repetition),
    host waits with ``torch.cuda.set_sync_debug_mode("warn")``.  The native sweep's bytes (values read once per pass,
    twice with a found range, plus the gather list and the weights) over its device time is its achieved bandwidth.
(b) Steps per second of ``Trainer.train`` (``log_details=False``) on a small synthetic scene against a hand-written loop
    of the same native calls in the same order, five runs each, each run on a fresh scene from the same seed.

It runs no reference code.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import synthetic  # noqa: E402

VIS_SMOOTH, MIN_VIS, BINS = 1e-3, 0.1, 64


# ------------------------------------------------------------------------------------------------- (a) the histograms
def point_table(n: int, seed: int = 0):
  """Tensors shaped like an MLPScene's after a backward: parameters, gradients (zero on the rows no view saw), optimizer
  state, accumulated visibility, and a rendering's per-point outputs over the M rows it culled to."""
  gen = torch.Generator(device="cuda").manual_seed(seed)
  rand = lambda *s: torch.randn(*s, device="cuda", generator=gen)
  widths = dict(position=3, log_scaling=3, rotation=4, alpha_logit=1, feature=8)
  visible = torch.where(torch.rand(n, device="cuda", generator=gen) < 0.6, torch.exp(2.0 * rand(n)), torch.zeros(n, device="cuda"))
  seen = (visible > 0)[:, None]
  table = dict(visible=visible, params={k: rand(n, c) for k, c in widths.items()},
               grads={k: torch.exp(3.0 * rand(n, c) - 6.0) * torch.sign(rand(n, c)) * seen for k, c in widths.items()},
               state={k: dict(exp_avg=0.2 * rand(n, c), exp_avg_sq=torch.exp(2.0 * rand(n, c) - 8.0)) for k, c in widths.items()},
               glo=rand(200, 8))
  m = n // 3
  table["rendering"] = dict(prune_cost=torch.exp(3.0 * rand(m) - 12.0), split_score=torch.exp(3.0 * rand(m) - 9.0),
                            screen_scale=torch.exp(rand(m, 2)), visibility=torch.exp(2.0 * rand(m)) * (rand(m) > -0.5))
  return table


def native_step(table):
  out = []
  visible = table["visible"]
  vis_idx = torch.nonzero(visible > MIN_VIS).squeeze(1)
  for g in table["grads"].values():
    out.append(sta.tensor_histogram(g, BINS, rows=vis_idx, log10="drop", min_value=1e-16))
    out.append(sta.tensor_histogram(g, BINS, rows=vis_idx, weight=visible, eps=VIS_SMOOTH, log10="drop", min_value=1e-16))
  for state in table["state"].values():
    for v in state.values():
      out.append(sta.tensor_histogram(v, BINS, log10="drop", min_value=1e-16))
  p = table["params"]
  scale = torch.exp(p["log_scaling"])
  largest = scale.max(1).values
  for v in (torch.sigmoid(p["alpha_logit"]), p["log_scaling"], p["feature"], table["glo"], scale.sum(1) / largest,
            largest / (scale.min(1).values + 1e-4)):
    out.append(sta.tensor_histogram(v, BINS))
  r = table["rendering"]
  rows = torch.nonzero(r["visibility"] > 0).squeeze(1)
  for name, min_value in (("prune_cost", 1e-20), ("split_score", 1e-10), ("screen_scale", 1e-6), ("visibility", 1e-10)):
    out.append(sta.tensor_histogram(r[name], BINS, rows=rows, log10="drop", min_value=min_value))
  return [(h.counts.shape[0], h.sum, h.sum_squares, h.range) for h in out]       # read on the host, one copy each


def torch_histogram(values, num_bins=BINS):
  """A logger's histogram of a tensor in the reference's form: the range by two waits, then its Histogram class."""
  values = values.reshape(-1)
  if values.numel() == 0:
    return torch.zeros(num_bins, dtype=torch.long, device=values.device), 0.0, 0.0
  lower, upper = values.min().item(), values.max().item()
  index = ((values - lower) * num_bins / max(upper - lower, 1e-30)).long()
  valid = (index >= 0) & (index < num_bins)
  values, index = values[valid], index[valid]
  index.clamp_(0, num_bins - 1)
  return torch.bincount(index, minlength=num_bins), values.sum().item(), values.norm(2).item()


def torch_log_nonzero(value, min_value):
  return torch_histogram(torch.log10(value[value > min_value]))


def torch_step(table):
  out = []
  visible = table["visible"]
  vis_idx = torch.nonzero(visible > MIN_VIS).squeeze(1)
  weight = visible[vis_idx].view(-1, 1)
  for g in table["grads"].values():
    grad = g[vis_idx].view(vis_idx.shape[0], -1)
    out.append(torch_log_nonzero(grad, 1e-16))
    out.append(torch_log_nonzero(grad / (VIS_SMOOTH + weight), 1e-16))
  for state in table["state"].values():
    for v in state.values():
      out.append(torch_log_nonzero(v, 1e-16))
  p = table["params"]
  scale = torch.exp(p["log_scaling"])
  largest = scale.max(1).values
  for v in (torch.sigmoid(p["alpha_logit"]), p["log_scaling"], p["feature"], table["glo"], scale.sum(1) / largest,
            largest / (scale.min(1).values + 1e-4)):
    out.append(torch_histogram(v))
  r = table["rendering"]
  mask = r["visibility"] > 0
  for name, min_value in (("prune_cost", 1e-20), ("split_score", 1e-10), ("screen_scale", 1e-6), ("visibility", 1e-10)):
    out.append(torch_log_nonzero(r[name][mask], min_value))
  return out


def wall_ms(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3


def launches_and_waits(fn):
  previous = torch.cuda.get_sync_debug_mode()
  with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter("always")
    torch.cuda.set_sync_debug_mode("warn")
    try:
      fn()
    finally:
      torch.cuda.set_sync_debug_mode(previous)
  waits = sum("synchron" in str(w.message) for w in caught)
  try:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
      fn()
      torch.cuda.synchronize()
    device = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
    launches = len(device)
    device_ms = sum(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0) for e in device) / 1e3
  except Exception as e:                                   # (the profiler is optional: the times do not depend on it)
    launches, device_ms = f"n/a ({type(e).__name__})", None
  return launches, waits, device_ms


def native_bytes(table):
  """Bytes the native sweeps read: every values tensor once per pass (two with a found range), a gathered one only its
  rows, plus the gather list and the weights."""
  vis_rows = int((table["visible"] > MIN_VIS).sum())
  total = 0
  for g in table["grads"].values():
    total += 2 * (vis_rows * g.shape[1] * 4 + vis_rows * 8) * 2 + 2 * vis_rows * 4
  for state in table["state"].values():
    total += sum(2 * v.numel() * 4 for v in state.values())
  n = table["visible"].shape[0]
  total += 2 * 4 * (n + 3 * n + 8 * n + table["glo"].numel() + n + n)
  r = table["rendering"]
  rows = int((r["visibility"] > 0).sum())
  total += sum(2 * (rows * (v.numel() // v.shape[0]) * 4 + rows * 8) for v in r.values())
  return total


def bench_histograms(n: int, reps: int):
  table = point_table(n)
  for _ in range(2):
    native_step(table)
    torch_step(table)
  native, ref = [], []
  for _ in range(reps):
    native.append(wall_ms(lambda: native_step(table)))
    ref.append(wall_ms(lambda: torch_step(table)))
  stat = lambda t: [round(x, 3) for x in (sorted(t)[len(t) // 2], min(t), max(t))]
  n_launch, n_wait, n_dev = launches_and_waits(lambda: native_step(table))
  t_launch, t_wait, t_dev = launches_and_waits(lambda: torch_step(table))
  gb = native_bytes(table) / 1e9
  return dict(points=n, native_ms=stat(native), torch_ms=stat(ref), clear=max(native) < min(ref),
              native_launches=n_launch, native_waits=n_wait, torch_launches=t_launch, torch_waits=t_wait,
              native_device_ms=None if n_dev is None else round(n_dev, 3), torch_device_ms=None if t_dev is None else round(t_dev, 3),
              native_read_gb=round(gb, 3), native_gb_per_s=None if not n_dev else round(gb / (n_dev / 1e3), 1))


# ----------------------------------------------------------------------------------------------------- (b) the trainer
PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))


def make_dataset(points: int, w: int, h: int, cameras: int):
  g, cams = synthetic.scene_b(2 * points, w, h, sh_degree=1, seed=4, num_cameras=cameras, sigma_px=2.5)
  gd = g.to("cuda")
  with torch.no_grad():
    images = [(sta.render_gaussians(gd, c.to("cuda"), sta.RasterConfig(), use_sh=True).image.clamp(0, 1) * 255).round()
              .to(torch.uint8).cpu() for c in cams]
  keep = torch.randperm(2 * points, generator=torch.Generator().manual_seed(1))[:points]
  cloud = sta.PointCloud(g.position[keep], (0.5 + 0.282094791773878 * g.feature[keep, :, 0]).clamp(0, 1))
  projection = sta.Projections(intrinsics=cams[0].projection[None], image_size=torch.tensor([[w, h]]),
                               depth_range=torch.tensor([[0.1, 100.0]]))
  table = sta.MultiCameraTable(camera_t_world=torch.stack([c.T_camera_world for c in cams]),
                               camera_idx=torch.zeros(cameras, dtype=torch.int64), projection=projection,
                               image_names=[f"view/{i}.png" for i in range(cameras)],
                               labels=torch.full((cameras,), 2, dtype=torch.int64))
  return sta.TensorDataset(table, images, cloud=cloud)


def make_trainer(dataset, steps: int, out: str):
  scene = sta.MLPSceneConfig(parameters=PARAMETERS, reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
                             color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=3, lr_diffuse=1e-2, lr_specular=1e-2),
                             lr_glo_feature=0.1, image_features=8, point_features=8)
  config = sta.TrainConfig(scene=scene, controller=sta.TargetConfig(prune_rate=0.025, min_views=2, densify_prune_interval=50),
                           view_selection=sta.RandomSamplerConfig(batch_size=1),
                           cloud_init=sta.CloudInitConfig(num_neighbors=3, initial_point_scale=0.5, initial_alpha=0.5),
                           total_steps=steps, eval_steps=10 ** 9, log_interval=10, log_details=False,
                           target_points=int(1.2 * dataset.pointcloud().num_points), l1_weight=0.8, ssim_weight=0.2, ssim_levels=2,
                           vis_clusters=64, device="cuda", save_output=False, output_path=out, seed=3, log_images=False)
  torch.manual_seed(0)
  return sta.Trainer.initialize(config, dataset, sta.NullLogger())


def trainer_rate(dataset, steps: int, out: str) -> float:
  """Steps per second of Trainer.train between its first and its last logging step (the evaluation at step 0 is outside)."""
  trainer = make_trainer(dataset, steps, out)
  os.environ["TQDM_DISABLE"] = "1"
  marks = []

  def mark():
    torch.cuda.synchronize()
    marks.append((trainer.step, time.perf_counter()))
  trainer.bind(on_update=mark)
  trainer.train()
  (s0, t0), (s1, t1) = marks[0], marks[-1]
  return (s1 - s0) / (t1 - t0)


def hand_rate(dataset, steps: int, out: str) -> float:
  """The same native calls in the same order, written out: no Trainer.train, no logger, no prefetch thread."""
  trainer = make_trainer(dataset, steps, out)                               # (for the scene, the controller and the sampler)
  scene, controller, sampler, config = trainer.scene, trainer.controller, trainer.view_selection, trainer.config
  images = {v.image_idx: trainer.load_data(v).image for v in dataset.train(shuffle=False)}
  cameras = {i: trainer.camera_params(i) for i in images}
  step, t0, s0 = 0, None, None
  while step < steps:
    i = int(sampler.select_images(None, None)[0])
    step += 1
    progress = sta.Progress(step, steps, step % config.log_interval == 0)
    rendering = scene.render(cameras[i], i, antialias=False, compute_visibility=True, compute_point_heuristic=True, blur_cov=0.3)
    loss = sta.reference_loss(rendering.image, images[i], l1_weight=config.l1_weight, mse_weight=config.mse_weight,
                              ssim_weight=config.ssim_weight, ssim_levels=config.ssim_levels)
    (loss + scene.reg_loss(rendering)).backward()
    with torch.no_grad():
      scene.add_rendering(i, rendering)
      controller.add_rendering(i, rendering, progress)
    scene.step()
    controller.step(progress)
    if step % config.log_interval == 0:
      torch.cuda.synchronize()
      if t0 is None:
        t0, s0 = time.perf_counter(), step
      t1, s1 = time.perf_counter(), step
  return (s1 - s0) / (t1 - t0)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--quick", action="store_true")
  ap.add_argument("--json")
  args = ap.parse_args()
  result = dict(histograms=[], trainer={})
  for n in ((50_000,) if args.quick else (500_000, 3_000_000)):
    r = bench_histograms(n, 3 if args.quick else 7)
    result["histograms"].append(r)
    print(f"histograms of one log_details step, N = {n}: native {r['native_ms'][0]} [{r['native_ms'][1]}, {r['native_ms'][2]}] ms, "
          f"torch form {r['torch_ms'][0]} [{r['torch_ms'][1]}, {r['torch_ms'][2]}] ms, "
          f"{r['torch_ms'][0] / r['native_ms'][0]:.1f}x {'(clear)' if r['clear'] else '(NOT clear: the spreads overlap)'}", flush=True)
    print(f"  launches native {r['native_launches']} / torch {r['torch_launches']}; host waits native {r['native_waits']} / "
          f"torch {r['torch_waits']}; device time native {r['native_device_ms']} ms / torch {r['torch_device_ms']} ms; native "
          f"sweeps read {r['native_read_gb']} GB -> {r['native_gb_per_s']} GB/s", flush=True)
  points, w, h, cameras, steps = (2000, 96, 64, 6, 60) if args.quick else (20000, 320, 240, 8, 300)
  dataset = make_dataset(points, w, h, cameras)
  with tempfile.TemporaryDirectory() as out:
    trainer_rate(dataset, 30, out)                                          # warm-up
    rates = dict(trainer=[], hand=[])
    for _ in range(5):
      rates["trainer"].append(round(trainer_rate(dataset, steps, out), 2))
      rates["hand"].append(round(hand_rate(dataset, steps, out), 2))
  result["trainer"] = dict(points=points, image=[w, h], cameras=cameras, steps=steps, **rates)
  inside = sorted(rates["trainer"])[2] >= min(rates["hand"])
  print(f"Trainer.train, log_details=False, {points} points, {w}x{h}, {steps} steps: steps/s trainer {rates['trainer']} "
        f"(spread [{min(rates['trainer'])}, {max(rates['trainer'])}]), hand-written loop {rates['hand']} "
        f"(spread [{min(rates['hand'])}, {max(rates['hand'])}]): the trainer's median is "
        f"{'inside' if inside else 'BELOW'} the hand-written loop's spread", flush=True)
  if args.json:
    with open(args.json, "w") as f:
      json.dump(result, f, indent=1)


if __name__ == "__main__":
  main()
