"""Times the normal-consistency kernels on the GPU, each beside a torch form written here, and what the regulariser adds
to a training step.

    python tools/normals_bench.py [--json out.json] [--size WxH] [--points N]

kernels   The three kernel pairs at 1920 x 1080 and M = 500 000 visible rows, forward + backward of one autograd node:
          ``splat_normals`` (backward of sum(n g)), ``depth_normals`` (forward only) and ``normal_consistency_loss``
          (backward of L).  The torch forms are the contract's formulas in fp32 torch on the same GPU: quaternion to
          matrix, ``gather`` of the thin column, ``cross`` / ``norm`` / ``where`` over shifted views of the image, with
          autograd for the backward.  ``max_diff`` is the largest difference between the two forms' results.
          ``gb_per_s`` is the paper estimate of the native pair's traffic over its time.
step      One render + loss + backward of synthetic.scene_a(500 000, 1920 x 1080) through ``project_to_image`` and
          ``render_projected`` with a photometric loss ((image - 0.5)^2 mean): C = 3 as today, and C = 8 with
          ``geometry_features`` behind the colour and ``normal_consistency_loss`` added.  The difference is what switching
          the regulariser on costs per step.

tools/timing.py's loop: 3 warm-up calls per form, REPS repetitions of one window per form, 5 calls per window (2 for the
steps), fixed order, device events; lower median and [min, max].  No speed-up is asserted: the tool prints both times and
their ratio.
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
from splat_trainer_amd import synthetic  # noqa: E402
from timing import comparison_row, lower_median, repetitions, spread  # noqa: E402

REPS = 7
ALPHA_MIN = 0.5


# ---- the torch forms ---------------------------------------------------------------------------------------------------
def torch_splat_normals(rotation, log_scaling, position, indexes, T):
  q = rotation[indexes]
  q = q / q.norm(dim=-1, keepdim=True)
  x, y, z, w = q.unbind(-1)
  R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                   2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                   2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
  k = log_scaling[indexes].argmin(dim=1)
  col = R.gather(2, k[:, None, None].expand(-1, 3, 1)).squeeze(2)
  n = col @ T[:3, :3].t()
  p = position[indexes] @ T[:3, :3].t() + T[:3, 3]
  return torch.where(((n.detach() * p).sum(1) > 0)[:, None], -n, n)


def torch_depth_normals(depth, projection):
  H, W = depth.shape
  fx, fy, cx, cy = projection.unbind(0)
  u = (torch.arange(W, dtype=torch.float32, device=depth.device) + 0.5 - cx) / fx
  v = (torch.arange(H, dtype=torch.float32, device=depth.device) + 0.5 - cy) / fy
  ok = torch.isfinite(depth) & (depth > 0)
  safe = torch.where(ok, depth, torch.ones_like(depth))
  P = torch.stack([u[None, :] * safe, v[:, None] * safe, safe], -1)
  a = P[1:-1, 2:] - P[1:-1, :-2]
  b = P[2:, 1:-1] - P[:-2, 1:-1]
  c = torch.cross(b, a, dim=-1)
  ln = c.norm(dim=-1)
  inner = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1] & (ln > 0)
  unit = c / torch.where(inner, ln, torch.ones_like(ln))[..., None]
  n = torch.nn.functional.pad(torch.where(inner[..., None], unit, torch.zeros_like(unit)), (0, 0, 1, 1, 1, 1))
  return n, torch.nn.functional.pad(inner, (1, 1, 1, 1))


def torch_normal_loss(G, projection, alpha_min=ALPHA_MIN):
  D, A = G[..., 3], G[..., 4]
  seen = A >= alpha_min
  d = torch.where(seen, D / torch.where(seen, A, torch.ones_like(A)), torch.zeros_like(D))
  n_d, valid = torch_depth_normals(d, projection)
  per_pixel = A - (G[..., :3] * n_d).sum(-1)
  return torch.where(valid, per_pixel, torch.zeros_like(per_pixel)).sum() / (G.shape[0] * G.shape[1])


# ---- the measurements ----------------------------------------------------------------------------------------------------
def _row(name, times, native, torch_form, bytes_moved, max_diff):
  row = comparison_row(name, times[native], times[torch_form])
  row.update(gb_per_s=round(bytes_moved / (lower_median(times[native]) * 1e-3) / 1e9, 1), max_diff=float(max_diff))
  return row


def kernels(W, H, M):
  gen = torch.Generator(device="cuda").manual_seed(0)
  rand = lambda *s: torch.rand(*s, device="cuda", generator=gen)                      # noqa: E731
  N = 2 * M
  rotation = (rand(N, 4) - 0.5).requires_grad_(True)
  g = sta.Gaussians3D(position=4 * rand(N, 3) - 2, rotation=rotation, log_scaling=rand(N, 3) - 3,
                      alpha_logit=rand(N, 1), feature=rand(N, 1))
  indexes = torch.arange(0, N, 2, device="cuda")
  focal = 1100.0 / 1920.0 * W
  projection = torch.tensor([focal, focal, W / 2, H / 2], device="cuda")
  T = torch.eye(4, device="cuda")
  T[:3, 3] = torch.tensor([0.1, 0.2, 5.0])
  camera = sta.CameraParams(T_camera_world=T, projection=projection, image_size=(W, H))
  g_n = rand(M, 3)
  depth = 2.0 + rand(H, W) + 0.002 * torch.arange(W, device="cuda")[None, :]
  A = torch.where(rand(H, W) < 0.25, 0.05 + 0.39 * rand(H, W), 0.56 + 0.44 * rand(H, W))
  G = torch.cat([2 * rand(H, W, 3) - 1, (depth * A)[..., None], A[..., None]], -1).requires_grad_(True)

  def grad_of(fn, leaf):
    leaf.grad = None
    out = fn()
    out.backward()
    return leaf.grad

  forms = {
      "splat native": lambda: grad_of(lambda: (sta.splat_normals(g, indexes, camera) * g_n).sum(), rotation),
      "splat torch": lambda: grad_of(lambda: (torch_splat_normals(rotation, g.log_scaling, g.position, indexes, T) * g_n).sum(),
                                     rotation),
      "depth native": lambda: sta.depth_normals(depth, projection),
      "depth torch": lambda: torch_depth_normals(depth, projection)[0],
      "loss native": lambda: grad_of(lambda: sta.normal_consistency_loss(G, projection, ALPHA_MIN), G),
      "loss torch": lambda: grad_of(lambda: torch_normal_loss(G, projection), G),
  }
  diffs = {}
  with torch.no_grad():
    diffs["splat"] = (sta.splat_normals(g, indexes, camera) -
                      torch_splat_normals(rotation, g.log_scaling, g.position, indexes, T)).abs().max().item()
    diffs["depth"] = (forms["depth native"]() - forms["depth torch"]()).abs().max().item()
  diffs["loss"] = (forms["loss native"]().clone() - forms["loss torch"]()).abs().max().item()
  times = repetitions(forms, REPS, 3, calls=5)
  P = W * H
  return [
      # forward: index 8, rotation 16, scales 12, position 12, out 12; backward: the same inputs + g 12, d_rotation 16 + its zero fill
      _row(f"splat_normals fwd+bwd M={M}", times, "splat native", "splat torch", M * (60 + 76) + N * 16, diffs["splat"]),
      _row(f"depth_normals {W}x{H}", times, "depth native", "depth torch", P * 16, diffs["depth"]),
      # forward: G 20, n_d 12; backward: G 20, d_G 20
      _row(f"normal_consistency_loss fwd+bwd {W}x{H}", times, "loss native", "loss torch", P * 72, diffs["loss"]),
  ]


def step(W, H, points):
  scene, cam = synthetic.scene_a(points, W, H, sh_degree=0, seed=0)
  camd = cam.to("cuda")
  gd = sta.Gaussians3D(*(t.cuda().requires_grad_(True) for t in (scene.position, scene.rotation, scene.log_scaling,
                                                                  scene.alpha_logit, scene.feature)))
  cfg = sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True)
  colour = None

  def one(geometry: bool):
    nonlocal colour
    for t in (gd.position, gd.rotation, gd.log_scaling, gd.alpha_logit):
      t.grad = None
    g2d, depth, idx = sta.project_to_image(gd, camd, cfg)
    if colour is None or colour.shape[0] != idx.shape[0]:
      colour = torch.rand(idx.shape[0], 3, device="cuda")
    feats = torch.cat([colour, sta.geometry_features(gd, idx, depth, camd)], 1) if geometry else colour
    r = sta.render_projected(idx, g2d, feats, depth, camd, cfg)
    loss = ((r.image[..., :3] - 0.5) ** 2).mean()
    if geometry:
      loss = loss + 0.05 * sta.normal_consistency_loss(r.image[..., 3:8], camd.projection, ALPHA_MIN)
    loss.backward()
    return idx.shape[0]

  visible = one(False)
  times = repetitions({"C=3": lambda: one(False), "C=8 + normal loss": lambda: one(True)}, REPS, 2, calls=2)
  plain, geo = lower_median(times["C=3"]), lower_median(times["C=8 + normal loss"])
  return dict(case=f"step {points} splats {W}x{H}, {visible} visible", c3_ms=round(plain, 3),
              c3_range=[round(t, 3) for t in spread(times["C=3"])], c8_normal_ms=round(geo, 3),
              c8_normal_range=[round(t, 3) for t in spread(times["C=8 + normal loss"])],
              added_ms=round(geo - plain, 3), ratio=round(geo / plain, 3))


def main():
  ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
  ap.add_argument("--json")
  ap.add_argument("--size", default="1920x1080")
  ap.add_argument("--points", type=int, default=500_000)
  args = ap.parse_args()
  W, H = (int(v) for v in args.size.split("x"))
  rows = kernels(W, H, args.points)
  for row in rows:
    print(json.dumps(row), flush=True)
  cost = step(W, H, args.points)
  print(json.dumps(cost), flush=True)
  if args.json:
    with open(args.json, "w") as f:
      json.dump(dict(kernels=rows, step=cost), f, indent=1)


if __name__ == "__main__":
  main()
