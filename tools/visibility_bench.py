"""Times the visibility kernels (splat_trainer_amd.visibility) against the torch form of the reference they replace, on
the same GPU in the same process: the two are alternated repetition by repetition after a warm-up, timed with device
events, and reported as median and [min, max] over the repetitions.  The loop is tools/timing.py's: 2 interleaved
warm-up rounds, 5 to 9 repetitions, one call per window, fixed order, one reused event pair, lower median.

    python tools/visibility_bench.py [--quick] [--json out.json]

frustum counts   native ``frustum_counts`` (both outputs, one pass) against the reference's loop over the cameras
                 (query_points.py:73-102: homogeneous copy, 4x4 product, division, six comparisons, an indexed increment
                 and a mask sum per camera) -- with the projection shared between the two outputs, which favours torch;
view features    native ``PointClusters.view_features`` against cluster.py:36-47 (mask, three gathers, scatter_add_).

A native call counts as faster only when its slowest repetition beats torch's fastest (``clear``).
Issue bound of the frustum test: 256 CUs x 4 SIMDs x 16 lanes per cycle at 2.4 GHz (full-rate fp32), at the VALU
operations per pair counted in the gfx950 code of the inner loop.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from splat_trainer_amd import visibility as vis  # noqa: E402
from timing import comparison_row, lower_median, repetitions  # noqa: E402

ISSUE_BOUND = 256 * 4 * 16 * 2.4e9
FRUSTUM_OPS = 25            # 9 v_fma, 2 v_mul, 6 v_cmp, the count select / add and the ballot's share, per pair


def ring(V, device="cuda"):
  ctw = torch.zeros(V, 4, 4)
  for i in range(V):
    a = 2 * math.pi * i / V
    c = torch.tensor([6 * math.cos(a), 0.0, 6 * math.sin(a)])
    z = -c / c.norm()
    x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), z)
    x = x / x.norm()
    R = torch.stack([x, torch.linalg.cross(z, x), z])
    ctw[i, :3, :3], ctw[i, :3, 3], ctw[i, 3, 3] = R, -R @ c, 1
  f = 400 + 300 * torch.rand(V, generator=torch.Generator().manual_seed(0))
  intr = torch.stack([f, f, torch.full((V,), 320.0), torch.full((V,), 240.0)], 1)
  return vis.CameraBatch(ctw.to(device), intr.to(device), torch.tensor([[640, 480]] * V, device=device),
                         torch.tensor([[0.1, 100.0]] * V, device=device))


def torch_frustum(image_t_world, sizes, ranges, points):
  homog = torch.cat([points, torch.ones_like(points[:, :1])], dim=-1)
  vis_counts = torch.zeros(points.shape[0], dtype=torch.int32, device=points.device)
  cam_counts = torch.zeros(image_t_world.shape[0], dtype=torch.int32, device=points.device)
  for i in range(image_t_world.shape[0]):
    proj = (image_t_world[i].reshape(-1, 4, 4) @ homog.reshape(-1, 4, 1))[..., 0].reshape(-1, 4)
    depth = proj[..., 2]
    xy = proj[..., :2] / depth.unsqueeze(-1)
    (w, h), (near, far) = sizes[i], ranges[i]
    mask = ((xy[..., 0] >= 0) & (xy[..., 0] < w) & (xy[..., 1] >= 0) & (xy[..., 1] < h) & (depth > near) & (depth < far))
    vis_counts[mask] += 1
    cam_counts[i] = mask.sum()
  return vis_counts, cam_counts


def torch_view_features(labels, K, idx, v, threshold=0.01):
  vector = torch.zeros(K, device=labels.device)
  mask = v > threshold
  vector.scatter_add_(0, labels[idx[mask]], v[mask])
  return vector


def measure(native, reference, reps):
  ms = repetitions((("native", native), ("torch", reference)), reps, warmup=2)
  return ms["native"], ms["torch"]


def row(name, native, reference, pairs=None, ops=None):
  r = comparison_row(name, native, reference)
  if pairs:
    r["pairs_per_s"] = pairs / (lower_median(native) * 1e-3)
    r["valu_issue_share"] = round((pairs * ops / ISSUE_BOUND) / (lower_median(native) * 1e-3), 3)
  return r


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--quick", action="store_true", help="small sizes (a functional run)")
  ap.add_argument("--json", default=None)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  rows = []
  g = torch.Generator().manual_seed(0)
  sizes_n = (50_000, 200_000) if args.quick else (500_000, 3_000_000)
  cams_v = (8, 32) if args.quick else (64, 256)
  for N in sizes_n:
    points = (torch.randn(N, 3, generator=g) * torch.tensor([3.0, 1.5, 3.0])).cuda()
    for V in cams_v:
      cams = ring(V)
      cams.records()
      m, sizes, ranges = cams.image_t_world(), cams.image_sizes.tolist(), cams.depth_ranges.tolist()
      native, reference = measure(lambda: vis.frustum_counts(cams, points),
                                  lambda: torch_frustum(m, sizes, ranges, points), reps=7 if V <= 64 else 5)
      rows.append(row(f"frustum_counts N={N} V={V}", native, reference, N * V, FRUSTUM_OPS))
  N, K = sizes_n[1], 1024                       # the reference's default vis_clusters (config/trainer/default.yaml)
  labels = torch.randint(0, K, (N,), generator=g).cuda()
  clusters = vis.PointClusters(labels, torch.zeros(K, 3, device="cuda"))
  for M in sizes_n:
    idx = torch.randperm(N, generator=g)[:M].cuda()
    v = (torch.rand(M, generator=g) ** 3).cuda()
    native, reference = measure(lambda: clusters.view_features(idx, v),
                                lambda: torch_view_features(labels, K, idx, v), reps=9)
    rows.append(row(f"view_features N={N} M={M} K={K}", native, reference))
  for r in rows:
    print(json.dumps(r))
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
