"""Times the depth fusion's two hot paths on the GPU, each beside a torch form written here.

    python tools/fusion_bench.py [--json out.json] [--size WxH] [--points N]

consistency  ``depth_consistency`` of one 1920 x 1080 reference depth map against 8 sources of the same size: a plane
             at z = 4 with 2 % of the pixels displaced, cameras of identity rotation shifted along x.  The torch form
             does the contract's arithmetic in float64 tensors -- unproject, transform, project, floor, a ``gather`` for
             the source depth, the two comparisons -- source after source, and sums the votes.  ``differing`` counts the
             counters that differ between the two (the torch form is free to contract and to divide as it likes).
             The cameras are on the device, so both forms read them back once per call (``fusion.read_cameras``);
             ``native_host_cameras_ms`` is the native form handed ``HostCamera`` records, as ``fuse_depth_maps`` hands
             them down: no read at all, the zero-fill of the counters and the launch.
voxel        ``voxel_downsample`` of 20 M points (normal, sigma 2, voxel 0.05) with colours.  The torch form computes
             the cell indexes in float64, packs the key, and reduces with ``torch.unique(return_inverse, return_counts)``
             and ``index_add_`` of float64 positions and colours; its sums are float atomics, so its means are not
             reproducible, and ``max_abs_difference`` is what separates it from the native result.

tools/timing.py's loop: 2 warm-up calls per form, REPS repetitions of one window per form, 5 calls per window (1 for
the voxel case), fixed order, the host clock (``perf_counter`` around a window that ends in a synchronise: both forms
read a count back), lower median and [min, max].  No speed-up is asserted: the tool prints both times and their ratio.
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
from splat_trainer_amd import fusion  # noqa: E402
from timing import HostClock, comparison_row, lower_median, repetitions  # noqa: E402

W, H, SOURCES, POINTS = 1920, 1080, 8, 20_000_000
REL_TOL, VOXEL = 0.01, 0.05
REPS = 5


def views():
  """(depth maps, cameras): view 0 is the reference."""
  g = torch.Generator().manual_seed(0)
  depths, cameras = [], []
  for v in range(SOURCES + 1):
    d = torch.full((H, W), 4.0)
    odd = torch.rand(H, W, generator=g) < 0.02
    d[odd] = 4.0 + (torch.rand(int(odd.sum()), generator=g) - 0.5)
    T = torch.eye(4)
    T[0, 3] = -0.125 * ((v + 1) // 2) * (1 if v % 2 else -1)
    cameras.append(sta.CameraParams(T_camera_world=T.cuda(), projection=torch.tensor([1600.0, 1600.0, W / 2, H / 2]).cuda(),
                                    image_size=(W, H)))
    depths.append(d.cuda())
  return depths, cameras


def torch_consistency(ref, ref_camera, sources, rel_tol):
  """The contract of gsr_fuse_check in float64 tensors with a gather for the lookup: uint8 (H, W, 2)."""
  views = fusion.read_cameras([ref_camera] + [camera for _, camera in sources])      # one host read, as the native form
  fx, fy, cx, cy = (float(v) for v in views[0].intrinsics)
  h, w = ref.shape
  d = ref.to(torch.float64)
  j = torch.arange(w, dtype=torch.float64, device=ref.device)[None, :] + 0.5
  i = torch.arange(h, dtype=torch.float64, device=ref.device)[:, None] + 0.5
  X, Y = (j - cx) / fx * d, (i - cy) / fy * d
  ok0 = (d > 0) & torch.isfinite(d)
  world_t_ref = fusion.rigid_inverse(views[0].pose)
  agree = torch.zeros((h, w), dtype=torch.int32, device=ref.device)
  violate = torch.zeros_like(agree)
  for (depth, _), camera in zip(sources, views[1:]):
    r = fusion.compose(camera.pose, world_t_ref)
    sfx, sfy, scx, scy = (float(v) for v in camera.intrinsics)
    hs, ws = depth.shape
    p = [r[k, 0] * X + r[k, 1] * Y + r[k, 2] * d + r[k, 3] for k in range(3)]
    ok = ok0 & (p[2] > camera.near)
    us, vs = sfx * (p[0] / p[2]) + scx, sfy * (p[1] / p[2]) + scy
    ok = ok & (us >= 0) & (us < ws) & (vs >= 0) & (vs < hs)
    at = torch.where(ok, vs.floor() * ws + us.floor(), torch.zeros_like(us)).to(torch.int64)
    ds = torch.gather(depth.reshape(-1), 0, at.reshape(-1)).reshape(h, w).to(torch.float64)
    ok = ok & (ds > 0) & torch.isfinite(ds)
    tol, diff = rel_tol * p[2], ds - p[2]
    a = ok & (diff.abs() <= tol)
    agree += a
    violate += ok & ~a & (diff > tol)
  return torch.stack([agree, violate], -1).clamp(max=255).to(torch.uint8)


def torch_voxel(points, colors, voxel):
  """Mean position and colour per occupied voxel with torch.unique and index_add_: (points, colours, counts)."""
  s = points.to(torch.float64) / voxel
  q = s.floor().clamp(-(1 << 20), (1 << 20) - 1).to(torch.int64) + (1 << 20)
  key = (q[:, 2] << 42) | (q[:, 1] << 21) | q[:, 0]
  _, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
  K = counts.shape[0]
  sums = torch.zeros((K, 6), dtype=torch.float64, device=points.device)
  sums.index_add_(0, inverse, torch.cat([points.to(torch.float64), colors.to(torch.float64)], 1))
  mean = sums / counts[:, None]
  return mean[:, :3].to(torch.float32), (mean[:, 3:] + 0.5).floor().to(torch.uint8), counts.to(torch.int32)


def bench_consistency():
  depths, cameras = views()
  sources = list(zip(depths[1:], cameras[1:]))
  on_host = fusion.read_cameras(cameras)
  host_sources = list(zip(depths[1:], on_host[1:]))
  forms = (("native", lambda: sta.depth_consistency(depths[0], cameras[0], sources, REL_TOL)),
           ("torch", lambda: torch_consistency(depths[0], cameras[0], sources, REL_TOL)),
           ("native_host_cameras", lambda: sta.depth_consistency(depths[0], on_host[0], host_sources, REL_TOL)))
  a, b = forms[0][1](), forms[1][1]()
  differing = int((a != b).sum())
  votes = [int(a[:, :, 0].sum()), int(a[:, :, 1].sum())]
  del a, b
  ms = repetitions(forms, REPS, warmup=2, warmup_form="per_form", calls=5, clock=HostClock())
  row = comparison_row(f"consistency {W}x{H} against {SOURCES} sources", ms["native"], ms["torch"])
  return dict(row, native_host_cameras_ms=round(lower_median(ms["native_host_cameras"]), 4), agree_votes=votes[0],
              violate_votes=votes[1], differing=differing)


def bench_voxel():
  g = torch.Generator().manual_seed(1)
  points = (2.0 * torch.randn(POINTS, 3, generator=g)).cuda()
  colors = torch.randint(0, 256, (POINTS, 3), dtype=torch.uint8, generator=g).cuda()
  forms = (("native", lambda: sta.voxel_downsample(points, colors, VOXEL)), ("torch", lambda: torch_voxel(points, colors, VOXEL)))
  a, b = forms[0][1](), forms[1][1]()
  same_cells = a[0].shape == b[0].shape and bool((a[2] == b[2]).all())
  largest = float((a[0].double() - b[0].double()).abs().max()) if same_cells else None
  voxels = int(a[0].shape[0])
  del a, b
  ms = repetitions(forms, REPS, warmup=2, warmup_form="per_form", calls=1, clock=HostClock())
  row = comparison_row(f"voxel_downsample of {POINTS} points at {VOXEL}", ms["native"], ms["torch"], digits=(3, 3))
  return dict(row, voxels=voxels, same_cells_and_counts=same_cells, max_abs_difference=largest)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--json", default=None)
  ap.add_argument("--size", default=None, help="WxH of the depth maps, for a rehearsal (default 1920x1080)")
  ap.add_argument("--points", type=int, default=None, help="points of the voxel case, for a rehearsal (default 20 M)")
  args = ap.parse_args()
  global W, H, POINTS
  if args.size:
    W, H = (int(v) for v in args.size.split("x"))
  if args.points:
    POINTS = args.points
  if not torch.cuda.is_available():
    raise SystemExit("fusion_bench needs a GPU: nothing here is a measurement without one")
  torch.cuda.set_device(0)
  rows = [bench_consistency(), bench_voxel()]
  for r in rows:
    print(json.dumps(r), flush=True)
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
