"""Times the lens undistortion on the GPU.

    python tools/undistort_bench.py [--json out.json] [--size WxH]

remap   ``gsr_image_remap_u8`` alone on B = 8 images of 4032 x 3024 x 3 through the barrel map of a 4032 x 3024 camera
        onto its optimal pinhole, beside the torch form on the same GPU: uint8 -> float, ``F.grid_sample(...,
        mode="bilinear", align_corners=True)`` on the unquantised grid, round, -> uint8.  Two source batches of 293 MB
        each (past the 256 MiB Infinity Cache) are taken in turn, so no call finds its source in the cache.  Device
        events around CALLS calls enqueued back to back, the two forms alternated, median and [min, max] over the
        repetitions (tools/timing.py's loop: 3 warm-up calls per form, REPS repetitions of CALLS calls per window,
        fixed order, a fresh event pair per window, lower median; a form is handed the call index).  ``GBps`` is
        (source bytes + map bytes + destination bytes) over that time -- for the torch form too, so it is the rate at which it does the same job, not its own traffic -- and ``hbm_share`` is that over the
        6.29 TB/s a float4 copy reaches on this GPU.  ``differing_bytes`` counts where the float form on the unquantised
        grid is not the fixed-point result, ``max_difference`` the largest such step.
map     ``gsr_undistort_map`` of that camera alone, the same way: 12.2 M entries of 8 bytes.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import splat_trainer_amd as sta  # noqa: E402
from timing import repetitions  # noqa: E402

W, H, B = 4032, 3024, 8
HBM_COPY_TBPS = 6.29
CALLS, REPS = 10, 5


def camera() -> sta.LensCamera:
  s = W / 4032
  return sta.LensCamera(W, H, 3000.0 * s, 3010.0 * s, 2010.3 * s, 1500.7 * s, k1=-0.12, k2=0.03, p1=0.0005, p2=-0.0007)


def float_grid(cam: sta.LensCamera, target) -> torch.Tensor:
  """The unquantised map as grid_sample's (1, H, W, 2) grid with align_corners=True: float32, on the device."""
  fx, fy, cx, cy = target
  v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device="cuda"), torch.arange(W, dtype=torch.float64, device="cuda"),
                        indexing="ij")
  x, y = (u - cx) / fx, (v - cy) / fy
  r2 = x * x + y * y
  rad = 1 + r2 * (cam.k1 + r2 * (cam.k2 + r2 * cam.k3))
  xs = cam.fx * (x * rad + 2 * cam.p1 * x * y + cam.p2 * (r2 + 2 * x * x)) + cam.cx
  ys = cam.fy * (y * rad + cam.p1 * (r2 + 2 * y * y) + 2 * cam.p2 * x * y) + cam.cy
  return torch.stack([xs / (W - 1) * 2 - 1, ys / (H - 1) * 2 - 1], dim=-1).to(torch.float32)[None]


def torch_remap(src: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
  x = F.grid_sample(src.permute(0, 3, 1, 2).to(torch.float32), grid.expand(src.shape[0], -1, -1, -1), mode="bilinear",
                    padding_mode="zeros", align_corners=True)
  return x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def stats(times):
  times = sorted(times)
  return dict(median=round(times[len(times) // 2], 4), range=[round(times[0], 4), round(times[-1], 4)])


def timed(forms):
  """forms: (name, fn(call index)) -> name -> per-call milliseconds of each repetition, the forms alternated."""
  return repetitions(forms, REPS, warmup=3, warmup_form="per_form", calls=CALLS, fresh_events=True)


def bench_remap(cam, und):
  g = torch.Generator().manual_seed(0)
  sources = [torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(2)]
  map_dev, grid = und.map_on("cuda"), float_grid(cam, und.target)
  forms = (("native", lambda k: sta.remap(sources[k & 1], map_dev)), ("torch", lambda k: torch_remap(sources[k & 1], grid)))
  a, b = forms[0][1](0), forms[1][1](0)
  differing = int((a != b).sum())
  largest = int((a.to(torch.int16) - b.to(torch.int16)).abs().max())
  del a, b
  ms = timed(forms)
  moved = B * 3 * H * W * 2 + 8 * H * W
  r = dict(case=f"remap {B} x {W}x{H}x3 through a barrel map", bytes_source_map_destination=moved, differing_bytes=differing,
           differing_share=round(differing / (B * 3 * H * W), 6), max_difference=largest)
  for name, _ in forms:
    r[f"{name}_ms"] = stats(ms[name])
    r[f"{name}_GBps"] = round(moved / (r[f"{name}_ms"]["median"] * 1e-3) / 1e9, 1)
  r["native_hbm_share"] = round(r["native_GBps"] / (HBM_COPY_TBPS * 1e3), 3)
  r["speedup"] = round(r["torch_ms"]["median"] / r["native_ms"]["median"], 2)
  r["native_faster"] = r["native_ms"]["median"] < r["torch_ms"]["median"]
  return r


def bench_map(cam, und):
  ms = timed((("native", lambda k: sta.undistort_map(cam, und.target, device="cuda")),))
  r = dict(case=f"map of a {W}x{H} camera", bytes_written=8 * H * W, native_ms=stats(ms["native"]))
  r["native_GBps"] = round(8 * H * W / (r["native_ms"]["median"] * 1e-3) / 1e9, 1)
  return r


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--json", default=None)
  ap.add_argument("--size", default=None, help="WxH of the images, for a rehearsal (default 4032x3024)")
  args = ap.parse_args()
  if args.size:
    global W, H
    W, H = (int(v) for v in args.size.split("x"))
  if not torch.cuda.is_available():
    raise SystemExit("undistort_bench needs a GPU: nothing here is a measurement without one")
  torch.cuda.set_device(0)
  cam = camera()
  und = sta.Undistortion(cam)
  rows = [dict(case="camera", camera=str(cam), optimal_pinhole=[round(v, 4) for v in und.target]),
          bench_remap(cam, und), bench_map(cam, und)]
  for r in rows:
    print(json.dumps(r), flush=True)
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
