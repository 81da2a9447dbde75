"""Times the area resize and ``COLMAPDataset.load_images`` on the GPU.

    python tools/dataset_bench.py [--images 32] [--json out.json]

resize        ``gsr_image_resize_area_u8`` alone on B = 8 images of 4032 x 3024 x 3 (293 MB: past the 256 MiB Infinity
              Cache) to scale 0.5, scale 0.25 and ``resize_longest=1600``, beside the torch form on the same GPU: uint8
              -> float, ``F.interpolate(mode="area")``, round, -> uint8.  Device events around CALLS calls enqueued back
              to back, the two forms alternated, median and [min, max] over the repetitions (tools/timing.py's loop: 3
              warm-up calls per form, REPS repetitions of CALLS calls per window, fixed order, a fresh event pair per
              window, lower median).  ``GBps`` is (bytes read +
              bytes written) of the uint8 tensors over that time -- for the torch form too, so it is the rate at which it
              does the same job, not its own traffic -- and ``hbm_share`` is that over the 6.29 TB/s a float4 copy
              reaches on this GPU.  ``differing_bytes`` counts where the float form is not the exact mean rounded half up.
load_images   a generated directory of JPEGs of that size with a one-camera model: the decode alone (the dataset's own
              pool and ``_decode``), then ``load_images()`` at ``image_scale=0.5`` on the device and through the host
              fallback, host clock around each.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from multiprocessing.pool import ThreadPool
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import colmap, colmap_io  # noqa: E402
from timing import repetitions  # noqa: E402

W, H, B = 4032, 3024, 8
HBM_COPY_TBPS = 6.29
CALLS, REPS = 10, 5


def torch_area(src: torch.Tensor, size) -> torch.Tensor:
  x = F.interpolate(src.permute(0, 3, 1, 2).to(torch.float32), size=size, mode="area")
  return x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def stats(times):
  times = sorted(times)
  return dict(median=round(times[len(times) // 2], 4), range=[round(times[0], 4), round(times[-1], 4)])


def bench_resize():
  g = torch.Generator().manual_seed(0)
  src = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
  rows = []
  s = 1600 / max(W, H)
  for label, (hd, wd) in (("scale 0.5", (H // 2, W // 2)), ("scale 0.25", (H // 4, W // 4)),
                          ("resize_longest 1600", (round(H * s), round(W * s)))):
    forms = (("native", lambda: sta.resize_area(src, (hd, wd))), ("torch", lambda: torch_area(src, (hd, wd))))
    differing = int((forms[0][1]() != forms[1][1]()).sum())
    ms = repetitions(forms, REPS, warmup=3, warmup_form="per_form", calls=CALLS, fresh_events=True)
    moved = B * 3 * (H * W + hd * wd)
    r = dict(case=f"resize {B} x {W}x{H}x3 -> {wd}x{hd} ({label})", bytes_read_plus_written=moved, differing_bytes=differing,
             differing_share=round(differing / (B * 3 * hd * wd), 6))
    for name, _ in forms:
      r[f"{name}_ms"] = stats(ms[name])
      r[f"{name}_GBps"] = round(moved / (r[f"{name}_ms"]["median"] * 1e-3) / 1e9, 1)
    r["native_hbm_share"] = round(r["native_GBps"] / (HBM_COPY_TBPS * 1e3), 3)
    r["speedup"] = round(r["torch_ms"]["median"] / r["native_ms"]["median"], 2)
    r["native_no_slower"] = r["native_ms"]["median"] <= r["torch_ms"]["median"]
    rows.append(r)
  return rows


def make_directory(path: Path, n: int):
  from PIL import Image
  rng = np.random.default_rng(0)
  yy, xx = np.mgrid[0:H, 0:W]
  base = 127 + 100 * np.sin(xx / 40.0) * np.cos(yy / 55.0)
  first = np.clip(base[..., None] + rng.normal(0, 12, size=(H, W, 3)), 0, 255).astype(np.uint8)
  (path / "images").mkdir(parents=True)
  images = []
  for k in range(n):
    Image.fromarray(np.roll(first, 37 * k, axis=1)).save(path / "images" / f"{k:03d}.jpg", quality=90)
    images.append(colmap_io.Image(k + 1, np.array([1.0, 0, 0, 0]), np.array([0.1 * k, 0, 0]), 1, f"{k:03d}.jpg"))
  cameras = {1: colmap_io.Camera("PINHOLE", W, H, np.array([3000.0, 3000.0, W / 2, H / 2]))}
  colmap_io.write_model(path / "sparse" / "0", cameras, images, None)


def bench_load(n: int):
  with tempfile.TemporaryDirectory() as tmp:
    path = Path(tmp)
    make_directory(path, n)
    ds = sta.COLMAPDataset(path, image_scale=0.5, device="cuda")
    t0 = time.perf_counter()
    with ThreadPool(processes=colmap.decode_threads()) as pool:
      pool.map(ds._decode, range(n))
    decode = time.perf_counter() - t0
    out = {}
    for name, kw in (("native", dict(device="cuda")), ("native_resident", dict(device="cuda", resident=True)),
                     ("host_fallback", dict(device="cpu"))):
      ds = sta.COLMAPDataset(path, image_scale=0.5, **kw)
      t0 = time.perf_counter()
      views = ds.load_images()
      torch.cuda.synchronize()
      out[name] = (time.perf_counter() - t0, views)
    same = all(torch.equal(a.image, b.image) for a, b in zip(out["native"][1], out["host_fallback"][1]))
    r = dict(case=f"load_images: {n} JPEGs of {W}x{H} at image_scale=0.5", decode_threads=colmap.decode_threads(),
             decode_only_s=round(decode, 3), same_bytes=same)
    for name, (seconds, _) in out.items():
      r[f"{name}_s"] = round(seconds, 3)
      r[f"{name}_less_decode_s"] = round(seconds - decode, 3)
    return [r]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--images", type=int, default=32)
  ap.add_argument("--json", default=None)
  ap.add_argument("--size", default=None, help="WxH of the images, for a rehearsal (default 4032x3024)")
  args = ap.parse_args()
  if args.size:
    global W, H
    W, H = (int(v) for v in args.size.split("x"))
  if not torch.cuda.is_available():
    raise SystemExit("dataset_bench needs a GPU: nothing here is a measurement without one")
  torch.cuda.set_device(0)
  rows = bench_resize() + bench_load(args.images)
  for r in rows:
    print(json.dumps(r), flush=True)
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
