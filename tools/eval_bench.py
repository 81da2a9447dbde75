"""Evaluation pass at 1080p: ``Evaluation.metrics`` and ``color_corrected()`` of splat_trainer_amd.evaluation against the
torch form the reference runs (trainer/evaluation.py, util/colors.py), written out here.  Reports ms per image.

    python tools/eval_bench.py [--height 1080 --width 1920 --repeats 5]

Each figure is the median over ``--repeats`` images of the wall time from the call to the values being on the host (the
metrics are read back, the corrected image is synchronised), after one warm-up image (tools/timing.py's loop: each form
alone, 1 warm-up call, --repeats repetitions of one call, host clock, the mean-of-middles median).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import splat_trainer_amd as sta  # noqa: E402
from timing import HostClock, mid_median, repetitions  # noqa: E402


def torch_metrics(image, source):
  """The reference's three properties: three reductions, three .item() waits."""
  psnr = (10 * torch.log10(1 / torch.nn.functional.mse_loss(image, source))).item()
  l1 = torch.nn.functional.l1_loss(image, source).item()
  ref = source.unsqueeze(0).permute(0, 3, 1, 2).to(memory_format=torch.channels_last)
  pred = image.unsqueeze(0).permute(0, 3, 1, 2).to(memory_format=torch.channels_last)
  return dict(psnr=psnr, l1=l1, ssim=sta.fused_ssim(pred, ref, padding="valid").item())


def torch_fit_colors(img, ref, num_iters=5, eps=0.5 / 255):
  """The iterative fit as torch ops: a (pixels x 10) design matrix and three lstsq solves per iteration."""
  x0 = img.reshape(-1, 3)
  r = ref.reshape(-1, 3)
  ok = lambda z: (z >= eps) & (z <= 1 - eps)
  mask0, x = ok(x0), x0
  for _ in range(num_iters):
    a = torch.cat([x[:, c:c + 1] * x[:, c:] for c in range(3)] + [x, torch.ones_like(x[:, :1])], dim=-1)
    warp = []
    for c in range(3):
      m = mask0[:, c] & ok(x[:, c]) & ok(r[:, c])
      warp.append(torch.linalg.lstsq(torch.where(m[:, None], a, torch.zeros_like(a)),
                                     torch.where(m, r[:, c], torch.zeros_like(r[:, c])), rcond=-1)[0])
    x = torch.clip(a @ torch.stack(warp, dim=-1), 0, 1)
  return x.reshape(img.shape)


def timed(fn, repeats):
  return mid_median(repetitions({"fn": fn}, repeats, warmup=1, clock=HostClock())["fn"])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--height", type=int, default=1080)
  ap.add_argument("--width", type=int, default=1920)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--skip-torch-fit", action="store_true")
  args = ap.parse_args()
  gen = torch.Generator(device="cuda").manual_seed(0)
  H, W = args.height, args.width
  yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
  base = torch.stack([0.5 + 0.6 * torch.sin(xx / 97.0 + k) * torch.cos(yy / 61.0 + 2 * k) for k in range(3)], dim=2)
  image = (base + 0.05 * torch.randn(H, W, 3, device="cuda", generator=gen)).clamp(0, 1).contiguous()
  matrix = torch.eye(3, device="cuda") + 0.1 * torch.randn(3, 3, device="cuda", generator=gen)
  source = ((image ** 1.15) @ matrix + 0.02 + 0.01 * torch.randn(H, W, 3, device="cuda", generator=gen)).clamp(0, 1).contiguous()
  rendering = sta.Rendering(image=image, camera=None, points=None)

  out = dict(height=H, width=W, repeats=args.repeats)
  out["metrics_native_ms"] = timed(lambda: sta.Evaluation("a", rendering, source).metrics, args.repeats)
  out["metrics_torch_ms"] = timed(lambda: torch_metrics(image, source), args.repeats)
  out["color_fit_native_ms"] = timed(lambda: sta.fit_colors(image, source), args.repeats)
  out["color_corrected_metrics_native_ms"] = timed(lambda: sta.Evaluation("a", rendering, source).color_corrected().metrics,
                                                   args.repeats)
  native = sta.fit_colors(image, source)
  print(json.dumps(dict(out, partial="native only")), flush=True)
  if not args.skip_torch_fit:
    out["color_fit_torch_ms"] = timed(lambda: torch_fit_colors(image, source), args.repeats)
    out["max_abs_native_minus_torch"] = (native - torch_fit_colors(image, source)).abs().max().item()
  ev = sta.Evaluation("a", rendering, source)
  out["psnr"], out["psnr_color_corrected"] = ev.psnr, ev.color_corrected().psnr
  print(json.dumps(out))


if __name__ == "__main__":
  main()
