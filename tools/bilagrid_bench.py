"""Cost of the bilateral-grid colour correction (csrc/bilagrid.hip, splat_trainer_amd.bilateral).

    python tools/bilagrid_bench.py [--parts slice,tv,c2] [--reps 30] [--warmup 5] [--only native|base|corrected]

  slice  native slice forward + backward (image and grid gradients) at 1920 x 1080 and 3840 x 2160, (16, 16, 8) grid,
         against the torch formulation (meshgrid, 5-D F.grid_sample, batched 3x4 matmul) on the same GPU
  tv     BilateralCorrector.step (TV value + gradient in one kernel call, Adam) for N = 100 and 300 grids, against the
         torch formulation (the reference's total_variation_loss, backward, Adam)
  c2     one-call c2 fwd+bwd steps (render_gaussians(use_sh=True) + clamped MSE + backward) without and with the corrector
         (correct + corrector.step), alternating in one process

Device-event timing, warm-up first, median of --reps (tools/timing.py's loop: --warmup interleaved rounds, one call per
window, the forms mirrored on odd repetitions, a fresh event pair per window, the mean-of-middles median).
``--only``: one variant alone, for a
`rocprofv3 --kernel-trace --stats -- python tools/bilagrid_bench.py --parts slice --only native --reps 5` run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import synthetic  # noqa: E402
from splat_trainer_amd.bilateral import BilateralCorrectorConfig  # noqa: E402
from timing import mid_median, repetitions  # noqa: E402


def timed(fns: dict, reps: int, warmup: int) -> dict:
  times = repetitions(fns, reps, warmup, order="mirrored", fresh_events=True)
  return {n: dict(median_ms=mid_median(t), min_ms=min(t)) for n, t in times.items()}


def torch_slice(grids, k, image):
  """The torch formulation of the reference's correct_grid (restated, float32)."""
  H, W = image.shape[0], image.shape[1]
  gy, gx = torch.meshgrid((torch.arange(H, device=image.device) + 0.5) / H,
                          (torch.arange(W, device=image.device) + 0.5) / W, indexing="ij")
  xy = torch.stack([gx, gy], dim=-1) * 2 - 1
  z = (image @ torch.tensor([0.299, 0.587, 0.114], device=image.device)).unsqueeze(-1) * 2 - 1
  coords = torch.cat([xy, z], dim=-1).view(1, 1, H, W, 3)
  A = F.grid_sample(grids[k:k + 1], coords, mode="bilinear", padding_mode="border", align_corners=True)
  A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
  return (A[..., :3] @ image.unsqueeze(-1)).squeeze(-1) + A[..., 3]


def torch_tv(x):
  tv = 0
  for i in range(2, 5):
    n = x.shape[i]
    tv = tv + (x.narrow(i, 1, n - 1) - x.narrow(i, 0, n - 1)).pow(2).sum() / (x.numel() // x.shape[0])
  return tv / x.shape[0]


def part_slice(reps, warmup, only):
  out = {}
  for W, H in ((1920, 1080), (3840, 2160)):
    gen = torch.Generator().manual_seed(0)
    grids = (torch.rand(4, 12, 8, 16, 16, generator=gen) * 0.2 - 0.1).cuda()
    grids += sta.BilateralGrid(1).grids.detach().cuda()
    grids.requires_grad_(True)
    image = torch.rand(H, W, 3, generator=gen).cuda().requires_grad_(True)
    go = torch.randn(H, W, 3, generator=gen).cuda()

    def native():
      sta.bilateral_correct(grids, 1, image).backward(go)
      grids.grad = image.grad = None

    def native_fwd():
      with torch.no_grad():
        sta.bilateral_correct(grids, 1, image)

    def ref():
      torch_slice(grids, 1, image).backward(go)
      grids.grad = image.grad = None

    fns = {"native": native, "native_forward": native_fwd, "torch": ref}
    if only:
      fns = {only: fns[only]}
    r = timed(fns, reps, warmup)
    if "torch" in r and "native" in r:
      r["speedup"] = r["torch"]["median_ms"] / r["native"]["median_ms"]
    out[f"{W}x{H}"] = r
    print(f"slice {W}x{H}: " + "  ".join(f"{k} {v['median_ms'] * 1000:.1f} us" for k, v in r.items() if isinstance(v, dict))
          + (f"  speedup {r['speedup']:.1f}x" if "speedup" in r else ""), flush=True)
  return out


def part_tv(reps, warmup, only):
  out = {}
  for N in (100, 300):
    corr = BilateralCorrectorConfig().make_corrector(N, "cuda")
    grids = corr.bil_grids.grids
    with torch.no_grad():
      grids.add_(0.01 * torch.randn_like(grids))
    ref_grids = grids.detach().clone().requires_grad_(True)
    ref_opt = torch.optim.Adam([ref_grids], lr=2e-4)

    def native():
      corr.step(0.5)

    def ref():
      (10.0 * torch_tv(ref_grids)).backward()
      ref_opt.step()
      ref_opt.zero_grad()

    fns = {"native": native, "torch": ref}
    if only:
      fns = {only: fns[only]}
    r = timed(fns, reps, warmup)
    out[f"N{N}"] = r
    print(f"tv + adam N={N}: " + "  ".join(f"{k} {v['median_ms'] * 1000:.1f} us" for k, v in r.items()), flush=True)
  return out


def part_c2(reps, warmup, only):
  g, cam = synthetic.scene_a(500_000, 1920, 1080, sh_degree=3, seed=0)
  cfg = sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True)
  params = [t.cuda().requires_grad_(True) for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)]
  gd = sta.Gaussians3D(*params)
  camd = cam.to("cuda")
  corr = BilateralCorrectorConfig().make_corrector(1, "cuda")

  def base():
    r = sta.render_gaussians(gd, camd, cfg, use_sh=True)
    ((r.image.clamp(0, 1) - 0.5) ** 2).mean().backward()
    for p in params:
      p.grad = None

  def corrected():
    r = sta.render_gaussians(gd, camd, cfg, use_sh=True)
    ((corr.correct(r, 0).clamp(0, 1) - 0.5) ** 2).mean().backward()
    corr.step(0.5)
    for p in params:
      p.grad = None

  fns = {"base": base, "corrected": corrected}
  if only:
    fns = {only: fns[only]}
  r = timed(fns, reps, warmup)
  if len(r) == 2:
    r["overhead_pct"] = 100.0 * (r["corrected"]["median_ms"] / r["base"]["median_ms"] - 1.0)
  print("c2 one-call fwd+bwd: " + "  ".join(f"{k} {v['median_ms']:.3f} ms" for k, v in r.items() if isinstance(v, dict))
        + (f"  overhead {r['overhead_pct']:+.2f} %" if "overhead_pct" in r else ""), flush=True)
  return r


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--parts", default="slice,tv,c2")
  ap.add_argument("--reps", type=int, default=30)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--only", default=None)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  parts = dict(slice=part_slice, tv=part_tv, c2=part_c2)
  res = {p: parts[p](args.reps, args.warmup, args.only) for p in args.parts.split(",")}
  print(json.dumps(res))


if __name__ == "__main__":
  main()
