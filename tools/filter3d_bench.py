"""Times the 3-D smoothing filter's kernels (splat_trainer_amd.filter3d) against the torch form a user would write, on
the same GPU in the same process: the two are alternated repetition by repetition after a warm-up, timed with device
events, and reported as median and [min, max] over the repetitions (tools/timing.py's loop: 2 interleaved warm-up
rounds, 5 to 9 repetitions, one call per window, fixed order, one reused event pair, lower median; the kernels alone:
1 warm-up call, 5 windows of twenty launches, a fresh event pair per window).

    python tools/filter3d_bench.py [--quick] [--json out.json]

sampling rate    native ``sampling_rate(unseen="zero")`` against a loop over the cameras in torch (homogeneous product,
                 six comparisons, a division, a masked maximum per camera), and -- the yardstick -- against the native
                 ``frustum_counts`` on the same points and cameras, alternated the same way;
filter           native ``smooth_gaussians`` forward + backward (one autograd node, two launches) against the same
                 stable form written with torch ops and differentiated by autograd; and each kernel alone through the
                 C ABI, twenty launches between two events (the node itself is host-bound at these sizes).

A native call counts as faster only when its slowest repetition beats torch's fastest (``clear``).
Issue bound of the rate pass: 256 CUs x 4 SIMDs x 16 lanes per cycle at 2.4 GHz, at the VALU instructions per pair
counted in the gfx950 code of the main loop (416 for 4 cameras x 4 points: 26 per pair, 7.2 of them packed).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import _lib, visibility as vis  # noqa: E402
from timing import comparison_row, lower_median, repetitions, spread  # noqa: E402
from visibility_bench import ring, row  # noqa: E402  (a scene and the issue-bound arithmetic of a row; no timing)

RATE_OPS = 26
STRENGTH = 0.2


def torch_rate(image_t_world, sizes, ranges, focal, points, margin):
  homog = torch.cat([points, torch.ones_like(points[:, :1])], dim=-1)
  rate = torch.zeros(points.shape[0], device=points.device)
  for i in range(image_t_world.shape[0]):
    proj = homog @ image_t_world[i].T
    d = proj[:, 2]
    (w, h), (near, far) = sizes[i], ranges[i]
    mask = ((proj[:, 0] >= -margin * w * d) & (proj[:, 0] < (1 + margin) * w * d) & (proj[:, 1] >= -margin * h * d)
            & (proj[:, 1] < (1 + margin) * h * d) & (d > near) & (d < far))
    rate = torch.maximum(rate, torch.where(mask, focal[i] / d, torch.zeros_like(d)))
  return rate


def torch_smooth(ls, a, rate, strength):
  c = torch.where(rate > 0, strength / (rate * rate), torch.zeros_like(rate))
  l = torch.log1p(c[:, None] * torch.exp(-2 * ls))
  lc = -0.5 * l.sum(dim=1, keepdim=True)
  D = torch.sigmoid(-a) + torch.sigmoid(a) * -torch.expm1(lc)
  return ls + 0.5 * l, torch.nn.functional.logsigmoid(a) + lc - torch.log(D)


def kernels_alone(ls, a, rate, g_ls, g_a, launches=20):
  """The two kernels through the C ABI into preallocated outputs, ``launches`` back to back between two events: the
  device time of one launch each, without the autograd node's allocations (at these sizes the node is host-bound)."""
  lib, N = _lib.load(), ls.shape[0]
  out_ls, out_a, stream = torch.empty_like(ls), torch.empty_like(a), _lib.current_stream_ptr()
  p = lambda t: t.data_ptr()
  forward = lambda: _lib.check(lib.gsr_filter3d_forward(p(ls), p(a), p(rate), N, STRENGTH, p(out_ls), p(out_a), stream),
                               "gsr_filter3d_forward")
  backward = lambda: _lib.check(lib.gsr_filter3d_backward(p(ls), p(a), p(rate), N, STRENGTH, p(g_ls), p(g_a), p(out_ls),
                                                          p(out_a), stream), "gsr_filter3d_backward")
  out = {}
  for name, fn in (("forward_kernel_ms", forward), ("backward_kernel_ms", backward)):
    times = repetitions({name: fn}, 5, warmup=1, calls=launches, fresh_events=True)[name]
    out[name] = round(lower_median(times), 4)
    out[name.replace("_ms", "_range")] = [round(t, 4) for t in spread(times)]
  return out


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
  margin = 0.15
  for N in sizes_n:
    points = (torch.randn(N, 3, generator=g) * torch.tensor([3.0, 1.5, 3.0])).cuda()
    for V in cams_v:
      cams = ring(V)
      cams.records()
      m, sizes, ranges = cams.image_t_world(), cams.image_sizes.tolist(), cams.depth_ranges.tolist()
      focal = cams.intrinsics[:, :2].max(dim=1).values.tolist()
      native = lambda: sta.sampling_rate(cams, points, margin=margin, unseen="zero")
      reps = 7 if V <= 64 else 5
      ms = repetitions(dict(native=native, torch=lambda: torch_rate(m, sizes, ranges, focal, points, margin)), reps, warmup=2)
      r = row(f"sampling_rate N={N} V={V}", ms["native"], ms["torch"], N * V, RATE_OPS)
      ms = repetitions(dict(rate=native, frustum=lambda: vis.frustum_counts(cams, points)), 9, warmup=2)
      med, r4 = lower_median, lambda ts: [round(t, 4) for t in spread(ts)]
      r.update(beside_frustum_ms=round(med(ms["rate"]), 4), beside_frustum_range=r4(ms["rate"]),
               frustum_ms=round(med(ms["frustum"]), 4), frustum_range=r4(ms["frustum"]),
               rate_over_frustum=round(med(ms["rate"]) / med(ms["frustum"]), 2))
      rows.append(r)
  for N in sizes_n:
    ls = (-3 + torch.randn(N, 3, generator=g)).cuda().requires_grad_(True)
    a = (2 * torch.randn(N, 1, generator=g)).cuda().requires_grad_(True)
    rate = (50 + 400 * torch.rand(N, generator=g)).cuda()
    g_ls, g_a = torch.randn(N, 3, generator=g).cuda(), torch.randn(N, 1, generator=g).cuda()
    gaussians = sta.Gaussians3D(position=ls.detach(), rotation=ls.detach(), log_scaling=ls, alpha_logit=a,
                                feature=ls.detach())

    def native():
      out = sta.smooth_gaussians(gaussians, rate, STRENGTH)
      return torch.autograd.grad([out.log_scaling, out.alpha_logit], [ls, a], [g_ls, g_a])

    def reference():
      return torch.autograd.grad(list(torch_smooth(ls, a, rate, STRENGTH)), [ls, a], [g_ls, g_a])

    ms = repetitions(dict(native=native, torch=reference), 9, warmup=2)
    r = comparison_row(f"filter forward+backward N={N}", ms["native"], ms["torch"])
    r.update(kernels_alone(ls.detach(), a.detach(), rate, g_ls, g_a))
    rows.append(r)
  for r in rows:
    print(json.dumps(r))
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
