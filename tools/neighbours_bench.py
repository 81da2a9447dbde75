"""Times the neighbour-search kernels (splat_trainer_amd.neighbours) with device events after warm-up, on seeded clouds,
next to a chunked torch formulation on the same GPU, and reports pairs per second and the share of the fp32 VALU issue
bound.  The loop is tools/timing.py's: each form alone, 2 warm-up calls (1 for the long ones), 1 to 10 repetitions of one
call, one reused event pair, lower median.

    python tools/neighbours_bench.py [--quick] [--json out.json]

Issue bound: 256 CUs x 4 SIMDs x 32 lanes per cycle at 2.4 GHz = 78.6e12 lane-operations/s.  The operations per pair
are those of the inner loops (csrc/neighbours.hip, counted in the gfx950 code): kNN 3 v_sub + v_mul + 2 v_fma + a
v_min per candidate for the step minimum (1 per pair, the 8-wide tree is 7 per 8) = 7; assign 3 v_sub + v_mul + 2 v_fma
+ v_cmp + 2 v_cndmask (best, label) + v_mov (label constant) = 10.
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
from timing import lower_median, repetitions  # noqa: E402

ISSUE_BOUND = 256 * 4 * 32 * 2.4e9
OPS = {"knn": 7, "assign": 10}


def cloud(n, seed):
  g = torch.Generator().manual_seed(seed)
  return (torch.randn(n, 3, generator=g) * torch.tensor([1.0, 2.0, 0.5])).cuda()


def timed(fn, reps, warmup=2):
  return lower_median(repetitions({"fn": fn}, reps, warmup)["fn"])


def torch_assign(x, c, chunk=1 << 18):
  return torch.cat([torch.cdist(x[a:a + chunk], c).argmin(1) for a in range(0, len(x), chunk)])


def torch_knn(p, k, rows):
  out, chunk = [], max(64, (1 << 28) // len(p))          # (chunk, N, 3) intermediates of at most 3 GiB
  for a in range(0, rows, chunk):
    d = ((p[a:a + chunk, None, :] - p[None]) ** 2).sum(-1)
    out.append(torch.topk(d, k + 1, 1, largest=False).values[:, 1:])
  return torch.cat(out)


def torch_kmeans_iter(x, c, iters):
  K = c.shape[0]
  for _ in range(iters):
    labels = torch_assign(x, c)
    c.zero_()
    c.scatter_add_(0, labels[:, None].repeat(1, 3), x)
    c /= torch.bincount(labels, minlength=K).type_as(c).view(K, 1)
  return labels, c


def row(name, ms, pairs, ops, torch_ms=None, aim=None):
  r = dict(case=name, ms=round(ms, 4), pairs=pairs, pairs_per_s=pairs / (ms * 1e-3),
           valu_issue_share=(pairs * ops / ISSUE_BOUND) / (ms * 1e-3) if ops else None)
  if torch_ms is not None:
    r["torch_ms"] = round(torch_ms, 3)
    r["speedup"] = round(torch_ms / ms, 1)
  if aim is not None:
    r["aim_ms"] = aim
  return r


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--quick", action="store_true", help="small sizes (a functional run)")
  ap.add_argument("--json", default=None)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  rows = []
  N, K = (300_000, 256) if args.quick else (3_000_000, 1024)
  iters = 10 if args.quick else 100
  x = cloud(N, 0)
  c0 = x[torch.randperm(N, generator=torch.Generator().manual_seed(1))[:K].cuda()].contiguous()
  ms = timed(lambda: sta.assign_clusters(x, c0), 10)
  tms = timed(lambda: torch_assign(x, c0), 3)
  rows.append(row(f"assign {N} x {K}", ms, N * K, OPS["assign"], tms, 0.5))
  c = c0.clone()
  ms = timed(lambda: sta.kmeans_iter(x, c.copy_(c0), iters), 3, warmup=1)
  t_iters = 5
  tms = timed(lambda: torch_kmeans_iter(x, c.copy_(c0), t_iters), 1, warmup=1) * iters / t_iters
  rows.append(row(f"kmeans_iter {N} x {K} x {iters}", ms, N * K * iters, None, tms, 80.0))
  for n, aim in ((20_000, None), (100_000, 3.0)) if args.quick else ((100_000, 3.0), (1_000_000, 150.0)):
    p = cloud(n, 2)
    ms = timed(lambda: sta.knn(p, 5), 5)
    sample = min(n, 20_000)                                  # torch on a sample of query rows, scaled to all rows
    tms = timed(lambda: torch_knn(p, 5, sample), 2, warmup=1) * n / sample
    rows.append(row(f"knn k=5 {n}", ms, n * (n - 1), OPS["knn"], tms, aim))
  for r in rows:
    print(json.dumps(r))
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
