"""Times the neural colour model (splat_trainer_amd.ColorModel, csrc/color_model.hip) with device events after warm-up,
next to the reference's path today (the torch modules under fp16 autocast, tests/color_model_oracle.py's restatement), in
the shipped configuration (scene/mlp.yaml: 16 point features, 32 GLO features, H 32, L 1, S 5), and reports bytes,
FLOPs and the share of the chip's peaks.  The loop is tools/timing.py's: each form alone, 3 warm-up calls, --reps
repetitions of one call, one reused event pair, lower median, in microseconds.

    python tools/color_model_bench.py [--rows 500000 3000000] [--json out.json]

Native forward = one pack + one fused forward launch; native backward = pack + fused backward + finish (torch's
autograd bookkeeping included).  Bytes per row: the forward reads point features (4 P) and the position (12) and writes
diffuse and specular (24); the backward reads the same inputs and both upstream gradients (24) and writes d_point_features
(4 P).  FLOPs per row: 2 x the Linears' multiply-adds (F 2H + H 4 twice, (S+1)^2 2F once); the backward recomputes the
forward and runs the data and weight products (3x).  Peaks: 6.3 TB/s achievable HBM, 2.5 PFLOP/s dense f16 MFMA.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import splat_trainer_amd as sta  # noqa: E402
import color_model_oracle as cmo  # noqa: E402
from timing import lower_median, repetitions  # noqa: E402

HBM = 6.3e12
MFMA_F16 = 2.5e15
P, G, H, L, S = 16, 32, 32, 1, 5


def timed(fn, reps, warmup=3):
  return lower_median(repetitions({"fn": fn}, reps, warmup)["fn"]) * 1e3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rows", type=int, nargs="+", default=[500_000, 3_000_000])
  ap.add_argument("--reps", type=int, default=50)
  ap.add_argument("--json", default=None)
  args = ap.parse_args()
  F_ = P + G
  macs = F_ * 2 * H + H * 4 + (S + 1) ** 2 * 2 * F_ + F_ * 2 * H + H * 4
  results = []
  for M in args.rows:
    torch.manual_seed(0)
    model = sta.ColorModel(sta.ColorModelConfig(hidden_features=H, hidden_layers=L, sh_degree=S), glo_features=G,
                           point_features=P).cuda()
    params = list(model.parameters())
    pf = torch.randn(M, P, device="cuda", requires_grad=True)
    pos = torch.randn(M, 3, device="cuda") * 2
    cam = torch.zeros(3, device="cuda")
    glo = (torch.randn(1, G, device="cuda") * 0.5).requires_grad_(True)
    dd, ds = torch.randn(M, 3, device="cuda") * 1e-7, torch.randn(M, 3, device="cuda") * 1e-7
    sd = {k: v for k, v in model.named_parameters()}

    def native_fwd():
      with torch.no_grad():
        model(pf, pos, cam, glo)

    col = model(pf, pos, cam, glo)

    def native_bwd():
      torch.autograd.grad([col.diffuse, col.specular], [pf, glo] + params, [dd, ds], retain_graph=True)

    def native_both():
      c = model(pf, pos, cam, glo)
      torch.autograd.grad([c.diffuse, c.specular], [pf, glo] + params, [dd, ds])

    def torch_fwd():
      with torch.no_grad():
        cmo.autocast_restatement(sd, pf, pos, cam, glo, L, S)

    tdif, tspec = cmo.autocast_restatement(sd, pf, pos, cam, glo, L, S)

    def torch_bwd():
      torch.autograd.grad([tdif, tspec], [pf, glo] + params, [dd, ds], retain_graph=True)

    def torch_both():
      a, b = cmo.autocast_restatement(sd, pf, pos, cam, glo, L, S)
      torch.autograd.grad([a, b], [pf, glo] + params, [dd, ds])

    row = dict(M=M)
    for name, fn in (("native_fwd_us", native_fwd), ("native_bwd_us", native_bwd), ("native_fwd_bwd_us", native_both),
                     ("torch_fwd_us", torch_fwd), ("torch_bwd_us", torch_bwd), ("torch_fwd_bwd_us", torch_both)):
      row[name] = timed(fn, args.reps)
    fb, bb = M * (4 * P + 12 + 24), M * (4 * P + 12 + 24 + 4 * P)
    ff, bf = 2 * macs * M, 3 * 2 * macs * M
    row.update(fwd_bytes=fb, bwd_bytes=bb, fwd_flop=ff, bwd_flop=bf,
               fwd_hbm_share=fb / (row["native_fwd_us"] * 1e-6) / HBM,
               fwd_mfma_share=ff / (row["native_fwd_us"] * 1e-6) / MFMA_F16,
               bwd_hbm_share=bb / (row["native_bwd_us"] * 1e-6) / HBM,
               bwd_mfma_share=bf / (row["native_bwd_us"] * 1e-6) / MFMA_F16,
               speedup_fwd_bwd=row["torch_fwd_bwd_us"] / row["native_fwd_bwd_us"])
    results.append(row)
    print(f"M={M}: native fwd {row['native_fwd_us']:.1f} us, bwd {row['native_bwd_us']:.1f} us, fwd+bwd "
          f"{row['native_fwd_bwd_us']:.1f} us | torch autocast fwd {row['torch_fwd_us']:.1f} us, bwd "
          f"{row['torch_bwd_us']:.1f} us, fwd+bwd {row['torch_fwd_bwd_us']:.1f} us | x{row['speedup_fwd_bwd']:.1f}")
    print(f"  fwd {fb / 1e6:.1f} MB {ff / 1e9:.2f} GFLOP: {100 * row['fwd_hbm_share']:.1f} % of HBM, "
          f"{100 * row['fwd_mfma_share']:.2f} % of f16 MFMA; bwd {bb / 1e6:.1f} MB {bf / 1e9:.2f} GFLOP: "
          f"{100 * row['bwd_hbm_share']:.1f} % of HBM, {100 * row['bwd_mfma_share']:.2f} % of f16 MFMA")
  if args.json:
    with open(args.json, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
