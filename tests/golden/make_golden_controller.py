"""Generates tests/golden/controller_vectors.json from the reference's util/misc.py (run once where the reference is
importable; it does not exist on the GPU box): ``soft_lt(o, 0.05, margin=16)`` -- the gate of the MCMC controller's noise
(mcmc_controller.py:95 at the default opacity_threshold 0.1) -- on a grid of opacities, evaluated in float64.  The
reference's own form ``1 - sigmoid(x)`` quantises to multiples of 1.1e-16 even there, so the fixture also holds the
reference's ``soft_gt(2 h - o, h, margin)`` = sigmoid(-(o - h) margin / h): the same function of ``o`` without the
subtraction from 1, which resolves the gates down to 2^-100 and below.

Usage:  TORCHDYNAMO_DISABLE=1 python tests/golden/make_golden_controller.py
"""
import json
import os

import numpy as np
import torch

from make_golden import REF, load

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
  misc = load(os.path.join(REF, "util/misc.py"), "ref_misc")
  # logits on a grid, the opacities as the float32 sigmoid would hand them to soft_lt, taken to float64 exactly
  # (-12 .. 12 in steps of 1/8, and -3 .. 0 in steps of 1/64: where the gate falls from 1 to below 2^-100)
  logits = np.union1d(np.linspace(-12.0, 12.0, 193), np.linspace(-3.0, 0.0, 193)).astype(np.float32)
  opacity = torch.sigmoid(torch.from_numpy(logits).double())
  gate = misc.soft_lt(opacity, 0.05, margin=16.0)
  mirrored = misc.soft_gt(2 * 0.05 - opacity, 0.05, margin=16.0)
  vec = {"threshold": 0.05, "margin": 16.0, "logit": logits.tolist(), "opacity": opacity.tolist(),
         "soft_lt": gate.tolist(), "soft_gt_mirrored": mirrored.tolist(),
         # 1 - sigmoid(x) in float64 carries an absolute error of 2^-53: relative 2^-29 or better above this gate
         "resolved_above": 2.0 ** -24}
  with open(os.path.join(OUT, "controller_vectors.json"), "w") as f:
    json.dump(vec, f, indent=1)


if __name__ == "__main__":
  main()
