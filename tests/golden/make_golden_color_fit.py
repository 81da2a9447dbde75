"""Writes tests/golden/color_fit_ref.npz from the reference's own util/colors.py (splat-trainer checkout given by
--reference; the module is loaded by file path).  Development machines only; only the .npz is kept in this repository.

    python tests/golden/make_golden_color_fit.py --reference /path/to/splat-trainer

Three fixtures (12 x 11, 24 x 40, 37 x 53).  The image is a smooth random field plus a little noise, stretched until
10-15 % of its entries are clipped, stored as uint16 (value k / 65535); the target is that image through a gamma curve, a
colour matrix and noise, stored as uint8 (value k / 255, a photograph).  Per fixture i: ``f{i}_img_u16``, ``f{i}_ref_u8``,
``f{i}_out64`` (fit_colors_batch on the inputs widened to fp64, which is exact), ``f{i}_out32_steps`` (fit_colors_batch in
fp32, as the integer distance in float32 steps from the rounded fp64 result), ``f{i}_threshold_distance`` (smallest
distance of any entry of the images or of any iterate to eps or 1 - eps), ``f{i}_eig_ratio`` (smallest kept-to-largest
eigenvalue ratio of the scaled normal equations), ``f{i}_seed``.

A seed is refused when its threshold distance is below 1e-5 or its eigenvalue ratio below 1e-6: a mask decision that
flips moves every pixel of the result, so the fixtures exclude flips outright instead of allowing for them.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import color_fit_oracle as cfo  # noqa: E402

OUT = os.path.join(HERE, "color_fit_ref.npz")
SIZES = [(12, 11), (24, 40), (37, 53)]
EPS = 0.5 / 255
MIN_DISTANCE, MIN_RATIO = 1e-5, 1e-6


def load_colors(root):
  spec = importlib.util.spec_from_file_location("reference_colors", os.path.join(root, "splat_trainer", "util", "colors.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def bilinear(coarse, H, W):
  ch, cw = coarse.shape[:2]
  ys, xs = np.linspace(0, ch - 1, H), np.linspace(0, cw - 1, W)
  y0, x0 = np.minimum(ys.astype(int), ch - 2), np.minimum(xs.astype(int), cw - 2)
  ty, tx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
  c = lambda dy, dx: coarse[y0 + dy][:, x0 + dx]
  return (c(0, 0) * (1 - tx) + c(0, 1) * tx) * (1 - ty) + (c(1, 0) * (1 - tx) + c(1, 1) * tx) * ty


def make_images(H, W, seed):
  rng = np.random.default_rng(seed)
  field = bilinear(rng.random((H // 5 + 3, W // 5 + 3, 3)), H, W) + 0.04 * rng.standard_normal((H, W, 3))
  clipped = lambda img: np.mean((img < EPS) | (img > 1 - EPS))
  lo, hi = 0.5, 8.0                                    # the stretch at which 12.5 % of the entries are clipped
  for _ in range(40):
    gain = 0.5 * (lo + hi)
    lo, hi = (gain, hi) if clipped(np.clip(0.5 + gain * (field - 0.5), 0, 1)) < 0.125 else (lo, gain)
  img_u16 = np.round(np.clip(0.5 + gain * (field - 0.5), 0, 1) * 65535).astype(np.uint16)
  for near, away in ((128, 127), (129, 130), (65407, 65408), (65406, 65405)):   # the codes within 1e-5 of eps or 1 - eps
    img_u16[img_u16 == near] = away
  img = img_u16.astype(np.float64) / 65535
  matrix = np.eye(3) + 0.12 * rng.standard_normal((3, 3))
  target = (img ** rng.uniform(0.8, 1.25)) @ matrix + 0.03 * rng.standard_normal(3) + 0.015 * rng.standard_normal((H, W, 3))
  ref_u8 = np.round(np.clip(target, 0, 1) * 255).astype(np.uint8)
  share = clipped(img)
  assert 0.10 <= share <= 0.15, share
  return img_u16, ref_u8


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reference", required=True)
  ap.add_argument("--first-seed", type=int, default=0)
  args = ap.parse_args()
  colors = load_colors(args.reference)
  data, seed = dict(count=np.int64(len(SIZES))), args.first_seed
  for i, (H, W) in enumerate(SIZES):
    while True:
      seed += 1
      try:
        img_u16, ref_u8 = make_images(H, W, seed)
      except AssertionError as e:
        print(f"{H}x{W} seed {seed}: refused, clipped share {e}")
        continue
      img, ref = cfo.decode_images(img_u16, ref_u8)
      _, info = cfo.fit(img, ref, form="lstsq")
      if info["threshold_distance"] < MIN_DISTANCE or info["eig_ratio"] < MIN_RATIO:
        print(f"{H}x{W} seed {seed}: refused, threshold distance {info['threshold_distance']:.2e}, "
              f"eigenvalue ratio {info['eig_ratio']:.2e}")
        continue
      break
    out64 = colors.fit_colors_batch(torch.from_numpy(img).double(), torch.from_numpy(ref).double()).numpy()
    out32 = colors.fit_colors_batch(torch.from_numpy(img), torch.from_numpy(ref)).numpy()
    assert np.isfinite(out64).all() and np.isfinite(out32).all()
    steps = out32.view(np.int32) - out64.astype(np.float32).view(np.int32)
    print(f"{H}x{W} seed {seed}: clipped {np.mean((img < EPS) | (img > 1 - EPS)):.3f}, threshold distance "
          f"{info['threshold_distance']:.2e}, eigenvalue ratio {info['eig_ratio']:.2e}, max |fp32 - fp64| "
          f"{np.abs(out32.astype(np.float64) - out64).max():.2e}, mse before {np.mean((img - ref) ** 2):.2e} after "
          f"{np.mean((out64 - ref) ** 2):.2e}")
    data.update({f"f{i}_img_u16": img_u16, f"f{i}_ref_u8": ref_u8, f"f{i}_out64": out64, f"f{i}_out32_steps": steps,
                 f"f{i}_threshold_distance": np.float64(info["threshold_distance"]),
                 f"f{i}_eig_ratio": np.float64(info["eig_ratio"]), f"f{i}_seed": np.int64(seed)})
  np.savez_compressed(OUT, **data)
  print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
  main()
