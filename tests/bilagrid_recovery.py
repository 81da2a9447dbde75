"""Bilateral-grid oracle and grid-recovery loop shared by tests/test_bilagrid_host.py, tests/test_gpu_bilagrid.py and the
calibration of the recovery thresholds on the CPU fp64 oracle (``python tests/bilagrid_recovery.py``).

The oracle is torch itself: F.grid_sample (trilinear, border padding, align_corners=True) of grid k at the pixel centres
and the pixel luma, the sampled 3x4 affine applied to the colour, and the reference's total variation formula."""
import os
import sys

import torch
import torch.nn.functional as F

LUMA = (0.299, 0.587, 0.114)

# Recovery: 3 renders (96 x 72) of synthetic.scene_b, each through its own known grid (8, 8, 4): a smooth random
# near-identity grid times a per-image gain and white balance.  STEPS corrector steps (Adam, LR, TV_WEIGHT) over the
# grids alone.  Calibration on the fp64 oracle (python tests/bilagrid_recovery.py): image MSE falls 496x in 150 steps (2.7e-3 -> 5.5e-6).
# The test asks for 10x (at least 2x margin on the calibration).
SHAPE = (8, 8, 4)
NUM_IMAGES = 3
STEPS = 150
LR = 1e-2
TV_WEIGHT = 1.0
MIN_RATIO = 10.0


def oracle_slice(grid: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
  """grid (12, L, GH, GW), rgb (H, W, 3) -> (H, W, 3), differentiable in both (use float64)."""
  H, W = rgb.shape[0], rgb.shape[1]
  dt, dev = rgb.dtype, rgb.device
  ys = (torch.arange(H, dtype=dt, device=dev) + 0.5) / H * 2 - 1
  xs = (torch.arange(W, dtype=dt, device=dev) + 0.5) / W * 2 - 1
  gy, gx = torch.meshgrid(ys, xs, indexing="ij")
  lum = rgb @ torch.tensor(LUMA, dtype=dt, device=dev)
  coords = torch.stack([gx, gy, lum * 2 - 1], dim=-1).view(1, 1, H, W, 3)
  A = F.grid_sample(grid.unsqueeze(0).to(dt), coords, mode="bilinear", padding_mode="border", align_corners=True)
  A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
  return (A[..., :3] @ rgb.unsqueeze(-1)).squeeze(-1) + A[..., 3]


def oracle_tv(grids: torch.Tensor) -> torch.Tensor:
  N = grids.shape[0]
  count = grids[0].numel()
  tv = 0
  for ax in range(2, 5):
    n = grids.shape[ax]
    tv = tv + (grids.narrow(ax, 1, n - 1) - grids.narrow(ax, 0, n - 1)).pow(2).sum() / count
  return tv / N


def identity(N, shape, dtype=torch.float32, device="cpu"):
  X, Y, L = shape
  eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=dtype, device=device)
  return eye.view(1, 12, 1, 1, 1).repeat(N, 1, L, Y, X)


def random_grids(N, shape, scale=0.2, seed=0, dtype=torch.float32):
  """Identity plus uniform noise of the given scale at every vertex (parity tests)."""
  gen = torch.Generator().manual_seed(seed)
  X, Y, L = shape
  return identity(N, shape, dtype) + scale * (2 * torch.rand(N, 12, L, Y, X, generator=gen, dtype=dtype) - 1)


def true_grids(N=NUM_IMAGES, shape=SHAPE, seed=7):
  """Smooth near-identity grids (noise on a 2 x 2 x 2 lattice, upsampled trilinearly) times a per-image gain and white
  balance on the output rows: a luminance-dependent, smooth colour transform per image (float64)."""
  gen = torch.Generator().manual_seed(seed)
  X, Y, L = shape
  coarse = 0.08 * (2 * torch.rand(N, 12, 2, 2, 2, generator=gen, dtype=torch.float64) - 1)
  fine = F.interpolate(coarse, size=(L, Y, X), mode="trilinear", align_corners=True)
  G = identity(N, shape, torch.float64) + fine
  gain = 0.8 + 0.4 * torch.rand(N, generator=gen, dtype=torch.float64)
  wb = 0.9 + 0.2 * torch.rand(N, 3, generator=gen, dtype=torch.float64)
  row_scale = (gain[:, None] * wb).repeat_interleave(4, dim=1)          # (N, 12): rows m scale by gain * wb[m]
  return G * row_scale.view(N, 12, 1, 1, 1)


def scene(width=96, height=72):
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  if root not in sys.path:
    sys.path.insert(0, root)
  from splat_trainer_amd import synthetic
  return synthetic.scene_b(3000, width, height, sh_degree=0, seed=11, num_cameras=8, sigma_px=2.5)


def fit(correct, step, renders, targets, steps=STEPS):
  """correct(k, image) -> corrected image; step(t) -> the corrector's step.  Returns (mse before, mse after)."""
  def mse():
    with torch.no_grad():
      return sum(float(((correct(k, r) - t) ** 2).mean()) for k, (r, t) in enumerate(zip(renders, targets))) / len(renders)

  before = sum(float(((r - t) ** 2).mean()) for r, t in zip(renders, targets)) / len(renders)
  for s in range(steps):
    for k, (r, t) in enumerate(zip(renders, targets)):
      ((correct(k, r) - t) ** 2).mean().backward()
    step(s / steps)
  return before, mse()


def calibrate():
  """The recovery loop on the CPU fp64 oracle: Adam over fp64 grids, the oracle slice and TV."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  sys.path.insert(0, root)
  from oracle import torch_oracle as oracle
  from splat_trainer_amd import RasterConfig
  g, cams = scene()
  cfg = RasterConfig()
  renders = []
  for cam in cams[:NUM_IMAGES]:
    out = oracle.render(g.position.double(), g.log_scaling.double(), g.rotation.double(), g.alpha_logit.double(),
                        g.feature.double(), cam.T_camera_world.double(), cam.projection.double(), cam.image_size,
                        cam.near_plane, cam.far_plane, cfg, use_sh=True)[0]
    renders.append(out.image.detach())
  Gt = true_grids()
  targets = [oracle_slice(Gt[k], r).detach() for k, r in enumerate(renders)]
  grids = identity(NUM_IMAGES, SHAPE, torch.float64).requires_grad_(True)
  opt = torch.optim.Adam([grids], lr=LR)

  def step(t):
    (TV_WEIGHT * oracle_tv(grids)).backward()
    opt.step()
    opt.zero_grad()

  before, after = fit(lambda k, r: oracle_slice(grids[k], r), step, renders, targets)
  print(f"fp64 oracle: image mse {before:.3e} -> {after:.3e} ({before / after:.1f}x) in {STEPS} steps")


if __name__ == "__main__":
  calibrate()
