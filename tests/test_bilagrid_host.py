"""CPU checks of the per-pixel bilateral-grid maths (csrc/gsr_bilagrid.h, the source the HIP kernels compile) through
the host shim: the slice forward, dL/drgb and dL/dgrid against fp64 F.grid_sample and autograd, including the guidance
border (luma at or beyond 0 and 1, where the guidance gradient is 0 as in torch)."""
import numpy as np
import pytest
import torch

import hostmath
from bilagrid_recovery import oracle_slice, random_grids

TOL = 1e-5          # relative to the largest magnitude of the reference tensor


def _np(t):
  return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))


def _rel(got, want):
  want = np.asarray(want, np.float64)
  return np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30)


def _run(lib, grid, rgb, go):
  L, GH, GW = grid.shape[1:]
  H, W = rgb.shape[:2]
  g32, x32, go32 = _np(grid), _np(rgb), _np(go)
  out = np.zeros((H, W, 3), np.float32)
  d_rgb = np.zeros((H, W, 3), np.float32)
  d_grid = np.zeros(grid.shape, np.float32)
  lib.hm_bilagrid_forward(g32, L, GH, GW, x32, H, W, out)
  lib.hm_bilagrid_backward(g32, L, GH, GW, x32, H, W, go32, d_rgb, d_grid)
  return out, d_rgb, d_grid


def _oracle(grid, rgb, go):
  G = grid.double().clone().requires_grad_(True)
  x = rgb.double().clone().requires_grad_(True)
  out = oracle_slice(G, x)
  (out * go.double()).sum().backward()
  return out.detach().numpy(), x.grad.numpy(), G.grad.numpy()


@pytest.mark.parametrize("shape,H,W,seed", [((16, 16, 8), 48, 64, 0), ((8, 12, 4), 37, 29, 1), ((2, 2, 2), 7, 5, 2),
                                            ((32, 32, 16), 40, 50, 3), ((5, 3, 6), 1, 1, 4)])
def test_slice_matches_grid_sample(built_libs, shape, H, W, seed):
  lib = hostmath.load(built_libs)
  grid = random_grids(1, shape, scale=0.3, seed=seed)[0]
  gen = torch.Generator().manual_seed(100 + seed)
  rgb = 1.4 * torch.rand(H, W, 3, generator=gen) - 0.2          # luma below 0 and above 1 included
  rgb = rgb.float().double().float()
  go = torch.randn(H, W, 3, generator=gen)
  out, d_rgb, d_grid = _run(lib, grid, rgb, go)
  o_out, o_rgb, o_grid = _oracle(grid, rgb, go)
  assert _rel(out, o_out) < TOL, _rel(out, o_out)
  assert _rel(d_rgb, o_rgb) < TOL, _rel(d_rgb, o_rgb)
  assert _rel(d_grid, o_grid) < TOL, _rel(d_grid, o_grid)


def _affine_only_grad(grid, rgb, go):
  """dL/drgb with the guidance detached: A^T go, the whole gradient where grid_sample's z gradient is 0."""
  import torch.nn.functional as F
  H, W = rgb.shape[:2]
  x = rgb.double().clone().requires_grad_(True)
  ys = (torch.arange(H, dtype=torch.float64) + 0.5) / H * 2 - 1
  xs = (torch.arange(W, dtype=torch.float64) + 0.5) / W * 2 - 1
  gy, gx = torch.meshgrid(ys, xs, indexing="ij")
  lum = x.detach() @ torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64)
  A = F.grid_sample(grid.double().unsqueeze(0), torch.stack([gx, gy, lum * 2 - 1], -1).view(1, 1, H, W, 3),
                    mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
  out = (A[..., :3] @ x.unsqueeze(-1)).squeeze(-1) + A[..., 3]
  (out * go.double()).sum().backward()
  return x.grad.numpy()


def test_guidance_gradient_is_zero_on_and_beyond_the_border(built_libs):
  """Pixels with luma exactly 0, below 0, above 1 and exactly 1 get no guidance term (dL/drgb = A^T go), as grid_sample
  gives; just inside the border the term is there."""
  lib = hostmath.load(built_libs)
  grid = random_grids(1, (4, 4, 4), scale=0.5, seed=9)[0]
  vals = [[0.0, 0.0, 0.0], [-0.3, -0.1, -0.2], [1.2, 1.5, 1.1], [1.0, 1.0, 1.0], [0.01, 0.02, 0.01], [0.98, 0.99, 0.97]]
  rgb = torch.tensor(vals, dtype=torch.float32).view(1, 6, 3)
  go = torch.tensor([[0.7, -1.1, 0.4]] * 6, dtype=torch.float32).view(1, 6, 3)
  _, d_rgb, _ = _run(lib, grid, rgb, go)
  _, o_rgb, _ = _oracle(grid, rgb, go)
  plain = _affine_only_grad(grid, rgb, go)
  assert _rel(d_rgb, o_rgb) < TOL
  for px in range(4):                                   # border and beyond: torch's guidance gradient is 0
    assert np.abs(o_rgb[0, px] - plain[0, px]).max() < 1e-12, px
    assert np.abs(d_rgb[0, px] - plain[0, px]).max() < TOL * np.abs(plain).max(), px
  for px in (4, 5):                                     # just inside: it is not
    assert np.abs(o_rgb[0, px] - plain[0, px]).max() > 1e-3, px


def test_identity_grid_reproduces_the_image_bit_for_bit(built_libs):
  lib = hostmath.load(built_libs)
  from bilagrid_recovery import identity
  grid = identity(1, (16, 16, 8))[0]
  gen = torch.Generator().manual_seed(5)
  rgb = 1.6 * torch.rand(33, 47, 3, generator=gen) - 0.3
  out, _, _ = _run(lib, grid, rgb, torch.zeros_like(rgb))
  assert np.array_equal(out.view(np.uint32), _np(rgb).view(np.uint32))
