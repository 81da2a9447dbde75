"""Bilateral-grid colour correction: the reference's ``splat_trainer.color_corrector`` BilateralCorrector
(bilateral_corrector.py, util/lib_bilagrid.py; ``--bilateral`` in scripts/train_scan.py) on HIP kernels.

One grid per training image, ``grids`` of shape (N, 12, L, GH, GW) (float32), identity affine at start.  Image k is
corrected by sampling grid k at each pixel -- x and y from the pixel centre, z from the pixel's BT.601 luma -- with
trilinear interpolation (``F.grid_sample`` with align_corners=True and border padding) and applying the sampled 3x4
affine to the pixel's colour.  The slice forward and backward and the grids' total variation are HIP kernels
(csrc/bilagrid.hip) with fixed-order sums: no float atomics, bit-reproducible.  There is no CPU fallback.

    corrector = BilateralCorrectorConfig().make_corrector(num_images, "cuda")
    image = corrector.correct(rendering, image_idx)      # (H, W, 3), differentiable in the grids and the image
    ...loss(image, target).backward()...
    corrector.step(t)                                    # weighted TV + its gradient, Adam over the grids, zero_grad
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, Dict, Tuple, Union

import torch
from torch import nn

from . import _lib
from ._args import f32
from ._lib import current_stream_ptr as _stream, ptr as _ptr

MIN_GRID, MAX_GRID = 2, 64


def _grid_shape(grids: torch.Tensor) -> Tuple[int, int, int, int]:
  if grids.dim() != 5 or grids.shape[1] != 12:
    raise ValueError(f"grids must have shape (N, 12, L, GH, GW), got {tuple(grids.shape)}")
  N, _, L, GH, GW = grids.shape
  if N < 1 or not all(MIN_GRID <= d <= MAX_GRID for d in (L, GH, GW)):
    raise ValueError(f"grid dimensions must lie in {MIN_GRID}..{MAX_GRID} and N >= 1, got {tuple(grids.shape)}")
  if grids.dtype is not torch.float32 or not grids.is_contiguous():
    raise ValueError("grids must be a contiguous float32 tensor")
  if not grids.is_cuda:
    raise ValueError("bilateral grids run only on a HIP device; there is no CPU fallback")
  return N, L, GH, GW


class _SliceFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, grids, image, k):
    N, L, GH, GW = grids.shape[0], grids.shape[2], grids.shape[3], grids.shape[4]
    H, W = image.shape[0], image.shape[1]
    out = torch.empty_like(image)
    _lib.call("gsr_bilagrid_slice_forward", _ptr(grids), N, L, GH, GW, k, _ptr(image), H, W, _ptr(out), _stream())
    ctx.save_for_backward(grids, image)
    ctx.k = k
    return out

  @staticmethod
  def backward(ctx, g):
    grids, image = ctx.saved_tensors
    want_grids, want_image = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not (want_grids or want_image):
      return None, None, None
    N, L, GH, GW = grids.shape[0], grids.shape[2], grids.shape[3], grids.shape[4]
    H, W = image.shape[0], image.shape[1]
    go = f32(g)
    d_image = torch.empty_like(image) if want_image else None
    d_grids, ws = None, None
    if want_grids:
      d_grids = torch.zeros_like(grids)          # the kernels write slice k; the other images get no gradient
      ws = _lib.workspace(_lib.load().gsr_bilagrid_workspace_bytes(L, GH, GW), grids.device)
    _lib.call("gsr_bilagrid_slice_backward", _ptr(grids), N, L, GH, GW, ctx.k, _ptr(image), H, W, _ptr(go), _ptr(d_image),
              _ptr(d_grids), _ptr(ws), ws.numel() if want_grids else 0, _stream())
    return d_grids, d_image, None


def bilateral_correct(grids: torch.Tensor, image_idx: int, image: torch.Tensor) -> torch.Tensor:
  """Colour-corrects ``image`` (H, W, 3) with grid ``image_idx`` of ``grids`` (N, 12, L, GH, GW); returns (H, W, 3)
  float32.  Gradients flow to ``grids`` (slice ``image_idx`` only) and to ``image``.  ``image`` may be of any float
  dtype and any strides: it is cast to contiguous float32 in front of the kernels, and its gradient comes back in its
  own dtype.  Raises ValueError for a channel count other than 3, an index outside [0, N), a grid dimension outside
  2..64 and for CPU tensors."""
  N, L, GH, GW = _grid_shape(grids)
  if image.dim() != 3 or image.shape[2] != 3:
    raise ValueError(f"image must have shape (H, W, 3), got {tuple(image.shape)}")
  if not image.is_floating_point():
    raise ValueError(f"image must be a float tensor, got {image.dtype}")
  if not image.is_cuda:
    raise ValueError("bilateral_correct runs only on a HIP device; there is no CPU fallback")
  if image.device != grids.device:
    raise ValueError(f"image on {image.device} and grids on {grids.device}")
  H, W = image.shape[0], image.shape[1]
  if not (1 <= H <= _lib.BILAGRID_MAX_SIDE and 1 <= W <= _lib.BILAGRID_MAX_SIDE):
    raise ValueError(f"image sides must lie in 1..{_lib.BILAGRID_MAX_SIDE}, got {H} x {W}")
  k = int(image_idx)
  if not 0 <= k < N:
    raise ValueError(f"image_idx {k} outside [0, {N})")
  return _SliceFn.apply(grids, f32(image, detach=False), k)


class _TVFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, grids):
    N, L, GH, GW = grids.shape[0], grids.shape[2], grids.shape[3], grids.shape[4]
    tv = torch.empty(1, dtype=torch.float32, device=grids.device)
    d = torch.empty_like(grids) if ctx.needs_input_grad[0] else None
    _tv_launch(grids, N, L, GH, GW, 1.0, tv, d, False)
    ctx.save_for_backward(d)
    return tv[0]

  @staticmethod
  def backward(ctx, g):
    (d,) = ctx.saved_tensors
    return d * g.to(torch.float32)


def _tv_launch(grids, N, L, GH, GW, weight, tv, d, accumulate):
  ws = _lib.workspace(_lib.load().gsr_bilagrid_workspace_bytes(L, GH, GW), grids.device)
  _lib.call("gsr_bilagrid_tv", _ptr(grids), N, L, GH, GW, float(weight), _ptr(tv), _ptr(d), 1 if accumulate else 0,
            _ptr(ws), ws.numel(), _stream())


def bilateral_tv_loss(grids: torch.Tensor) -> torch.Tensor:
  """Total variation of the grids as the reference's total_variation_loss computes it:
  (1/N) sum over the three grid axes of sum((G shifted by one - G)^2) / (12 L GH GW).  A 0-d device tensor (no host
  sync); differentiable in ``grids``."""
  _grid_shape(grids)
  return _TVFn.apply(grids)


def _identity_grid(L: int, GH: int, GW: int) -> torch.Tensor:
  eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=torch.float32)
  return eye.view(1, 12, 1, 1, 1).repeat(1, 1, L, GH, GW)


class BilateralGrid(nn.Module):
  """``num`` grids of ``grid_X`` (width) x ``grid_Y`` (height) x ``grid_W`` (guidance levels), identity at start.
  Its state dict (``grids`` (num, 12, grid_W, grid_Y, grid_X), ``rgb2gray_weight`` (1, 3)) matches the reference's
  BilateralGrid, so a reference checkpoint's ``bil_grids`` loads as it is."""

  def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8):
    super().__init__()
    if not all(MIN_GRID <= d <= MAX_GRID for d in (grid_X, grid_Y, grid_W)) or num < 1:
      raise ValueError(f"grid dimensions must lie in {MIN_GRID}..{MAX_GRID} and num >= 1")
    self.grid_width, self.grid_height, self.grid_guidance = grid_X, grid_Y, grid_W
    self.grids = nn.Parameter(_identity_grid(grid_W, grid_Y, grid_X).repeat(num, 1, 1, 1, 1))
    self.register_buffer("rgb2gray_weight", torch.tensor([[0.299, 0.587, 0.114]]))

  @property
  def num(self) -> int:
    return self.grids.shape[0]

  def forward(self, image: torch.Tensor, image_idx: int) -> torch.Tensor:
    return bilateral_correct(self.grids, image_idx, image)


LearningRate = Union[float, Callable[[float], float]]


@dataclass
class BilateralCorrectorConfig:
  """The reference's BilateralCorrectorConfig.  ``lr`` is a float or a schedule ``t -> lr`` (t = training progress in
  [0, 1]); the reference's VaryingFloat schedules are not reproduced."""
  bilateral_grid_shape: Tuple[int, int, int] = (16, 16, 8)
  tv_weight: float = 10.0
  lr: LearningRate = 2e-4

  def make_corrector(self, num_images: int, device) -> "BilateralCorrector":
    return BilateralCorrector(self, num_images, device)

  def from_state_dict(self, state_dict: dict, device) -> "BilateralCorrector":
    corrector = BilateralCorrector(self, state_dict["num_images"], device)
    corrector.bil_grids.load_state_dict(state_dict["bil_grids"])
    corrector.bil_grid_optimizer.load_state_dict(state_dict["optimizer"])
    return corrector


def _lr_at(lr: LearningRate, t: float) -> float:
  return float(lr(t)) if callable(lr) else float(lr)


class BilateralCorrector:
  """correct(rendering, image_idx) -> (H, W, 3); step(t) adds tv_weight * TV of all grids to their gradient (one
  kernel writes the value and the gradient), takes an Adam step over the grids and clears the gradients, and returns
  the weighted TV as a device tensor (the reference reads it back to the host every step; nothing here does)."""

  def __init__(self, config: BilateralCorrectorConfig, num_images: int, device):
    self.config = config
    X, Y, Wl = config.bilateral_grid_shape
    self.bil_grids = BilateralGrid(num_images, grid_X=X, grid_Y=Y, grid_W=Wl).to(device)
    self.bil_grid_optimizer = torch.optim.Adam(self.bil_grids.parameters(), lr=_lr_at(config.lr, 0.0))

  @property
  def num_images(self) -> int:
    return self.bil_grids.num

  def correct(self, rendering, image_idx: int) -> torch.Tensor:
    image = rendering.image if hasattr(rendering, "image") else rendering
    return bilateral_correct(self.bil_grids.grids, image_idx, image)

  def zero_grad(self):
    self.bil_grid_optimizer.zero_grad()

  def step(self, t: float = 0.0) -> torch.Tensor:
    lr = _lr_at(self.config.lr, t)
    for group in self.bil_grid_optimizer.param_groups:
      group["lr"] = lr
    grids = self.bil_grids.grids
    N, L, GH, GW = _grid_shape(grids)
    tv = torch.empty(1, dtype=torch.float32, device=grids.device)
    accumulate = grids.grad is not None
    if not accumulate:
      grids.grad = torch.empty_like(grids)
    elif not grids.grad.is_contiguous():
      grids.grad = grids.grad.contiguous()
    _tv_launch(grids.detach(), N, L, GH, GW, self.config.tv_weight, tv, grids.grad, accumulate)
    self.bil_grid_optimizer.step()
    self.zero_grad()
    return tv[0]

  def state_dict(self) -> Dict[str, Any]:
    return dict(bil_grids=self.bil_grids.state_dict(), optimizer=self.bil_grid_optimizer.state_dict(),
                num_images=self.num_images)
