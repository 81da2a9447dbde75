"""Direct least-squares fit of per-point SH coefficients to view-dependent colours: what ``transfer_sh`` approaches by
one Adam step per camera, written down and solved.  The colour ``0.5 + sum_k s_ck Y_k(d)`` is linear in the coefficients,
so per point the weighted fit over all views is a K x K ridge problem, K = (degree + 1)^2 <= 16:

    (G + ridge W Y0^2 diag(0, 1, ..., 1)) s_c = b_c,    G = sum w Y Y^T,  b_c = sum w Y (y_c - 0.5),  W = sum w

with Y the basis of ``evaluate_sh_at`` at ``normalize(position - camera)``, w the view's visibility of the point and Y0
the constant basis term (``E[Y_k^2] = Y0^2`` on the sphere, so ``ridge`` is relative to a typical diagonal entry).  Two
native passes (csrc/sh_fit.hip, maths in csrc/gsr_sh_fit.h): ``add_view`` is one read-modify-write of the rows a view
sees, in fp64 without atomics; ``solve`` is one fp64 Cholesky per point.  The result is the optimum itself, the same
bits on every run, with no optimiser state; a point that no view saw gets zero coefficients (grey) and weight 0.

Not part of the direct fit: the clamp of the prediction to [0, 1] and the 0.1 L1 term on the base colour that
``transfer_sh`` has, and autograd -- nothing here is differentiable.

Device tensors only; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch

from . import _lib
from ._args import f32, require
from ._lib import ptr as _ptr

WHAT = "the SH fit"

MIN_RIDGE = 1e-6
# The lowest mean held-out colour error among 1e-3, 1e-2 and 1e-1 over 4, 8, 16 and 32 noisy views of degree-3 colours
# fitted at degree 2 (profiles/r18_sh_fit.txt).  It shrinks the higher bands of a well-sampled point by about a tenth.
DEFAULT_RIDGE = 1e-1


def _row_doubles(K: int) -> int:
  return K * (K + 1) // 2 + 3 * K + 1


class ShFit:
  """The normal equations of one fit: ``ShFit(positions, sh_degree)``, ``add_view`` per view, ``solve``."""

  def __init__(self, positions: torch.Tensor, sh_degree: int = 2):
    if sh_degree not in (0, 1, 2, 3):
      raise ValueError(f"sh_degree must be 0..3, got {sh_degree!r}")
    self.sh_degree = int(sh_degree)
    self.K = (self.sh_degree + 1) ** 2
    self.positions = f32(require("positions", positions, shape=("N", 3), what=WHAT))
    self.N = int(self.positions.shape[0])
    assert _lib.load().gsr_sh_fit_row_doubles(self.K) == _row_doubles(self.K)
    self.acc = torch.zeros(self.N, _row_doubles(self.K), dtype=torch.float64, device=self.positions.device)

  @staticmethod
  def accumulator_bytes(N: int, sh_degree: int = 2) -> int:
    """Bytes of accumulator ``ShFit`` allocates for ``N`` points: 8 (K (K + 1) / 2 + 3 K + 1) each -- 40 B per point at
    degree 0, 184 B at degree 1, 584 B at degree 2, 1480 B at degree 3: 4.4 GB for 3 M points at degree 3."""
    return int(N) * 8 * _row_doubles((int(sh_degree) + 1) ** 2)

  def add_view(self, indexes: torch.Tensor, colors: torch.Tensor, weights: torch.Tensor,
               camera_position: torch.Tensor) -> None:
    """Adds one view: ``indexes`` (M,) int64, distinct (as ``query_visibility`` returns them; duplicates are not
    detected and lose updates; an index outside [0, N) is skipped), ``colors`` (M, 3) in [0, 1], ``weights`` (M,) >= 0,
    ``camera_position`` (3,).  Rows outside ``indexes`` are not touched; an empty view changes nothing.  No host wait."""
    tensors = (("indexes", indexes), ("colors", colors), ("weights", weights), ("camera_position", camera_position))
    for name, t in tensors:
      if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")       # (this method's own type for it)
      if require(name, t, what=WHAT).device != self.acc.device:
        raise ValueError(f"{name} is on {t.device}, the fit on {self.acc.device}")
    if indexes.dtype != torch.int64:
      raise TypeError("indexes must be int64")
    M = int(indexes.shape[0])
    if indexes.dim() != 1 or tuple(colors.shape) != (M, 3) or tuple(weights.shape) != (M,) or camera_position.numel() != 3:
      raise ValueError(f"indexes (M,), colors (M, 3), weights (M,) and camera_position (3,) expected, got "
                       f"{tuple(indexes.shape)}, {tuple(colors.shape)}, {tuple(weights.shape)}, "
                       f"{tuple(camera_position.shape)}")
    if M > self.N:
      raise ValueError(f"{M} indexes for {self.N} points: they cannot be distinct")
    if M == 0:
      return
    idx = indexes.contiguous()
    col, w, cam = f32(colors), f32(weights), f32(camera_position).reshape(3)
    with _lib.on_device(self.acc.device) as stream:
      _lib.call("gsr_sh_fit_accumulate", _ptr(self.positions), self.N, _ptr(idx), M, _ptr(col), _ptr(w), _ptr(cam), self.K,
                _ptr(self.acc), stream)

  def solve(self, ridge: float = DEFAULT_RIDGE) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(sh (N, 3, K) float32, weight (N,) float32)``: the minimiser per point and the sum of its weights.  A point no
    view saw has zero coefficients and weight 0 (prune by it).  ``ridge`` >= 1e-6 (it is passed on as float32): below that
    the matrix of a point seen from one side is too close to singular for the solve, and ``ValueError`` is raised
    before anything is launched.  The accumulators are left as they are: more views can follow."""
    ridge = float(ridge)
    if not (MIN_RIDGE <= ridge < float("inf")):
      raise ValueError(f"ridge must be a finite number >= {MIN_RIDGE}, got {ridge}")
    dev = self.acc.device
    sh = torch.empty(self.N, 3, self.K, dtype=torch.float32, device=dev)
    weight = torch.empty(self.N, dtype=torch.float32, device=dev)
    if self.N == 0:
      return sh, weight
    with _lib.on_device(dev) as stream:
      _lib.call("gsr_sh_fit_solve", _ptr(self.acc), self.N, self.K, ridge, _ptr(sh), _ptr(weight), stream)
    return sh, weight


def fit_sh(eval_colors: Callable, query_visibility: Callable, cameras: Sequence, image_indexes: Sequence[Optional[int]],
           positions: torch.Tensor, sh_degree: int = 2, ridge: float = DEFAULT_RIDGE) -> Tuple[torch.Tensor, torch.Tensor]:
  """``transfer_sh``'s arguments, solved directly: one pass over ``cameras`` in the given order --
  ``query_visibility(camera) -> (indexes, visibility)``, ``eval_colors(indexes, camera, image_index) -> (M, 3)`` -- and one
  solve.  Returns ``(sh (N, 3, K), weight (N,))``."""
  ridge = float(ridge)
  if not (MIN_RIDGE <= ridge < float("inf")):
    raise ValueError(f"ridge must be a finite number >= {MIN_RIDGE}, got {ridge}")
  if len(image_indexes) != len(cameras):
    raise ValueError(f"{len(cameras)} cameras but {len(image_indexes)} image indexes")
  fit = ShFit(positions, sh_degree)
  for camera, image_index in zip(cameras, image_indexes):
    point_indexes, visibility = query_visibility(camera)
    if point_indexes.shape[0] == 0:
      continue
    colors = eval_colors(point_indexes, camera, image_index)
    fit.add_view(point_indexes, colors, visibility, camera.camera_position)
  return fit.solve(ridge)
