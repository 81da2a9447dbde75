"""The scene regulariser (``MLPScene.compute_reg`` / ``reg_loss``, splat_trainer/scene/mlp_scene.py:246-288, weights in
config/scene/mlp.yaml:16-20) as one native forward and one native backward sweep (csrc/reg.hip), and the scene's
post-step projection (mlp_scene.py:236-237).

The reference gathers ``rendering.points.visible`` first -- ``nonzero()`` on the visibility mask, a host synchronisation
in the middle of the frame -- and then runs some twenty-five small launches per direction over the gathered rows.  Here
the mask ``visibility > 0`` is applied inside the kernel over all M culled rows and the number of visible rows stays on
the device.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping

import torch

from . import _lib
from ._args import on_one_device, require
from ._lib import ptr as _ptr
from .data_types import RenderedPoints

TERMS = ("scale", "opacity", "aspect", "specular")        # order of GsrReg.weight and of the terms buffer
WHAT = "the regulariser"


def _args(idx, log_scaling, depths, opacity, specular, visibility, weights, visibility_weighted) -> "_lib.GsrReg":
  a = _lib.GsrReg(idx=_ptr(idx), log_scaling=_ptr(log_scaling), depths=_ptr(depths), opacity=_ptr(opacity),
                   specular=_ptr(specular), visibility=_ptr(visibility), M=int(idx.shape[0]),
                   N=int(log_scaling.shape[0]), visibility_weighted=1 if visibility_weighted else 0)
  for k in range(4):
    a.weight[k] = weights[k]
  return a


class _RegFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, opacity, depths, specular, log_scaling, idx, visibility, weights, visibility_weighted):
    dev = opacity.device
    tensors = [t.detach().contiguous() for t in (opacity, depths, log_scaling)]
    spec = None if specular is None else specular.detach().contiguous()
    with _lib.on_device(dev) as stream:
      loss = torch.empty((), dtype=torch.float32, device=dev)
      terms = torch.empty(5, dtype=torch.float32, device=dev)
      ws = _lib.workspace(_lib.load().gsr_reg_workspace_bytes(int(idx.shape[0])), dev)
      a = _args(idx, tensors[2], tensors[1], tensors[0], spec, visibility, weights, visibility_weighted)
      _lib.call("gsr_reg_forward", C.byref(a), _ptr(loss), _ptr(terms), _ptr(ws), ws.numel(), stream)
    ctx.save_for_backward(*tensors, idx, visibility, terms, *(() if spec is None else (spec,)))
    ctx.has_specular = spec is not None
    ctx.weights, ctx.visibility_weighted = weights, visibility_weighted
    ctx.mark_non_differentiable(terms)
    return loss, terms

  @staticmethod
  def backward(ctx, d_loss, _d_terms):
    opacity, depths, log_scaling, idx, visibility, terms, *rest = ctx.saved_tensors
    spec = rest[0] if ctx.has_specular else None
    need_op, need_dep, need_spec, need_ls = ctx.needs_input_grad[:4]
    with _lib.on_device(opacity.device) as stream:
      d_op = torch.empty_like(opacity) if need_op else None
      d_dep = torch.empty_like(depths) if need_dep else None
      d_spec = torch.empty_like(spec) if (need_spec and spec is not None) else None
      d_ls = torch.zeros_like(log_scaling) if need_ls else None       # the kernel adds into the rows of idx
      a = _args(idx, log_scaling, depths, opacity, spec, visibility, ctx.weights, ctx.visibility_weighted)
      _lib.call("gsr_reg_backward", C.byref(a), _ptr(terms), _ptr(d_loss.float().contiguous()), _ptr(d_op), _ptr(d_dep),
                _ptr(d_spec), _ptr(d_ls), stream)
    return d_op, d_dep, d_spec, d_ls, None, None, None, None


def reg_loss(points: RenderedPoints, log_scaling: torch.Tensor, weights: Mapping[str, float],
             visibility_weighted: bool = True, return_terms: bool = False):
  """``MLPScene.reg_loss`` (mlp_scene.py:268-288) on the M culled rows of ``points``:

      s = exp(log_scaling[idx]); norm = (s . s) / depths^2; aspect = max(s) / min(s)
      opacity_term = (1 - exp(-4 opacity))^2 norm;  spec = |specular|.sum(1)   (0 when points.attributes has no specular)
      scale, opacity, aspect, specular = mean over the rows with visibility > 0 of {norm, opacity_term, aspect, spec} w
      loss = sum_k weights[k] term[k]

  with ``w = visibility`` (``visibility_weighted``, the reference's choice for a ``VisibilityOptimizer``) or 1.  A term
  whose weight is missing from ``weights`` or zero is dropped, as ``if k in weights`` does in the reference.  The mask is
  applied in the kernel: no ``points.visible``, no ``nonzero``, no read-back; when no row is visible the loss and every
  gradient are 0 (the reference's ``mean`` of nothing would be NaN).  Sums have a fixed order: two calls give the same
  bits.

  Differentiable inputs: ``points.opacity``, ``points.depths``, ``points.attributes.specular`` and the N-row
  ``log_scaling``.  ``points.visibility`` is a constant: it carries no gradient today (the reference's oracle detaches
  it too).  Reading it triggers the forward-side visibility reduction if backward has not run (``RenderedPoints``).

  Returns the loss as a device scalar; with ``return_terms`` also a device buffer of five floats for logging: the four
  unweighted terms in ``TERMS`` order and the number of visible rows."""
  unknown = set(weights) - set(TERMS)
  if unknown:
    raise ValueError(f"unknown regulariser term(s) {sorted(unknown)}; known: {TERMS}")
  w = tuple(float(weights.get(k, 0.0)) for k in TERMS)
  idx, visibility = points.idx, points.visibility
  specular = getattr(points.attributes, "specular", None) if points.attributes is not None else None
  if not isinstance(idx, torch.Tensor) or idx.dim() != 1:
    raise ValueError("points.idx must be an (M,) tensor")
  M = int(idx.shape[0])
  f32 = torch.float32
  require("points.idx", idx, dtype=torch.int64)
  require("points.opacity", points.opacity, shape=(M,), dtype=f32)
  require("points.depths", points.depths, shape=[(M, 1), (M,)], dtype=f32)
  require("points.visibility", visibility, shape=(M,), dtype=f32)
  if specular is not None:
    require("points.attributes.specular", specular, shape=(M, 3), dtype=f32)
  if not isinstance(log_scaling, torch.Tensor) or log_scaling.dim() != 2:
    raise ValueError("log_scaling must be an (N, 3) tensor")
  require("log_scaling", log_scaling, shape=(int(log_scaling.shape[0]), 3), dtype=f32)
  if M > 0 and log_scaling.shape[0] == 0:
    raise ValueError("log_scaling has no rows but points has some")
  on_one_device({"points.idx": idx, "points.opacity": points.opacity, "points.depths": points.depths,
                 "points.visibility": visibility, "points.attributes.specular": specular, "log_scaling": log_scaling},
                what=WHAT)
  loss, terms = _RegFn.apply(points.opacity, points.depths, specular, log_scaling, idx.contiguous(),
                             visibility.detach().contiguous(), w, bool(visibility_weighted))
  return (loss, terms) if return_terms else loss


@torch.no_grad()
def scene_post_step(rotation: torch.Tensor, log_scaling: torch.Tensor, eps: float = 1e-12, lo: float = -8.0,
                    hi: float = 8.0):
  """mlp_scene.py:236-237 in one launch, in place: ``rotation = F.normalize(rotation, dim=1)`` (eps 1e-12) and
  ``log_scaling.clamp_(-8, 8)``."""
  N = int(rotation.shape[0])
  require("rotation", rotation, shape=(N, 4), dtype=torch.float32)
  require("log_scaling", log_scaling, shape=(N, 3), dtype=torch.float32)
  if not (rotation.is_contiguous() and log_scaling.is_contiguous()):
    raise ValueError("rotation and log_scaling must be contiguous")
  on_one_device(dict(rotation=rotation, log_scaling=log_scaling), what=WHAT)
  with _lib.on_device(rotation.device) as stream:
    _lib.call("gsr_scene_post_step", _ptr(rotation), _ptr(log_scaling), N, float(eps), float(lo), float(hi), stream)
