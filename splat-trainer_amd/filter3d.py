"""Mip-Splatting's 3-D smoothing filter (Yu et al., CVPR 2024, section 5.1), the partner of the 2-D Mip filter that
``RasterConfig.antialias`` switches on in the projection kernel: every Gaussian's frequency is bounded by the highest
rate at which any camera samples it, so a scene trained at one sampling rate renders at another without erosion or
high-frequency artefacts.  Two native passes (csrc/filter3d.hip, maths in csrc/gsr_filter3d.h):

``sampling_rate``     points x cameras, once per change of the cameras or the points: ``rate[p]`` = the maximum over the
                      cameras that sample ``p`` of ``f_c / d``, with ``f_c = max(fx, fy)`` in pixels, ``d`` the depth of
                      ``p`` in camera ``c`` and "samples" the frustum test of ``visibility.py`` widened by a margin
                      (a fraction of the image on every side) between the camera's own near and far planes.
``smooth_gaussians``  per frame, N rows, one autograd node: ``c = strength / rate^2`` is added to the variance of every
                      axis (the rotation is unchanged: ``S + c I = R diag(s^2 + c) R^T``) and the opacity is scaled by
                      ``prod_j s_j / s'_j``, which keeps the Gaussian's integral.  Rows with ``rate == 0`` are copied.

Departures from the published code: it keeps one ``min d`` and one ``max f`` per point over the cameras and divides them;
here each camera contributes its own ``f_c / d``, so a distant long lens cannot be paired with a near wide one.  It tests
``d > 0.2``; here the camera's own near (and far) plane.  It uses ``fx``; here ``max(fx, fy)``.

Device tensors only; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Any

import torch

from . import _lib
from ._args import f32, on_one_device, require
from ._lib import ptr as _ptr
from .data_types import Gaussians3D
from .visibility import _query_args


def sampling_rate(cameras: Any, points: torch.Tensor, margin: float = 0.15, unseen: str = "min") -> torch.Tensor:
  """The highest rate, in pixels per world unit, at which any of ``cameras`` (anything ``CameraBatch.of`` accepts)
  samples each of ``points`` (N, 3): (N,) float32.  A point that no camera samples gets, with ``unseen="min"``, the
  smallest rate among the sampled points -- the strongest filter, as the published code does; no host wait -- and with
  ``unseen="zero"`` the rate 0, which ``smooth_gaussians`` reads as "no smoothing".  When no point is sampled at all
  every rate is 0 under both."""
  if unseen not in ("min", "zero"):
    raise ValueError(f"unseen must be 'min' or 'zero', got {unseen!r}")
  margin = float(margin)
  if not margin >= 0.0:
    raise ValueError(f"margin must be >= 0, got {margin}")
  cams, p = _query_args(cameras, points)
  with _lib.on_device(p.device) as stream:
    rec = cams.records()
    focal = cams.intrinsics[:, :2].max(dim=1).values.contiguous()
    rate = torch.empty(p.shape[0], dtype=torch.float32, device=p.device)
    _lib.call("gsr_sampling_rate", _ptr(p), p.shape[0], _ptr(rec), _ptr(focal), rec.shape[0], margin, _ptr(rate), stream)
    if unseen == "min":
      seen = rate > 0
      lowest = torch.where(seen, rate, rate.new_full((), float("inf"))).min()          # inf when nothing is sampled
      rate = torch.where(seen, rate, lowest.nan_to_num(posinf=0.0))
  return rate


class _Filter3dFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, log_scaling, alpha_logit, rate, strength):
    ls, a = f32(log_scaling, align16=True), f32(alpha_logit, align16=True)     # (the kernels move four rows at a time)
    with _lib.on_device(ls.device) as stream:
      out_ls, out_a = torch.empty_like(ls), torch.empty_like(a)
      _lib.call("gsr_filter3d_forward", _ptr(ls), _ptr(a), _ptr(rate), ls.shape[0], strength, _ptr(out_ls), _ptr(out_a),
                stream)
    ctx.save_for_backward(ls, a, rate)
    ctx.strength = strength
    return out_ls, out_a

  @staticmethod
  def backward(ctx, g_ls, g_a):
    ls, a, rate = ctx.saved_tensors
    with _lib.on_device(ls.device) as stream:
      g_ls, g_a = f32(g_ls, align16=True), f32(g_a, align16=True)         # (an unused output arrives as zeros)
      d_ls, d_a = torch.empty_like(ls), torch.empty_like(a)
      _lib.call("gsr_filter3d_backward", _ptr(ls), _ptr(a), _ptr(rate), ls.shape[0], ctx.strength, _ptr(g_ls), _ptr(g_a),
                _ptr(d_ls), _ptr(d_a), stream)
    return d_ls, d_a, None, None


def smooth_gaussians(gaussians: Gaussians3D, rate: torch.Tensor, strength: float = 0.2) -> Gaussians3D:
  """``gaussians`` with the 3-D smoothing filter applied: ``log_scaling`` and ``alpha_logit`` are new tensors, one
  autograd node over the two kernels (the backward recomputes, nothing but the inputs is kept); position, rotation and
  feature are the same tensors.  ``rate`` (N,) float32 from ``sampling_rate`` carries no gradient; ``strength`` is the
  paper's 0.2, and 0 returns ``gaussians`` itself."""
  strength = float(strength)
  if not strength >= 0.0:
    raise ValueError(f"strength must be >= 0, got {strength}")
  ls, a = gaussians.log_scaling, gaussians.alpha_logit
  N = int(require("log_scaling", ls, shape=("N", 3), dtype=torch.float32).shape[0])
  require("alpha_logit", a, shape=(N, 1), dtype=torch.float32)
  require("rate", rate, shape=(N,), dtype=torch.float32)
  on_one_device(dict(log_scaling=ls, alpha_logit=a, rate=rate), what="the 3-D smoothing filter")
  if strength == 0.0 or N == 0:
    return gaussians
  out_ls, out_a = _Filter3dFn.apply(ls, a, f32(rate, align16=True), strength)
  return Gaussians3D(position=gaussians.position, rotation=gaussians.rotation, log_scaling=out_ls, alpha_logit=out_a,
                     feature=gaussians.feature)
