"""Depth-normal consistency (2DGS, Huang et al. SIGGRAPH 2024, section 4.2; also used by GOF): the alpha-weighted splat
normals of a pixel must agree with the normal of the rendered depth surface.  Native passes (csrc/normals.hip, maths and
the contract of record in csrc/gsr_normals.h), each wrapped as one autograd node:

``splat_normals``            per visible point, the thinnest axis of the Gaussian in camera space, turned to the camera.
``geometry_features``        the same rows with the depth and a 1 behind them, (M, 5): rasterised beside the colour they
                             give the geometry image ``[N^x, N^y, N^z, D, A]`` -- alpha-weighted normal, alpha-weighted
                             depth, accumulated alpha.
``depth_normals``            the normals of a depth image, e.g. ``median_depth_image``.  Forward only.
``normal_consistency_loss``  ``mean(A - N^ . n_d)`` over the pixels whose depth stencil is valid, ``n_d`` the normals of
                             the expected depth ``D / A``; the backward reaches all five channels.

Device tensors only; there is no CPU fallback.  The camera (pose and intrinsics) receives no gradient from any of these.
"""
from __future__ import annotations

from typing import Tuple, Union

import torch

from . import _lib
from ._args import f32, on_one_device, require
from ._lib import ptr as _ptr
from .data_types import CameraParams, Gaussians3D

_WHAT = "normal consistency"


class _SplatNormalsFn(torch.autograd.Function):
  """rotation (and depth, when given) -> rows [n] or [n, depth, 1]."""

  @staticmethod
  def forward(ctx, rotation, depth, log_scaling, position, indexes, T):
    rot, ls, pos = f32(rotation, align16=True), f32(log_scaling), f32(position)
    dep = None if depth is None else f32(depth).reshape(-1)
    M, N = indexes.shape[0], rot.shape[0]
    with _lib.on_device(rot.device) as stream:
      out = torch.empty((M, 3 if dep is None else 5), dtype=torch.float32, device=rot.device)
      _lib.call("gsr_splat_normals_forward", _ptr(rot), _ptr(ls), _ptr(pos), N, _ptr(indexes), M, _ptr(T), _ptr(dep),
                _ptr(out), stream)
    ctx.save_for_backward(rot, ls, pos, indexes, T)
    ctx.depth_shape = None if depth is None else tuple(depth.shape)
    return out

  @staticmethod
  def backward(ctx, g):
    rot, ls, pos, indexes, T = ctx.saved_tensors
    M, N = indexes.shape[0], rot.shape[0]
    with _lib.on_device(rot.device) as stream:
      g = f32(g)
      d_rot = torch.zeros_like(rot)                                       # rows outside `indexes` are exactly 0
      d_depth = None
      if ctx.depth_shape is not None and ctx.needs_input_grad[1]:
        d_depth = torch.empty(M, dtype=torch.float32, device=rot.device)
      _lib.call("gsr_splat_normals_backward", _ptr(rot), _ptr(ls), _ptr(pos), N, _ptr(indexes), M, _ptr(T), _ptr(g),
                g.shape[1], _ptr(d_rot), _ptr(d_depth), stream)
    return d_rot, None if d_depth is None else d_depth.reshape(ctx.depth_shape), None, None, None, None


def _splat_rows(gaussians: Gaussians3D, indexes: torch.Tensor, depth, camera_params: CameraParams) -> torch.Tensor:
  rot = require("rotation", gaussians.rotation, shape=("N", 4), dtype=torch.float32)
  N = int(rot.shape[0])
  require("log_scaling", gaussians.log_scaling, shape=(N, 3), dtype=torch.float32)
  require("position", gaussians.position, shape=(N, 3), dtype=torch.float32)
  require("indexes", indexes, shape=("M",), dtype=torch.int64)
  M = int(indexes.shape[0])
  if depth is not None:
    require("depth", depth, shape=[(M, 1), (M,)], dtype=torch.float32)
  T = f32(require("T_camera_world", camera_params.T_camera_world, shape=(4, 4)))
  on_one_device(dict(rotation=rot, log_scaling=gaussians.log_scaling, position=gaussians.position, indexes=indexes,
                     depth=depth, T_camera_world=T), what=_WHAT)
  if M == 0:                                                              # no row: no launch
    return rot.new_zeros((0, 3 if depth is None else 5))
  return _SplatNormalsFn.apply(rot, depth, gaussians.log_scaling, gaussians.position, indexes.contiguous(), T)


def splat_normals(gaussians: Gaussians3D, indexes: torch.Tensor, camera_params: CameraParams) -> torch.Tensor:
  """The camera-space normal of each visible point ``indexes`` (M,) int64, unique rows of ``gaussians``: (M, 3) float32.
  The normal is the axis of the point's rotation that belongs to its smallest ``log_scaling`` (the lowest index on
  ties), rotated into the camera and negated where it points away from it.

  One autograd node.  Only ``rotation`` receives a gradient, (N, 4) with rows outside ``indexes`` exactly 0: the choice
  of the axis and the flip are constants, so ``position``, ``log_scaling`` and ``T_camera_world`` get none."""
  return _splat_rows(gaussians, indexes, None, camera_params)


def geometry_features(gaussians: Gaussians3D, indexes: torch.Tensor, depth: torch.Tensor, camera_params: CameraParams
                      ) -> torch.Tensor:
  """The feature rows ``[n, depth, 1]`` (M, 5) whose composite is the geometry image of ``normal_consistency_loss``:
  ``splat_normals`` with ``depth`` (M, 1) or (M,) from ``project_to_image`` and a constant 1 behind them.  One autograd
  node: ``rotation`` receives a gradient as in ``splat_normals``, ``depth`` its column's."""
  return _splat_rows(gaussians, indexes, depth, camera_params)


def _image_args(name: str, image: torch.Tensor, shape, projection: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
  require(name, image, shape=shape, dtype=torch.float32)
  require("projection", projection, shape=(4,))
  on_one_device({name: image, "projection": projection}, what=_WHAT)
  return f32(projection), int(image.shape[0]), int(image.shape[1])


def depth_normals(depth: torch.Tensor, projection: torch.Tensor) -> torch.Tensor:
  """The camera-space normals (H, W, 3) of a depth image (H, W) under ``projection`` = fx, fy, cx, cy: the normalised
  cross product of the central differences of the back-projected points, (0, 0, -1) for a fronto-parallel surface.
  Border pixels, and pixels whose depth or one of whose four neighbours' is not finite and above 0, get exactly 0.
  Forward only: the result carries no graph."""
  proj, H, W = _image_args("depth", depth, ("H", "W"), projection)
  d = f32(depth)
  out = torch.empty((H, W, 3), dtype=torch.float32, device=d.device)
  if H == 0 or W == 0:
    return out
  with _lib.on_device(d.device) as stream:
    _lib.call("gsr_depth_normals", _ptr(d), H, W, _ptr(proj), _ptr(out), stream)
  return out


class _NormalLossFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, geometry, projection, alpha_min):
    G = f32(geometry)
    H, W = G.shape[0], G.shape[1]
    with _lib.on_device(G.device) as stream:
      normals = torch.empty((H, W, 3), dtype=torch.float32, device=G.device)
      partials = torch.empty(_lib.load().gsr_normal_loss_blocks(H, W), dtype=torch.float32, device=G.device)
      loss = torch.empty(1, dtype=torch.float32, device=G.device)
      _lib.call("gsr_normal_loss_forward", _ptr(G), H, W, _ptr(projection), alpha_min, _ptr(normals), _ptr(partials),
                _ptr(loss), stream)
    ctx.save_for_backward(G, projection)
    ctx.alpha_min = alpha_min
    ctx.mark_non_differentiable(normals)
    return loss.reshape(()), normals

  @staticmethod
  def backward(ctx, g_loss, _g_normals):
    G, projection = ctx.saved_tensors
    with _lib.on_device(G.device) as stream:
      g = f32(g_loss).reshape(1)
      d_G = torch.empty_like(G)
      _lib.call("gsr_normal_loss_backward", _ptr(G), G.shape[0], G.shape[1], _ptr(projection), ctx.alpha_min, _ptr(g),
                _ptr(d_G), stream)
    return d_G, None, None


def normal_consistency_loss(geometry_image: torch.Tensor, projection: torch.Tensor, alpha_min: float = 0.5,
                            return_normals: bool = False) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
  """The depth-normal consistency loss of a geometry image (H, W, 5) = ``[N^x, N^y, N^z, D, A]``, the composite of
  ``geometry_features``: with ``d = D / A`` where ``A >= alpha_min`` (no depth elsewhere) and ``n_d`` the
  ``depth_normals`` of ``d``, the scalar ``sum(A - N^ . n_d) / (H W)`` over the pixels whose ``n_d`` is valid.  0 where
  splat and depth normals agree on an opaque surface.

  One autograd node; the gradient reaches all five channels (``D`` and ``A`` also through the depth of the four
  neighbouring stencils), not ``projection``.  A fixed-order sum: two calls give the same bits.  With
  ``return_normals`` also ``n_d`` (H, W, 3), without a graph -- the picture to look at."""
  alpha_min = float(alpha_min)
  if alpha_min != alpha_min:
    raise ValueError("alpha_min must be a number, got NaN")
  proj, H, W = _image_args("geometry_image", geometry_image, ("H", "W", 5), projection)
  if H == 0 or W == 0:                                                    # no pixel: no launch
    loss, normals = geometry_image.sum() * 0.0, geometry_image.new_zeros((H, W, 3))
  else:
    loss, normals = _NormalLossFn.apply(geometry_image, proj, alpha_min)
  return (loss, normals) if return_normals else loss
