"""evaluate_sh_at: view-dependent colour from spherical-harmonic coefficients (K3).

Call site in the reference: splat_trainer/scene/transfer_sh.py:49
``colors = evaluate_sh_at(self.sh_features, positions, indexes, cam_pos)   # N, 3``
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from ._args import f32
from ._lib import current_stream_ptr as _stream, ptr as _ptr


class ShFactorCollector:
  """Data-parallel helper: instead of forming the (N,3,K) coefficient gradient per camera, the backward pass of
  ``evaluate_sh_at`` only records the per-camera colour gradient (M,3) here; ``distributed.exchange_sh_factors``
  later all-gathers the 16x smaller factors over the ranks and one fused kernel rebuilds the summed coefficient
  gradient on every rank (csrc/geometry.hip: sh_bwd_multi_kernel)."""

  def __init__(self):
    self.items = []            # (indexes (M,), d_colour (M,3), camera_pos (3,), position term added locally?) in backward order
    # Configuration, the same on every rank (distributed.CameraShardedStep sets it): True = every rank adds the position
    # term of its OWN cameras' colour gradient to the position gradient before the all-reduce (render_gaussians' fused
    # node does, from the Jacobian its forward pass saves), so the multi-camera rebuild leaves the position gradient
    # alone and never reads the coefficient rows; False = the rebuild recomputes the term for all cameras on every rank
    # (what the three-call form needs: evaluate_sh_at hands on colour gradients only).
    self.position_term_local = False
    # Optional hook (distributed.CameraShardedStep): called by the fused node's backward pass as on_rows(indexes (M,),
    # grad_rows (M,16), camera_pos) right behind K7 + the per-splat reduction, BEFORE the geometry sweep is enqueued --
    # the colour-gradient factors are columns 8..10 of the rows, so their exchange can start there.
    self.on_rows = None

  def clear(self):
    self.items.clear()


def as_kernel_inputs(sh_features, positions, camera_pos):
  """The float32 contiguous views the kernels read (no copies when the caller already holds such tensors)."""
  return f32(sh_features), f32(positions), f32(camera_pos)


class ShSink(NamedTuple):
  """Where the SH coefficient gradient goes: the one internal form of the public ``grad_out=`` union (``sh_sink``)."""
  d_sh: Optional[torch.Tensor]        # caller-owned (N,3,K) buffer the coefficient gradient is written / added to
  d_pos: Optional[torch.Tensor]       # caller-owned (N,3) buffer the colour gradient's position term is added to
  owner: Optional[object]             # the renderer.GradOut that knows which of its buffers still hold nothing
  collector: Optional[ShFactorCollector]   # data-parallel: only the colour gradient is recorded (no d_sh, no d_pos)


def sh_sink(grad_out) -> Optional[ShSink]:
  """``None | (d_sh, d_pos) | (d_sh, d_pos, owner) | ShFactorCollector`` -> ``None`` (plain autograd) or a ``ShSink``."""
  if grad_out is None or isinstance(grad_out, ShSink):
    return grad_out
  if isinstance(grad_out, ShFactorCollector):
    return ShSink(None, None, None, grad_out)
  return ShSink(grad_out[0], grad_out[1], grad_out[2] if len(grad_out) > 2 else None, None)


def wants_position_grad(positions, sink: Optional[ShSink]) -> bool:
  return torch.is_grad_enabled() and (sink is None or sink.collector is None) and \
      (positions.requires_grad or (sink is not None and sink.d_pos is not None))


class Destination(NamedTuple):
  """How one backward node's kernels treat one group of gradient buffers (``gradient_destinations``)."""
  write_all: bool      # every scene row is written (zeros where the camera saw nothing): no zero-fill, no read-modify-write
  accumulate: bool     # the rows of ``indexes`` are added to what the buffer holds
  zero_fill: bool      # the node zero-fills the buffer itself before its kernels touch the rows of ``indexes``


_WRITE_ALL = Destination(True, False, False)           # fresh tensor or claimed buffer, written whole
_WRITE_ROWS = Destination(False, False, True)          # fresh tensor, too few rows for the whole-buffer kernels
_ACCUMULATE = Destination(False, True, False)
_ZERO_ACCUMULATE = Destination(False, True, True)

# node -> (forms the four geometry gradients?, the SH coefficient gradient?, has kernels that write EVERY scene row?)
_NODES = {"project_to_image.backward": (True, False, False),
          "render_gaussians.backward": (True, True, True),
          "evaluate_sh_at.backward": (False, True, True)}


def dense_rows(N: int, M: int) -> bool:
  """Are M visible rows of N enough for the kernels that write every scene row?  (Below an eighth of the scene the
  zero-fill + the sweep over the M rows is cheaper.)"""
  return N > 0 and (M == N or 8 * M >= N)


def gradient_destinations(node: str, N: int, M: int, K: int, grad_out, sink: Optional[ShSink], want_feature: bool = True):
  """THE decision of where a backward node's gradients go: ``(geometry, feature)``, each a ``Destination`` or None (the
  node does not form that gradient).  ``grad_out``: the renderer.GradOut whose geometry buffers the node writes, None:
  fresh tensors for autograd.  ``sink``: the SH gradient sink, None: a fresh tensor for autograd.  ``M``: the rows the
  node's kernels will write.  Every claim on a GradOut is made here, in the order the kernels run."""
  geometry_node, feature_node, every_row_kernels = _NODES[node]
  covers = dense_rows(N, M) if every_row_kernels else (N > 0 and M == N)
  geometry = feature = None
  if geometry_node:
    if grad_out is None:
      geometry = _WRITE_ALL if covers else _WRITE_ROWS
    elif every_row_kernels and covers:
      geometry = _WRITE_ALL if grad_out.claim_overwrite(node, grad_out.GEOMETRY) else _ACCUMULATE
    else:
      # (project_to_image's kernels touch only the rows of `indexes`, and in the three-call form autograd runs the SH
      # node, which ADDS its position term, before it: it never claims an overwrite)
      grad_out.claim_accumulate(node, grad_out.GEOMETRY)
      geometry = _ACCUMULATE
  if feature_node and want_feature and (sink is None or sink.collector is None):
    owner = sink.owner if sink is not None else None
    if sink is None:
      feature = _WRITE_ALL if covers else _WRITE_ROWS
    elif owner is None:
      feature = _ACCUMULATE                  # caller-owned buffer without an owner object: plain accumulation
    elif covers:
      feature = _WRITE_ALL if owner.claim_overwrite(node, ("feature",)) else _ACCUMULATE
    else:
      # The claim zero-fills the OWNER's feature buffer when that still held nothing.  A d_sh that is some other buffer is
      # zero-filled by the node: only evaluate_sh_at's public grad_out=(d_sh, d_pos, owner) can name one (render_gaussians
      # always hands its node the owner's own buffer, so the test never fires there).
      fresh = owner.claim_accumulate(node, ("feature",))
      feature = _ZERO_ACCUMULATE if (fresh and owner.feature is not sink.d_sh) else _ACCUMULATE
    if not geometry_node and owner is not None and sink.d_pos is not None and K > 1:
      # the node ADDS the colour gradient's position term to d_pos, and autograd runs it before the projection's node
      owner.claim_accumulate(node, owner.GEOMETRY)
  return geometry, feature


def launch_forward_counted(sh_features, positions, camera_pos, indexes_full, count_dev, want_pos_grad: bool):
  """K3 over an index buffer whose fill count is still on the device: N-sized outputs, rows past the count are left
  unwritten.  render_gaussians enqueues this right behind K1 + K2 so the GPU has work while the host reads the count
  back; the (out, jac) pair it returns is narrowed to M rows and handed to evaluate_sh_at(_precomputed=...)."""
  sh, pos, cam = as_kernel_inputs(sh_features, positions, camera_pos)
  N, K = indexes_full.shape[0], sh.shape[2]
  out = torch.empty(N, 3, dtype=torch.float32, device=sh.device)
  jac = torch.empty(N, 9, dtype=torch.float32, device=sh.device) if (want_pos_grad and K > 1 and N > 0) else None
  _lib.call("gsr_sh_forward", _ptr(sh), _ptr(pos), _ptr(indexes_full), N, K, _ptr(cam), _ptr(out), _ptr(jac),
            _ptr(count_dev), _stream())
  return out, jac


class _SHFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, sh_features, positions, indexes, camera_pos, sink, want_pos_grad, precomputed):
    sh, pos, cam = as_kernel_inputs(sh_features, positions, camera_pos)
    idx = indexes.contiguous()
    M, K = idx.shape[0], sh.shape[2]
    if precomputed is not None:
      out, jac = precomputed     # launch_forward_counted ran behind the projection, before M was known on the host
    else:
      out = torch.empty(M, 3, dtype=torch.float32, device=sh.device)
      # d colour / d position is cheap to form while the coefficient row is in registers; saving it (36 B per
      # splat) spares the backward pass a second sweep over the 12K-byte rows
      # (the camera position's gradient is formed from it too)
      jac = torch.empty(M, 9, dtype=torch.float32, device=sh.device) if (want_pos_grad and K > 1 and M > 0) else None
      _lib.call("gsr_sh_forward", _ptr(sh), _ptr(pos), _ptr(idx), M, K, _ptr(cam), _ptr(out), _ptr(jac), None, _stream())
    ctx.save_for_backward(sh, pos, idx, cam)
    ctx.jac = jac
    ctx.sink = sink
    ctx.in_dtypes = (sh_features.dtype, positions.dtype, camera_pos.dtype)
    return out

  @staticmethod
  def backward(ctx, d_out):
    sh, pos, idx, cam = ctx.saved_tensors
    N, _, K = sh.shape
    M = idx.shape[0]
    sink = ctx.sink
    if sink is not None and sink.collector is not None:    # data-parallel factor exchange: keep only the colour gradient
      # (4th entry False: this node hands on colour gradients only -- the position term of the colour gradient is left to
      # the multi-camera rebuild, which the exchange then runs WITH the position gradient as a target; K = 1 has no term)
      sink.collector.items.append((idx, f32(d_out), cam, K == 1))
      return None, None, None, None, None, None, None
    g = f32(d_out) if M > 0 else None
    _, dest = gradient_destinations("evaluate_sh_at.backward", N, M, K, None, sink)
    if sink is not None:                     # fused "+=" into caller-owned buffers (see renderer.GradOut)
      d_sh, d_pos = sink.d_sh, sink.d_pos
    else:
      d_sh = torch.empty(N, 3, K, dtype=torch.float32, device=pos.device)
      d_pos = torch.zeros_like(pos) if ctx.needs_input_grad[1] else None
    if dest.write_all:
      # every row of d_sh is written (zeros where this camera saw nothing): no zero-fill, no read-modify-write
      inv = None
      if M < N:
        inv = torch.empty(N, dtype=torch.int32, device=pos.device)
        _lib.call("gsr_inverse_map", _ptr(idx), M, N, _ptr(inv), _stream())
      _lib.call("gsr_sh_backward_dense", _ptr(g), _ptr(sh), _ptr(pos), _ptr(inv), M, N, K, _ptr(cam), _ptr(ctx.jac),
                _ptr(d_sh), _ptr(d_pos), _stream())
    else:
      if dest.zero_fill:
        d_sh.zero_()
      if M > 0:
        _lib.call("gsr_sh_backward", _ptr(g), _ptr(sh), _ptr(pos), _ptr(idx), M, K, _ptr(cam), _ptr(ctx.jac), _ptr(d_sh),
                  _ptr(d_pos), 1, _stream())
    d_cam = None
    if ctx.needs_input_grad[3]:
      # the colour depends on positions - camera_pos: minus the position term of every splat, summed in a fixed order
      d_cam = torch.empty(3, dtype=torch.float32, device=pos.device)
      rows = int(_lib.load().gsr_camera_grad_partial_rows(M)) if ctx.jac is not None else 0
      partials = torch.empty(max(rows, 1) * 20, dtype=torch.float32, device=pos.device)
      _lib.call("gsr_sh_camera_position_grad", _ptr(g), _ptr(ctx.jac), M, _ptr(partials), _ptr(d_cam), _stream())
      d_cam = d_cam.to(ctx.in_dtypes[2])
    if sink is not None:
      return None, None, None, d_cam, None, None, None
    return (d_sh.to(ctx.in_dtypes[0]), d_pos.to(ctx.in_dtypes[1]) if d_pos is not None else None,
            None, d_cam, None, None, None)


def evaluate_sh_at(sh_features: torch.Tensor, positions: torch.Tensor, indexes: torch.Tensor,
                   camera_pos: torch.Tensor, grad_out=None, _precomputed=None) -> torch.Tensor:
  """``sh_features (N,3,K)``, ``positions (N,3)``, ``indexes (M,) int64``, ``camera_pos (3,)`` -> ``(M,3)``.

  colour_c = 0.5 + sum_k sh[idx, c, k] * Y_k(normalize(positions[idx] - camera_pos)), K in {1,4,9,16}
  (degrees 0..3, basis order k = n(n+1)+m as splat_trainer/scene/mlp/rsh.py).  Differentiable wrt
  ``sh_features`` and, through the view direction, ``positions`` and ``camera_pos``; the caller clamps (transfer_sh.py:50).
  ``grad_out=(d_sh, d_positions[, owner])``: optional fused accumulation, see ``renderer.GradOut`` (with an ``owner``
  whose ``feature`` buffer still holds nothing this batch, the backward pass claims it and overwrites ``d_sh`` row for row
  instead of adding to it); a ``ShFactorCollector``: data-parallel, only the colour gradient is recorded."""
  for t in (sh_features, positions, indexes, camera_pos):
    if not t.is_cuda:
      raise _lib.GsplatHipError("evaluate_sh_at runs only on a HIP device; there is no CPU fallback")
  if sh_features.dim() != 3 or sh_features.shape[1] != 3 or sh_features.shape[2] not in (1, 4, 9, 16):
    raise ValueError(f"sh_features must be (N,3,K) with K in (1,4,9,16), got {tuple(sh_features.shape)}")
  if indexes.dtype != torch.int64:
    raise TypeError("indexes must be int64")
  sink = sh_sink(grad_out)
  cam_grad = torch.is_grad_enabled() and camera_pos.requires_grad
  if cam_grad and sink is not None and sink.collector is not None:
    raise ValueError("camera gradients are not supported in data-parallel mode (ShFactorCollector): detach the camera "
                     "position, or evaluate on one device")
  # the saved Jacobian also gives the camera position's gradient
  want_pos_grad = wants_position_grad(positions, sink) or cam_grad
  if cam_grad and _precomputed is not None and _precomputed[1] is None and sh_features.shape[2] > 1:
    _precomputed = None                      # evaluated without the Jacobian: evaluate again with it
  return _SHFn.apply(sh_features, positions, indexes, camera_pos, sink, want_pos_grad, _precomputed)
