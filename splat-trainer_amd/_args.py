"""The tensor rules of the Python wrappers, each written once: what a kernel argument looks like (``f32``) and how an
entry point refuses one (``require``, ``on_one_device``).  The binding-side rules -- pointer, launch, workspace, device
scope -- are in ``_lib``.
"""
from __future__ import annotations

from typing import Mapping, Optional

import torch

from ._lib import GsplatHipError


def f32(t: torch.Tensor, *, detach: bool = True, align16: bool = False) -> torch.Tensor:
  """``t`` as the kernels read it: float32, contiguous and without a graph.  A tensor that already is all that comes back
  itself (same storage, no ``.to()``, no ``.contiguous()``: the host-bound frame makes a dozen of these calls).
  ``detach=False`` keeps the graph, for arguments whose gradient flows back through the cast.  ``align16`` adds a
  16-byte aligned start (kernels that move four floats at a time): a view that starts elsewhere is copied."""
  if t.dtype is not torch.float32 or not t.is_contiguous():
    t = (t.detach() if detach else t).to(torch.float32).contiguous()
  elif detach and t.requires_grad:
    t = t.detach()
  return t.clone() if align16 and t.data_ptr() & 15 else t


def _show(shape) -> str:
  return "(" + ", ".join(str(d) for d in shape) + ("," if len(shape) == 1 else "") + ")"


def _fits(t: torch.Tensor, shape) -> bool:
  return t.dim() == len(shape) and all(isinstance(d, str) or d == s for d, s in zip(shape, t.shape))


def require(name: str, t, *, shape=None, dtype: Optional[torch.dtype] = None, what: Optional[str] = None,
            device_error=GsplatHipError) -> torch.Tensor:
  """Refuses an argument, in this order: not a tensor and a wrong shape (ValueError), a wrong dtype (ValueError), not on
  the HIP device (``device_error``; looked at only when ``what``, the caller's phrase for itself, is given).  ``shape``
  is a tuple or a list of alternatives, ``[(M, 1), (M,)]``; a string entry, ``("N", 3)``, stands for any length.
  Returns ``t``.  A module that looks at these in another order calls it once per step."""
  if not isinstance(t, torch.Tensor):
    raise ValueError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
  if shape is not None:
    shapes = shape if isinstance(shape, list) else [shape]
    if not any(_fits(t, s) for s in shapes):
      raise ValueError(f"{name} must be {' or '.join(map(_show, shapes))}, got shape {tuple(t.shape)}")
  if dtype is not None and t.dtype is not dtype:
    raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
  if what is not None and not t.is_cuda:
    raise device_error(f"{name} is on {t.device}: {what} runs on the HIP device only (there is no CPU fallback)")
  return t


def on_one_device(tensors: Mapping[str, Optional[torch.Tensor]], what: Optional[str] = None,
                  device_error=GsplatHipError) -> None:
  """Every given tensor (None: an absent optional one) on the HIP device, as ``require`` tests it, and then all of them
  on the same one (ValueError)."""
  given = {name: t for name, t in tensors.items() if t is not None}
  for name, t in given.items():
    require(name, t, what=what, device_error=device_error)
  if len({t.device for t in given.values()}) > 1:
    raise ValueError("inputs on different devices: " + ", ".join(f"{name} on {t.device}" for name, t in given.items()))
