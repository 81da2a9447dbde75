"""The evaluation pass: the reference's ``trainer/evaluation.py`` (``Evaluation``) and ``util/colors.py``
(``mse_to_psnr``, ``compute_psnr``, ``fit_colors``, ``fit_colors_batch``) under the same names, so both are import swaps.

The colour fit runs as HIP kernels behind the C ABI (csrc/eval.hip, maths in csrc/gsr_eval.h): per iteration one pass over
the pixels that applies the previous warp and sums the normal equations in fp64, and a one-block solve on the device; no
vendor solver, no host round trip, bit-reproducible.  On systems of full rank the result equals the reference's
``torch.linalg.lstsq`` form to rounding.  Where the reference has no usable behaviour -- a rank-deficient system (a grey
image, a constant channel: NaN or garbage there) -- this one is defined: eigenvalues at or below 1e-9 of the largest are
dropped and the minimum-norm solution is used; a channel without a single unclipped pixel maps to 0.

The three image metrics (PSNR from the MSE, L1, SSIM with valid padding) of one image come from ONE native call that
writes three device floats -- a row of a caller's table if wanted -- so a whole evaluation set needs one read-back
(``evaluate_scene``) instead of three ``.item()`` waits per image.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from functools import cached_property
from typing import Any, Dict, Iterable, Optional, Tuple

import torch

from . import _lib
from ._args import f32
from ._lib import ptr as _ptr

__all__ = ["mse_to_psnr", "compute_psnr", "fit_colors", "fit_colors_batch", "image_metrics", "Evaluation",
           "evaluate_scene"]


def mse_to_psnr(mse):
  return 10 * torch.log10(1 / mse)


def compute_psnr(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
  return mse_to_psnr(torch.nn.functional.mse_loss(a, b))


def fit_colors_batch(img: torch.Tensor, ref: torch.Tensor, num_iters: int = 5, eps: float = 0.5 / 255) -> torch.Tensor:
  """Warp the colours of ``img`` (..., 3) towards ``ref`` with the iterative affine-quadratic fit; all leading
  dimensions form one system.  Returns a new float32 tensor of ``img``'s shape."""
  if img.shape != ref.shape:
    raise ValueError(f"img {tuple(img.shape)} and ref {tuple(ref.shape)} must have the same shape")
  if img.dim() < 1 or img.shape[-1] != 3:
    raise ValueError(f"the native colour fit takes three channels, got shape {tuple(img.shape)}")
  if not (img.is_cuda and ref.is_cuda) or img.device != ref.device:
    raise ValueError("fit_colors runs only on a HIP device (both images on the same one); there is no CPU fallback")
  if img.numel() == 0:
    raise ValueError("fit_colors needs at least one pixel")
  if not (0 <= int(num_iters) <= 64) or not (0.0 <= float(eps) < 0.5):
    raise ValueError("num_iters must be in 0..64 and eps in [0, 0.5)")
  x, r = f32(img, align16=True), f32(ref, align16=True)
  P = x.numel() // 3
  with _lib.on_device(x.device) as stream:
    out = torch.empty_like(x)
    ws = _lib.workspace(_lib.load().gsr_color_fit_workspace_bytes(P), x.device)
    _lib.call("gsr_color_fit", _ptr(x), _ptr(r), P, int(num_iters), float(eps), _ptr(out), _ptr(ws), ws.numel(), stream)
  return out


def fit_colors(pred_image: torch.Tensor, source_image: torch.Tensor) -> torch.Tensor:
  """Fit the colour transform between the two images and return the corrected ``pred_image``."""
  return fit_colors_batch(pred_image.unsqueeze(0), source_image.unsqueeze(0)).squeeze(0)


def image_metrics(image: torch.Tensor, source: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
  """[mse, l1, ssim (valid padding)] of two (H, W, 3) images as three device floats, from one native call.  ``out``: a
  contiguous float32 view of three elements to write into (a row of a table); a new tensor otherwise."""
  if image.dim() != 3 or image.shape[-1] != 3 or image.shape != source.shape:
    raise ValueError(f"expected two (H, W, 3) images of equal shape, got {tuple(image.shape)} and {tuple(source.shape)}")
  if not (image.is_cuda and source.is_cuda) or image.device != source.device:
    raise ValueError("image_metrics runs only on a HIP device (both images on the same one); there is no CPU fallback")
  H, W = image.shape[0], image.shape[1]
  if H <= 10 or W <= 10:
    raise ValueError("image too small for padding='valid' (needs more than 10 pixels per side)")       # as fused_ssim
  if out is None:
    out = torch.empty(3, dtype=torch.float32, device=image.device)
  elif (out.shape != (3,) or out.dtype is not torch.float32 or not out.is_contiguous() or out.device != image.device):
    raise ValueError("out must be a contiguous float32 tensor of three elements on the images' device")
  x, s = f32(image, align16=True), f32(source, align16=True)
  with _lib.on_device(x.device) as stream:
    ws = _lib.workspace(_lib.load().gsr_image_metrics_workspace_bytes(H, W), x.device)
    _lib.call("gsr_image_metrics", _ptr(x), _ptr(s), H, W, _ptr(out), _ptr(ws), ws.numel(), stream)
  return out


def _metrics_dict(row) -> Dict[str, float]:
  """psnr / l1 / ssim from one read-back row [mse, l1, ssim] (Python floats)."""
  mse, l1, ssim = (float(v) for v in row)
  psnr = math.inf if mse == 0.0 else (10.0 * math.log10(1.0 / mse) if mse > 0.0 else math.nan)
  return dict(psnr=psnr, l1=l1, ssim=ssim)


@dataclass(frozen=True)
class Evaluation:
  filename: str
  rendering: Any              # a Rendering (any dataclass with an ``image`` field)
  source_image: torch.Tensor

  @property
  def image_id(self) -> str:
    return self.filename.replace('/', '_')

  @property
  def image(self) -> torch.Tensor:
    return self.rendering.image

  @cached_property
  def metrics(self) -> Dict[str, float]:
    """One native call and one read-back for all three."""
    return _metrics_dict(image_metrics(self.image, self.source_image).tolist())

  @property
  def psnr(self) -> float:
    return self.metrics["psnr"]

  @property
  def l1(self) -> float:
    return self.metrics["l1"]

  @property
  def ssim(self) -> float:
    return self.metrics["ssim"]

  def color_corrected(self) -> "Evaluation":
    corrected = replace(self.rendering, image=fit_colors(self.image, self.source_image))
    return replace(self, rendering=corrected)


def evaluate_scene(scene, views: Iterable[Tuple[str, Any, Optional[int], torch.Tensor]], color_correct: bool = False,
                   **render_options):
  """The metric loops of ``Trainer.evaluate_training`` / ``evaluate_dataset`` (trainer.py:315-402) without a host wait
  per image.  ``views`` yields ``(filename, camera_params, image_idx, source_image)``; each is rendered by
  ``scene.render(camera_params, image_idx, render_median_depth=True, **render_options)`` under ``no_grad``, its metrics
  go into a row of one device table (those of the colour-corrected image into a second one) and the tables are read back
  once at the end.  Returns ``{filename: dict(psnr, l1, ssim)}`` and, with ``color_correct``, the pair of that and the
  colour-corrected dictionary."""
  views = list(views)
  if not views:
    return ({}, {}) if color_correct else {}
  device = views[0][3].device
  table = torch.zeros((2 if color_correct else 1, len(views), 3), dtype=torch.float32, device=device)
  with torch.no_grad():
    for i, (_, camera_params, image_idx, source_image) in enumerate(views):
      rendering = scene.render(camera_params, image_idx, render_median_depth=True, **render_options)
      image_metrics(rendering.image, source_image, out=table[0, i])
      if color_correct:
        image_metrics(fit_colors(rendering.image, source_image), source_image, out=table[1, i])
  rows = table.tolist()                                                    # the one read-back
  metrics = {view[0]: _metrics_dict(rows[0][i]) for i, view in enumerate(views)}
  if not color_correct:
    return metrics
  return metrics, {view[0]: _metrics_dict(rows[1][i]) for i, view in enumerate(views)}
