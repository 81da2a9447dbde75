"""CPU oracle for the loss stage next to the rasterizer path.  TEST INFRASTRUCTURE ONLY.

PARITY UNPINNED.  The reference computes SSIM with the third-party CUDA package ``fused-ssim``
(/root/reference/pyproject.toml:23, unpinned version; call sites splat_trainer/trainer/trainer.py:17,112,450-462 and
splat_trainer/trainer/evaluation.py:7,42), which is neither vendored nor installed here, and the reference holds no
SSIM fixtures.  This file restates the published algorithm that package implements (Wang et al. 2004 SSIM as used by
3D Gaussian Splatting): an 11x11 Gaussian window (sigma = 1.5, separable, normalised), zero padding, per channel,

    mu1 = G*x, mu2 = G*y, s1 = G*x^2 - mu1^2, s2 = G*y^2 - mu2^2, s12 = G*xy - mu1 mu2
    ssim = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),   C1 = 0.01^2, C2 = 0.03^2

``padding="same"`` averages the whole map, ``padding="valid"`` averages the map cropped by 5 pixels on every side
(the reference always uses "valid").  Written with differentiable torch ops: autograd is the gradient oracle.

``ssim_terms`` / ``multiscale_terms`` add what a per-pixel comparison needs, in the dtype of their inputs: the map, the
three derivative maps the forward kernel hands to the backward kernel, the explicit gradient (tests/test_ssim.py ties it
to autograd's in fp64) and the per-pixel TERM SCALE S, the same sum as the gradient with every term replaced by its
magnitude: what a gradient entry is measured against, so that a faint border pixel is not hidden behind the image's
largest entry.  ``form`` chooses how the window is applied: one 2-D convolution or a row pass followed by a column pass.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2
WINDOW = 11
SIGMA = 1.5


def gaussian_window(dtype=torch.float64) -> torch.Tensor:
  x = torch.arange(WINDOW, dtype=dtype) - WINDOW // 2
  g = torch.exp(-(x * x) / (2 * SIGMA * SIGMA))
  return g / g.sum()


def ssim_map(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
  """(B,C,H,W) x2 -> (B,C,H,W) SSIM map with zero ("same") padding."""
  B, C, H, W = img1.shape
  g = gaussian_window(img1.dtype).to(img1.device)
  w2d = (g[:, None] * g[None, :])[None, None].expand(C, 1, WINDOW, WINDOW).contiguous()

  def blur(t):
    return F.conv2d(t, w2d, padding=WINDOW // 2, groups=C)

  mu1, mu2 = blur(img1), blur(img2)
  s1 = blur(img1 * img1) - mu1 * mu1
  s2 = blur(img2 * img2) - mu2 * mu2
  s12 = blur(img1 * img2) - mu1 * mu2
  return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def fused_ssim(img1: torch.Tensor, img2: torch.Tensor, padding: str = "same") -> torch.Tensor:
  """Mean SSIM, same call shape as the package the reference imports (trainer.py:112: padding="valid")."""
  m = ssim_map(img1, img2)
  if padding == "valid":
    m = m[:, :, 5:-5, 5:-5]
  return m.mean()


def multiscale_ssim_loss(pred_hwc: torch.Tensor, ref_hwc: torch.Tensor, levels: int = 4, ssim=fused_ssim):
  """trainer.py:450-462 (compute_ssim_loss): 1 - SSIM at ``levels`` scales, 2x average pooling in between.
  Returns (loss, ssim at full resolution)."""
  ref = ref_hwc.unsqueeze(0).permute(0, 3, 1, 2)
  pred = pred_hwc.unsqueeze(0).permute(0, 3, 1, 2)
  s = ssim(pred, ref, padding="valid")
  loss = 1.0 - s
  for _ in range(1, levels):
    pred = F.avg_pool2d(pred, kernel_size=2, stride=2)
    ref = F.avg_pool2d(ref, kernel_size=2, stride=2)
    loss = loss + (1.0 - ssim(pred, ref, padding="valid"))
  return loss / levels, s


# ---- per-pixel terms (tests/loss_contract.py) ----------------------------------------------------------------------

def blur(t: torch.Tensor, window: torch.Tensor = None, form: str = "conv2d") -> torch.Tensor:
  """G * t with zero padding, per plane of a (B,C,H,W) tensor.  ``form``: "conv2d" or "separable" (rows, then columns)."""
  C = t.shape[1]
  g = gaussian_window(t.dtype).to(t.device) if window is None else window.to(t.dtype)
  n = g.numel()
  if form == "conv2d":
    w2d = (g[:, None] * g[None, :])[None, None].expand(C, 1, n, n).contiguous()
    return F.conv2d(t, w2d, padding=n // 2, groups=C)
  if form != "separable":
    raise ValueError(form)
  rows = F.conv2d(t, g.view(1, 1, 1, n).expand(C, 1, 1, n).contiguous(), padding=(0, n // 2), groups=C)
  return F.conv2d(rows, g.view(1, 1, n, 1).expand(C, 1, n, 1).contiguous(), padding=(n // 2, 0), groups=C)


def ssim_terms(img1: torch.Tensor, img2: torch.Tensor, crop: int = 0, window: torch.Tensor = None,
               form: str = "conv2d") -> dict:
  """Everything per pixel of mean SSIM over the map cropped by ``crop`` (0: "same", 5: "valid"), (B,C,H,W) each:
    map              the SSIM map (whole image; the mean counts [crop, H-crop) x [crop, W-crop))
    d_mu1/d_m11/d_m12  d mean / d mu1, d mean / d(G*x^2), d mean / d(G*xy): the map's derivatives times 1/count, zero
                     outside the counted region
    d_mu1_terms      d_mu1 with each of its four products replaced by its magnitude (identical images: d_mu1 itself is
                     zero up to rounding, its terms are not)
    grad             d mean / d img1 = G*d_mu1 + 2 x G*d_m11 + y G*d_m12
    scale            S = G*|d_mu1| + 2|x| G*|d_m11| + |y| G*|d_m12|
  and the scalars ``mean`` and ``count``.  Nothing here is attached to a graph."""
  x, y = img1.detach(), img2.detach()
  B, C, H, W = x.shape
  if H - 2 * crop <= 0 or W - 2 * crop <= 0:
    raise ValueError("nothing left to count")

  def G(t):
    return blur(t, window, form)

  mu1, mu2, m11, m22, m12 = G(x), G(y), G(x * x), G(y * y), G(x * y)
  s1, s2, s12 = m11 - mu1 * mu1, m22 - mu2 * mu2, m12 - mu1 * mu2
  A1, A2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
  B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
  m = (A1 * A2) / (B1 * B2)
  count = B * C * (H - 2 * crop) * (W - 2 * crop)
  counted = torch.zeros_like(x)
  counted[:, :, crop:H - crop, crop:W - crop] = 1.0 / count
  # quotient rule on A1 A2 / (B1 B2), mu1 entering A1, A2 (through s12), B1 and B2 (through s1)
  d_mu1 = (2 * mu2 * (A2 - A1) / (B1 * B2) - 2 * mu1 * A1 * A2 * (B2 - B1) / (B1 * B2) ** 2) * counted
  d_mu1_terms = ((2 * mu2 * A2).abs() + (2 * mu2 * A1).abs()) / (B1 * B2).abs() * counted \
      + (2 * mu1 * A1 * A2).abs() * (B2.abs() + B1.abs()) / (B1 * B2) ** 2 * counted
  d_m11 = -(A1 * A2) / (B1 * B2 * B2) * counted
  d_m12 = 2 * A1 / (B1 * B2) * counted
  grad = G(d_mu1) + 2 * x * G(d_m11) + y * G(d_m12)
  scale = G(d_mu1.abs()) + 2 * x.abs() * G(d_m11.abs()) + y.abs() * G(d_m12.abs())
  return dict(map=m, d_mu1=d_mu1, d_m11=d_m11, d_m12=d_m12, d_mu1_terms=d_mu1_terms, grad=grad, scale=scale,
              mean=m[:, :, crop:H - crop, crop:W - crop].mean(), count=count)


def multiscale_terms(image_hwc: torch.Tensor, target_hwc: torch.Tensor, levels: int = 4, weights=(0.0, 10.0, 1.0),
                     clamp=(0.0, 1.0), form: str = "conv2d") -> dict:
  """The loss mix of trainer.py:448-488 without reg_loss, per pixel:
      loss = w_l1 mean|x - t| + w_mse mean (x - t)^2 + w_ssim / L sum_l (1 - ssim_valid(pool^l x, pool^l t)),
  x = clamp(image).  Returns ``loss``, ``l1``, ``mse``, ``ssim`` (list, one per level), ``grad`` (H,W,C) and the term
  scale ``scale`` = |l1 term| + |mse term| + sum_l (w_ssim / L) 0.25^l S_l[y >> l, x >> l], both zero where the clamp
  passes no gradient (torch.clamp: the bounds themselves pass)."""
  w_l1, w_mse, w_ssim = weights
  img, t = image_hwc.detach(), target_hwc.detach()
  H, W, C = img.shape
  x = img.clamp(*clamp) if clamp is not None else img
  passes = ((img >= clamp[0]) & (img <= clamp[1])) if clamp is not None else torch.ones_like(img, dtype=torch.bool)
  d = x - t
  n = d.numel()
  l1, mse = d.abs().mean(), (d * d).mean()
  g_l1, g_mse = w_l1 * torch.sign(d) / n, w_mse * 2 * d / n
  grad, scale = g_l1 + g_mse, g_l1.abs() + g_mse.abs()
  px, pt = x.permute(2, 0, 1)[None], t.permute(2, 0, 1)[None]
  ssims = []
  for l in range(levels):
    if l:
      px, pt = F.avg_pool2d(px, kernel_size=2, stride=2), F.avg_pool2d(pt, kernel_size=2, stride=2)
    terms = ssim_terms(px, pt, crop=5, form=form)
    ssims.append(terms["mean"])
    k = (w_ssim / levels) * 0.25 ** l
    for into, src, sign in ((grad, terms["grad"], -1.0), (scale, terms["scale"], 1.0)):
      up = src[0].permute(1, 2, 0)                                         # (H_l, W_l, C)
      up = up.repeat_interleave(2 ** l, 0).repeat_interleave(2 ** l, 1)    # entry [y >> l, x >> l]
      hh, ww = min(H, up.shape[0]), min(W, up.shape[1])                    # rows / columns the poolings dropped: nothing
      into[:hh, :ww] += sign * k * up[:hh, :ww]
  loss = w_l1 * l1 + w_mse * mse + w_ssim * sum(1.0 - s for s in ssims) / levels
  zero = torch.zeros_like(grad)
  return dict(loss=loss, l1=l1, mse=mse, ssim=ssims, grad=torch.where(passes, grad, zero),
              scale=torch.where(passes, scale, zero))
