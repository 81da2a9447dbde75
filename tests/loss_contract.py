"""Cases, figures and bounds of the loss stage's per-pixel contract, shared by tests/test_loss_contract_host.py (CPU: the
noise table, planted deviations of a float32 model) and tests/test_gpu_loss_contract.py (csrc/ssim.hip through
fused_ssim, reference_loss, the clamped pixel losses and gsr_ssim_forward against oracle/ssim_oracle.py in fp64).

Inputs are float32; the oracle gets the same values as doubles.  CONTENTS:
  noise      rand against clamp(rand + 0.15 randn), what tests/test_ssim.py uses
  smooth     rand blurred twice with a 3 x 3 box against clamp(image + 0.05 randn): what a trained render looks like
  flat       0.5 against 0.5 (left half) and 0.52 (right half): G*x^2 - mu1^2 cancels completely
  identical  an image against itself (SSIM 1, every gradient term cancels against another)
  outside    rand * 1.6 - 0.3 against rand: values outside [0, 1]
reference_loss runs on ms_noise (target rand, image = target + 0.1 randn + 0.05, so pixels leave [0, 1], and entries set
exactly to both clamp bounds) and ms_smooth (the smooth pair times 1.1 - 0.03).

Figures; each a maximum over pixels.  A zero denominator has to be met by a numerator that is exactly zero, a non-finite
result where the oracle is finite -- and a finite one where the oracle is not -- counts as infinite:
  map     |ssim - oracle| over the counted region.  No public path returns the map; it is recovered from the derivative
          map gsr_ssim_forward writes, ssim = -count * d_m11 * (s1 + s2 + C2) with the oracle's fp64 s1 + s2 + C2, and the
          float32 oracle goes through the same recovery when NOISE is measured
  dmaps   each derivative map against the oracle over that map's largest magnitude; the worst of the three.  Where the
          oracle's d_mu1 has cancelled to below CANCELLED = 1e-6 of its own terms (identical images: it is zero up to
          the oracle's rounding), the largest entry of those terms (ssim_terms: d_mu1_terms) stands in for it
  grad    |g - g_oracle| / S per pixel, S the oracle's term scale (ssim_oracle.ssim_terms / multiscale_terms).  A
          gradient returned in float16 / bfloat16 is first allowed the one rounding of that format,
          eps/2 |g_oracle| + half its smallest subnormal
  mean    |mean - oracle|, against 2e-6 as in tests/test_ssim.py (not from NOISE)
  levels  every entry of reference_loss's metrics [loss, l1, mse, ssim_0 ..]: |m - oracle| / max(1, |oracle|).  Bounded
          from NOISE like the per-pixel figures: a coarsest level of 11 x 11 pixels counts one pixel per channel, so its
          "mean" carries the map's error undiminished

NOISE[(content, figure)] is the float32 oracle against the float64 oracle on these same cases, measured in the 2-D
convolution form and in the separable form (rows, then columns; the kernel's order), the larger of the two, the worst
over the content's cases and SEEDS, rounded up to two digits.  tests/test_loss_contract_host.py re-measures it;
profiles/r29_loss_contract.txt has the run.  bound = MARGIN x NOISE, MARGIN = 4: the project's margin for a kernel that
orders the same float32 operations differently.  The bounds of smooth and flat content come out above BASELINE.json's
1e-4.  That excess is not slack: it is the cancellation in G*x^2 - mu1^2 (and G*xy - mu1 mu2) of the float32
formulation, which any float32 evaluation of these moments shows on such images; noise content, where the variance is
large, stays far below 1e-4.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import ssim_oracle as so

CONTENTS = ("noise", "smooth", "flat", "identical", "outside", "ms_noise", "ms_smooth")
MARGIN = 4.0
SEEDS = (0, 1, 2, 3, 4)
MEAN_BOUND = 2e-6
CANCELLED = 1e-6
FORMS = ("conv2d", "separable")
CROP = {"same": 0, "valid": 5}

NOISE = {
  ("noise", "map"): 8.0e-6, ("noise", "dmaps"): 2.5e-5, ("noise", "grad"): 2.1e-5,
  ("smooth", "map"): 1.4e-4, ("smooth", "dmaps"): 3.3e-4, ("smooth", "grad"): 2.8e-5,
  ("flat", "map"): 4.5e-4, ("flat", "dmaps"): 2.0e-3, ("flat", "grad"): 1.3e-6,
  ("identical", "map"): 1.2e-5, ("identical", "dmaps"): 8.4e-6, ("identical", "grad"): 8.4e-4,
  ("outside", "map"): 4.9e-6, ("outside", "dmaps"): 4.2e-5, ("outside", "grad"): 3.0e-6,
  ("ms_noise", "grad"): 2.2e-5, ("ms_smooth", "grad"): 2.5e-5, ("ms_noise", "levels"): 2.9e-5, ("ms_smooth", "levels"): 3.2e-5,
}
FIXED_BOUNDS = dict(mean=MEAN_BOUND)


def bound(content: str, figure: str) -> float:
  return FIXED_BOUNDS[figure] if figure in FIXED_BOUNDS else MARGIN * NOISE[(content, figure)]


# ---- cases ------------------------------------------------------------------------------------------------------------

BOTH = ("same", "valid")
_WIDE = ((2, 3, 33, 47), (3, 2, 37, 32))                       # B > 1 and C > 1 together, W = 32, odd sizes
SSIM_CASES = tuple(
    [(content, shape, pad) for content in ("noise", "smooth", "flat", "identical", "outside") for shape in _WIDE for pad in BOTH]
    + [("noise", (1, 1, 64, 65), pad) for pad in BOTH] + [("smooth", (1, 1, 64, 65), pad) for pad in BOTH]
    + [("noise", (2, 2, 43, 31), pad) for pad in BOTH] + [("flat", (2, 2, 43, 31), pad) for pad in BOTH]
    + [("noise", (1, 2, 11, 75), "valid"), ("smooth", (1, 2, 11, 75), "valid"),       # one counted row
       ("noise", (1, 1, 11, 11), "valid"), ("outside", (1, 1, 11, 11), "valid"),      # count = 1
       ("noise", (1, 3, 1, 1), "same"), ("outside", (1, 3, 1, 1), "same")])
LAYOUT_SHAPE = (2, 3, 33, 47)
LAYOUTS = ("nchw", "channels_last", "img2_channels_last", "img2_nchw", "crop", "hwc", "expanded")
DTYPES = (torch.float16, torch.bfloat16, torch.float64)

MS_SIZES = ((88, 91, 3, 4), (45, 47, 2, 3), (23, 22, 4, 2), (11, 11, 1, 1), (135, 181, 3, 4))     # (H, W, C, levels)
MS_WEIGHTS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.3, 2.0, 1.0))
MS_CLAMPS = ((0.0, 1.0), (-0.5, 2.0))
MS_UPSTREAM = 1.5
MS_CASES = tuple(
    [("ms_noise", size, w, MS_CLAMPS[0]) for size in MS_SIZES for w in MS_WEIGHTS]
    + [("ms_noise", size, MS_WEIGHTS[3], MS_CLAMPS[1]) for size in MS_SIZES]
    + [("ms_smooth", size, w, MS_CLAMPS[0]) for size in MS_SIZES for w in (MS_WEIGHTS[2], MS_WEIGHTS[3])])
MS_UNFUSED_SIZES = (MS_SIZES[1], MS_SIZES[3])


def case_id(case) -> str:
  return "-".join("x".join(str(v) for v in part) if isinstance(part, tuple) else str(part) for part in case)


def _gen(*key) -> torch.Generator:
  return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _box(t):
  return F.avg_pool2d(t, 3, stride=1, padding=1, count_include_pad=False)


def _pair(content: str, shape, g: torch.Generator):
  x = torch.rand(shape, generator=g)
  if content == "noise":
    return x, (x + 0.15 * torch.randn(shape, generator=g)).clamp(0, 1)
  if content == "smooth":
    x = _box(_box(x))
    return x, (x + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
  if content == "flat":
    y = torch.full(shape, 0.5)
    y[..., shape[-1] // 2:] = 0.52
    return torch.full(shape, 0.5), y
  if content == "identical":
    return x, x.clone()
  if content == "outside":
    return x * 1.6 - 0.3, torch.rand(shape, generator=g)
  raise ValueError(content)


def ssim_inputs(case, seed: int = 0):
  """(img1, img2), float32 (B,C,H,W) on the CPU."""
  content, shape, pad = case
  return _pair(content, shape, _gen(seed, *shape, CROP[pad], CONTENTS.index(content)))


def ms_inputs(case, seed: int = 0):
  """(image, target), float32 (H,W,C) on the CPU; the image leaves the clamp and touches both of its bounds."""
  content, (H, W, C, levels), weights, (lo, hi) = case
  g = _gen(seed, H, W, C, levels, CONTENTS.index(content))
  if content == "ms_noise":
    t = torch.rand(H, W, C, generator=g)
    x = t + 0.1 * torch.randn(H, W, C, generator=g) + 0.05
  else:
    x, t = _pair("smooth", (1, C, H, W), g)
    x, t = (x[0].permute(1, 2, 0) * 1.1 - 0.03).contiguous(), t[0].permute(1, 2, 0).contiguous()
  x = lo + x * (hi - lo)                                  # the same picture inside another clamp
  t = lo + t * (hi - lo) if (lo, hi) != (0.0, 1.0) else t
  flat = x.view(-1)
  flat[0], flat[flat.numel() // 2] = lo, hi               # exactly on both bounds: the gradient passes
  if flat.numel() > 8:
    flat[3], flat[5] = lo - 0.25, hi + 0.25               # and certainly outside
  return x, t


# ---- figures ----------------------------------------------------------------------------------------------------------

def deviation(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
  """|got - want| entrywise in fp64; inf where exactly one of the two is not finite, 0 where neither is."""
  got, want = got.detach().double().cpu(), want.detach().double().cpu()
  gf, wf = torch.isfinite(got), torch.isfinite(want)
  inf = torch.full_like(want, math.inf)
  return torch.where(gf & wf, (got - want).abs(), torch.where(gf == wf, torch.zeros_like(want), inf))


def ratio_max(num: torch.Tensor, den: torch.Tensor) -> float:
  """max num / den; a zero denominator has to be met by an exactly zero numerator (else inf)."""
  if num.numel() == 0:
    return 0.0
  den = den.double().cpu().expand_as(num)
  q = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, math.inf)))
  return q.max().item()


def output_rounding(want: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
  """What one rounding into ``dtype`` may move ``want`` by (zero for float32 and wider: the bound already covers it)."""
  if dtype in (torch.float16, torch.bfloat16):
    fi = torch.finfo(dtype)
    return want.abs() * (fi.eps / 2) + fi.smallest_normal * fi.eps / 2
  return torch.zeros_like(want)


def recovered_map(d_m11: torch.Tensor, ref: dict) -> torch.Tensor:
  """The SSIM map behind a derivative map d_m11 = -ssim / (s1 + s2 + C2) / count (counted region only)."""
  B2 = -ref["map"] / (ref["d_m11"] * ref["count"])         # the oracle's s1 + s2 + C2 where d_m11 != 0
  return -ref["count"] * d_m11.detach().double().cpu() * B2


def ssim_figures(got: dict, ref: dict, crop: int, grad_dtype: torch.dtype = torch.float32) -> dict:
  """``got``: any of mean, grad, d_mu1 + d_m11 + d_m12; ``ref``: ssim_oracle.ssim_terms in fp64."""
  out = {}
  if "mean" in got:
    out["mean"] = deviation(torch.as_tensor(got["mean"]).reshape(()), ref["mean"]).item()
  if "d_m11" in got:
    H, W = ref["map"].shape[-2:]
    inner = (..., slice(crop, H - crop), slice(crop, W - crop))
    out["map"] = deviation(recovered_map(got["d_m11"], ref)[inner], ref["map"][inner]).max().item()
    top = {k: ref[k].abs().max() for k in ("d_mu1", "d_m11", "d_m12")}
    if top["d_mu1"] < CANCELLED * ref["d_mu1_terms"].max():       # identical images: the map is the oracle's own rounding
      top["d_mu1"] = ref["d_mu1_terms"].max()
    out["dmaps"] = max(ratio_max(deviation(got[k], ref[k]).max().reshape(1), top[k].reshape(1)) for k in top)
  if "grad" in got:
    dev = (deviation(got["grad"], ref["grad"]) - output_rounding(ref["grad"], grad_dtype)).clamp_min(0)
    out["grad"] = ratio_max(dev, ref["scale"])
  return out


def ms_figures(got: dict, ref: dict, upstream: float = 1.0) -> dict:
  """``got``: metrics (3 + levels entries) and / or grad (H,W,C) of ``upstream`` x loss; ``ref``: multiscale_terms."""
  out = {}
  if "metrics" in got:
    want = torch.stack([ref["loss"], ref["l1"], ref["mse"]] + list(ref["ssim"])).double()
    out["levels"] = (deviation(got["metrics"], want) / want.abs().clamp_min(1.0).nan_to_num(1.0)).max().item()
  if "grad" in got:
    out["grad"] = ratio_max(deviation(got["grad"], upstream * ref["grad"]), abs(upstream) * ref["scale"])
  return out


def outside(content: str, figs: dict) -> list:
  return [(k, v, bound(content, k)) for k, v in figs.items() if not v <= bound(content, k)]


def old_criterion(got_grad: torch.Tensor, want_grad: torch.Tensor) -> float:
  """tests/test_ssim.py's: the largest gradient error over the image's largest gradient entry (against 1e-4)."""
  return ratio_max(deviation(got_grad, want_grad).max().reshape(1), want_grad.abs().max().reshape(1))


# ---- the float32 model and its planted deviations -----------------------------------------------------------------------

def _window(taps: int = 11, normalised: bool = True) -> torch.Tensor:
  x = torch.arange(taps, dtype=torch.float64) - taps // 2
  g = torch.exp(-(x * x) / (2 * so.SIGMA ** 2))
  return g / g.sum() if normalised else g


def model_ssim(x: torch.Tensor, y: torch.Tensor, crop: int, defect: str = None, form: str = "separable") -> dict:
  """fused_ssim's stage in float32 torch (ssim_oracle.ssim_terms on float32 inputs), optionally with one deviation."""
  x, y = x.float(), y.float()
  B, C, H, W = x.shape
  window = None
  if defect in ("crop4", "crop6"):
    crop = crop - 1 if defect == "crop4" else crop + 1
  if defect == "window9":
    window = _window(9)
  if defect == "unnormalised":
    window = _window(11, normalised=False)
  if defect == "planes_swapped":                          # img2's plane (p % B, p // B) read in place of (p // C, p % C)
    p = torch.arange(B * C)
    y = y.reshape(B * C, H, W)[(p % B) * C + p // B].reshape(B, C, H, W)
  t = so.ssim_terms(x, y, crop, window=window, form=form)
  if defect == "factor2":
    t["grad"] = (so.blur(t["d_mu1"], window, form) + x * so.blur(t["d_m11"], window, form) + y * so.blur(t["d_m12"], window, form))
  if defect == "tile_row":                                # the last row of every 32-row tile keeps what was there: zeros
    t["grad"] = t["grad"].clone()
    t["grad"][:, :, 31::32, :] = 0.0
  return dict(mean=t["mean"], grad=t["grad"], d_mu1=t["d_mu1"], d_m11=t["d_m11"], d_m12=t["d_m12"])


def model_loss(image: torch.Tensor, target: torch.Tensor, levels: int, weights, clamp, defect: str = None,
               form: str = "separable") -> dict:
  """reference_loss's stage in float32 torch, composed the way csrc/ssim.hip composes it, optionally with one deviation."""
  img, t = image.float(), target.float()
  lo, hi = clamp
  H, W, C = img.shape
  w_l1, w_mse, w_ssim = weights
  src = torch.where(torch.isnan(img), torch.full_like(img, lo), img) if defect == "nan_to_lo" else img
  x = src.clamp(lo, hi)
  passes = ((src > lo) & (src < hi)) if defect == "exclusive_mask" else ((src >= lo) & (src <= hi))
  d = x - t
  n = d.numel()
  l1, mse = d.abs().mean(), (d * d).mean()
  grad = w_l1 * torch.sign(d) / n + w_mse * 2 * d / n
  px, pt = x.permute(2, 0, 1)[None], t.permute(2, 0, 1)[None]
  ssims = []
  for l in range(levels):
    if l:
      ceil = defect == "pool_ceil"
      px, pt = (F.avg_pool2d(px, 2, 2, ceil_mode=ceil), F.avg_pool2d(pt, 2, 2, ceil_mode=ceil))
    terms = so.ssim_terms(px, pt, crop=5, form=form)
    ssims.append(terms["mean"])
    shift = 1 if (defect == "level2_shift1" and l == 2) else l
    g = terms["grad"][0].permute(1, 2, 0)
    ys, xs = (torch.arange(H) >> shift), (torch.arange(W) >> shift)
    ok = (ys < g.shape[0])[:, None] & (xs < g.shape[1])[None, :]
    routed = g[ys.clamp_max(g.shape[0] - 1)][:, xs.clamp_max(g.shape[1] - 1)]
    routed = torch.where(ok[..., None], routed, torch.zeros_like(routed))
    grad = grad - (w_ssim / levels) * 0.25 ** l * routed
  loss = w_l1 * l1 + w_mse * mse + w_ssim * sum(1.0 - s for s in ssims) / levels
  return dict(metrics=torch.stack([loss, l1, mse] + ssims), grad=torch.where(passes, grad, torch.zeros_like(grad)))


SSIM_DEFECTS = ("crop4", "crop6", "window9", "unnormalised", "planes_swapped", "factor2", "tile_row")
MS_DEFECTS = ("level2_shift1", "pool_ceil", "exclusive_mask", "nan_to_lo")
