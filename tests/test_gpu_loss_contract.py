"""csrc/ssim.hip against oracle/ssim_oracle.py in fp64, per pixel (loss_contract.py: cases, figures, bounds = 4 x the
float32 oracle's own noise; tests/test_loss_contract_host.py measures that noise and shows that the figures discriminate).

Through fused_ssim (mean and gradient), gsr_ssim_forward (the three derivative maps, and the map behind them),
reference_loss (fused and composed: every metrics entry and the gradient), clamped_mse_loss / clamped_l1_loss; layouts
that differ between the two images, views with an offset and padded rows, a prediction expanded over the batch, float16 /
bfloat16 / float64 predictions, NaN and +inf pixels, and every case twice for bit-equality.  Every figure is printed
next to its bound."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import loss_contract as lc
from oracle import ssim_oracle as so

pytestmark = pytest.mark.gpu


def _report(label, content, figs):
  for k, v in figs.items():
    b = lc.bound(content, k)
    print(f"CONTRACT {label} {k}: {v:.3e} (bound {b:.1e}, {v / b if b > 0 else math.inf:.2f} of it)")
  bad = lc.outside(content, figs)
  assert not bad, (label, bad)


@functools.lru_cache(maxsize=None)
def _ssim_ref(case):
  x, y = lc.ssim_inputs(case)
  return x, y, so.ssim_terms(x.double(), y.double(), lc.CROP[case[2]])


@functools.lru_cache(maxsize=None)
def _ms_ref(case):
  x, t = lc.ms_inputs(case)
  return x, t, so.multiscale_terms(x.double(), t.double(), case[1][3], case[2], case[3])


def _forward_maps(x, y, crop):
  """gsr_ssim_forward as fused_ssim calls it: (mean, d_mu1, d_m11, d_m12) of two float32 device tensors."""
  import ctypes as C
  from splat_trainer_amd import _lib
  from splat_trainer_amd._lib import current_stream_ptr, ptr
  B, Cc, H, W = x.shape
  mean = torch.empty(1, dtype=torch.float32, device=x.device)
  maps = torch.full((3, B, Cc, H, W), float("nan"), dtype=torch.float32, device=x.device)
  ws = _lib.workspace(_lib.load().gsr_ssim_workspace_bytes(B, Cc, H, W), x.device)
  _lib.call("gsr_ssim_forward", ptr(x), ptr(y), (C.c_int64 * 4)(*x.stride()), (C.c_int64 * 4)(*y.stride()), B, Cc, H, W, crop,
            ptr(mean), ptr(maps[0]), ptr(maps[1]), ptr(maps[2]), ptr(ws), ws.numel(), current_stream_ptr())
  torch.cuda.synchronize()
  return mean[0].cpu(), maps[0].cpu(), maps[1].cpu(), maps[2].cpu()


def _run_ssim(a, b, leaf, padding):
  import splat_trainer_amd as sta
  leaf.grad = None
  got = sta.fused_ssim(a, b, padding=padding)
  assert got.dim() == 0
  got.backward()
  return got.detach().cpu(), leaf.grad.clone()


@pytest.mark.parametrize("case", lc.SSIM_CASES, ids=lc.case_id)
def test_fused_ssim_per_pixel(case):
  """The derivative maps (gsr_ssim_forward), the map behind them and the gradient (fused_ssim), twice for bit-equality."""
  content, shape, padding = case
  x, y, ref = _ssim_ref(case)
  crop = lc.CROP[padding]
  xd, yd = x.cuda().requires_grad_(True), y.cuda()
  mean, grad = _run_ssim(xd, yd, xd, padding)
  assert grad.dtype is torch.float32 and grad.shape == x.shape
  fwd = _forward_maps(xd.detach(), yd, crop)
  assert fwd[0].item() == mean.item()
  _report(lc.case_id(case), content, lc.ssim_figures(dict(grad=grad, d_mu1=fwd[1], d_m11=fwd[2], d_m12=fwd[3]), ref, crop))
  mean2, grad2 = _run_ssim(xd, yd, xd, padding)
  fwd2 = _forward_maps(xd.detach(), yd, crop)
  assert mean2.item() == mean.item() and torch.equal(grad, grad2) and all(torch.equal(p, q) for p, q in zip(fwd, fwd2))


@pytest.mark.parametrize("case", lc.SSIM_CASES, ids=lc.case_id)
def test_fused_ssim_mean(case):
  """The scalar against the oracle within 2e-6, the bound tests/test_ssim.py has always used, on every case.  Near-flat
  content is the hard one: with plain moments G*x^2 - mu1^2 leaves the same 1e-7 at every interior pixel against
  C2 = 9e-4 and the mean was off by 2.4e-5 .. 5.3e-5; ssim_fwd's shifted moments bring it below 1e-7."""
  content, shape, padding = case
  x, y, ref = _ssim_ref(case)
  xd = x.cuda().requires_grad_(True)
  mean, _ = _run_ssim(xd, y.cuda(), xd, padding)
  _report("mean-" + lc.case_id(case), content, lc.ssim_figures(dict(mean=mean), ref, lc.CROP[padding]))


@pytest.mark.parametrize("padding", lc.BOTH)
@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_fused_ssim_layouts(layout, padding):
  """The two images in different layouts, a view with an offset and padded rows, the reference's (H,W,C) view, and one
  image expanded over the batch (its gradient is the sum over the batch)."""
  case = ("noise", lc.LAYOUT_SHAPE, padding)
  x, y, ref = _ssim_ref(case)
  B, C, H, W = x.shape
  crop = lc.CROP[padding]
  cl = torch.channels_last
  back = lambda g: g
  if layout in ("nchw", "channels_last", "img2_channels_last", "img2_nchw"):
    leaf = x.cuda().to(memory_format=cl if layout in ("channels_last", "img2_nchw") else torch.contiguous_format).requires_grad_(True)
    a, b = leaf, y.cuda().to(memory_format=cl if layout in ("channels_last", "img2_channels_last") else torch.contiguous_format)
    assert (a.stride() == b.stride()) == (layout in ("nchw", "channels_last"))
  elif layout == "crop":
    big = torch.rand(B, C, H + 2, W + 5)
    big[..., 1:-1, 2:-3] = x
    leaf = big.cuda().requires_grad_(True)
    bigy = torch.rand(B, C, H + 4, W + 3)
    bigy[..., 3:-1, 1:-2] = y
    a, b = leaf[..., 1:-1, 2:-3], bigy.cuda()[..., 3:-1, 1:-2]
    assert a.storage_offset() > 0 and not a.is_contiguous()
    back = lambda g: g[..., 1:-1, 2:-3]
  elif layout == "hwc":
    ref = so.ssim_terms(x[:1].double(), y[:1].double(), crop)
    leaf = x[0].permute(1, 2, 0).contiguous().cuda().requires_grad_(True)
    a, b = leaf.unsqueeze(0).permute(0, 3, 1, 2), y[0].permute(1, 2, 0).contiguous().cuda().unsqueeze(0).permute(0, 3, 1, 2)
    back = lambda g: g.permute(2, 0, 1).unsqueeze(0)
  else:
    xe = x[:1].expand(B, C, H, W)
    ref = so.ssim_terms(xe.double(), y.double(), crop)
    ref = dict(ref, grad=ref["grad"].sum(0, keepdim=True), scale=ref["scale"].sum(0, keepdim=True))
    leaf = x[:1].cuda().requires_grad_(True)
    a, b = leaf.expand(B, C, H, W), y.cuda()
    assert a.stride(0) == 0
  mean, grad = _run_ssim(a, b, leaf, padding)
  if layout == "crop":
    rim = torch.ones_like(grad, dtype=torch.bool)
    rim[..., 1:-1, 2:-3] = False
    assert (grad[rim] == 0).all()
  _report(f"{layout}-{padding}", "noise", lc.ssim_figures(dict(mean=mean, grad=back(grad)), ref, crop))
  mean2, grad2 = _run_ssim(a, b, leaf, padding)
  assert mean2.item() == mean.item() and torch.equal(grad, grad2)


@pytest.mark.parametrize("dtype", lc.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_fused_ssim_dtypes(dtype):
  """A float16 / bfloat16 / float64 prediction: computed on its float32-cast values, gradient in its own dtype."""
  case = ("noise", lc.LAYOUT_SHAPE, "valid")
  x, y = lc.ssim_inputs(case)
  leaf = x.to(dtype).cuda().requires_grad_(True)
  ref = so.ssim_terms(x.to(dtype).to(torch.float32).double(), y.double(), 5)
  mean, grad = _run_ssim(leaf, y.cuda(), leaf, "valid")
  assert grad.dtype is dtype
  _report(f"dtype-{dtype}", "noise", lc.ssim_figures(dict(mean=mean, grad=grad), ref, 5, grad_dtype=dtype))
  mean2, grad2 = _run_ssim(leaf, y.cuda(), leaf, "valid")
  assert mean2.item() == mean.item() and torch.equal(grad, grad2)


def _run_loss(x, t, case, fused=True):
  import splat_trainer_amd as sta
  _, (H, W, C, levels), w, clamp = case
  leaf = x.clone().cuda().requires_grad_(True)
  loss, metrics = sta.reference_loss(leaf, t.cuda(), l1_weight=w[0], mse_weight=w[1], ssim_weight=w[2], ssim_levels=levels,
                                     clamp=clamp, fused=fused, return_metrics=True)
  (loss * lc.MS_UPSTREAM).backward()
  assert metrics.shape == (3 + levels,) and (loss.item() == metrics[0].item() or not math.isfinite(loss.item()))
  return dict(metrics=metrics.detach().cpu(), grad=leaf.grad.cpu())


@pytest.mark.parametrize("case", lc.MS_CASES, ids=lc.case_id)
def test_reference_loss_per_pixel(case):
  """The fused loss: every metrics entry (the per-level SSIM values included) and the gradient of 1.5 x loss."""
  x, t, ref = _ms_ref(case)
  got = _run_loss(x, t, case)
  _report(lc.case_id(case), case[0], lc.ms_figures(got, ref, lc.MS_UPSTREAM))
  again = _run_loss(x, t, case)
  assert torch.equal(got["metrics"], again["metrics"]) and torch.equal(got["grad"], again["grad"])


@pytest.mark.parametrize("size", lc.MS_UNFUSED_SIZES, ids=lc.case_id)
@pytest.mark.parametrize("clamp", lc.MS_CLAMPS, ids=lc.case_id)
def test_composed_reference_loss_per_pixel(size, clamp):
  case = ("ms_noise", size, lc.MS_WEIGHTS[3], clamp)
  x, t, ref = _ms_ref(case)
  got = _run_loss(x, t, case, fused=False)
  _report("composed-" + lc.case_id(case), case[0], lc.ms_figures(got, ref, lc.MS_UPSTREAM))
  again = _run_loss(x, t, case, fused=False)
  assert torch.equal(got["metrics"], again["metrics"]) and torch.equal(got["grad"], again["grad"])


@pytest.mark.parametrize("size", lc.MS_SIZES, ids=lc.case_id)
@pytest.mark.parametrize("clamp", lc.MS_CLAMPS, ids=lc.case_id)
def test_pixel_losses_per_pixel(size, clamp):
  """clamped_l1_loss / clamped_mse_loss on the loss cases: the oracle's l1 / mse terms alone (one level, zero weights)."""
  import splat_trainer_amd as sta
  for kind, fn in enumerate((sta.clamped_l1_loss, sta.clamped_mse_loss)):
    w = (1.0, 0.0, 0.0) if kind == 0 else (0.0, 1.0, 0.0)
    case = ("ms_noise", size, w, clamp)
    x, t = lc.ms_inputs(case)
    ref = so.multiscale_terms(x.double(), t.double(), 1, w, clamp)
    runs = []
    for _ in range(2):
      leaf = x.clone().cuda().requires_grad_(True)
      loss = fn(leaf, t.cuda(), clamp=clamp)
      (loss * lc.MS_UPSTREAM).backward()
      runs.append((loss.detach().cpu(), leaf.grad.cpu()))
    want = ref["l1"] if kind == 0 else ref["mse"]
    figs = dict(levels=lc.deviation(runs[0][0], want).item() / max(1.0, abs(want.item())),
                grad=lc.ms_figures(dict(grad=runs[0][1]), ref, lc.MS_UPSTREAM)["grad"])
    _report(f"{fn.__name__}-{lc.case_id(case)}", "ms_noise", figs)
    assert runs[0][0].item() == runs[1][0].item() and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("offset", (0, 1))
@pytest.mark.parametrize("n", range(1, 10))
def test_pixel_losses_short_and_offset(n, offset):
  """n = 1..9 (the four-wide loads' tail) and a contiguous view that starts one element into its buffer, which is not
  16-byte aligned: value and gradient of both losses against the torch expression in fp64."""
  import splat_trainer_amd as sta
  g = torch.Generator().manual_seed(100 + n)
  x0 = torch.rand(n + 1, generator=g) * 1.6 - 0.3
  t0 = torch.rand(n + 1, generator=g)
  x0[offset] = 1.0                                         # on the bound: the gradient passes
  for fn, ref_fn in ((sta.clamped_mse_loss, F.mse_loss), (sta.clamped_l1_loss, F.l1_loss)):
    buf = x0.clone().cuda().requires_grad_(True)
    a, t = buf[offset:offset + n], t0.cuda()[offset:offset + n]
    assert a.is_contiguous() and (a.data_ptr() % 16 != 0) == (offset == 1)
    (fn(a, t) * 3.0).backward()
    xo = x0.double().requires_grad_(True)
    want = ref_fn(xo[offset:offset + n].clamp(0, 1), t0.double()[offset:offset + n]) * 3.0
    want.backward()
    got = fn(a.detach(), t)
    assert abs(got.item() * 3.0 - want.item()) <= 2e-6 * max(1.0, abs(want.item())), (got.item() * 3.0, want.item())
    assert torch.allclose(buf.grad.cpu().double(), xo.grad, rtol=1e-6, atol=1e-12), (buf.grad.cpu(), xo.grad)


def _same_non_finite(got: float, want: float) -> bool:
  return (math.isnan(got) and math.isnan(want)) or got == want or (math.isfinite(got) and math.isfinite(want))


@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_non_finite_pixel_through_fused_ssim(bad):
  """A NaN / +inf pixel in the prediction: the mean is what the torch expression gives (not finite), the gradient equals
  the oracle's wherever the oracle's is finite, which is everywhere outside the pixel's window of influence."""
  case = ("noise", (2, 2, 43, 31), "same")
  x, y = lc.ssim_inputs(case)
  x = x.clone()
  x[1, 0, 20, 13] = bad
  ref = so.ssim_terms(x.double(), y.double(), 0)
  assert not math.isfinite(ref["mean"].item())
  leaf = x.cuda().requires_grad_(True)
  mean, grad = _run_ssim(leaf, y.cuda(), leaf, "same")
  assert _same_non_finite(mean.item(), ref["mean"].item()) and not math.isfinite(mean.item()), (mean.item(), ref["mean"].item())
  fine = torch.isfinite(ref["grad"])
  far = torch.ones_like(fine)
  far[1, 0, 10:31, 3:24] = False                          # two windows: the map's, then the gradient's
  assert (fine | ~far).all() and fine[0].all() and fine[1, 1].all()
  e = lc.ratio_max(lc.deviation(grad, ref["grad"])[fine], ref["scale"][fine])
  print(f"CONTRACT non-finite-{bad} fused_ssim grad at finite pixels: {e:.3e} (bound {lc.bound('noise', 'grad'):.1e})")
  assert e <= lc.bound("noise", "grad")


@pytest.mark.parametrize("fused", (True, False), ids=("fused", "composed"))
@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_non_finite_pixel_through_reference_loss(bad, fused):
  """Under the clamp a NaN stays a NaN (loss and the per-level values it reaches are NaN, as F.mse_loss(image.clamp(0, 1), t)
  and the oracle give: the trainer's non-finite guard relies on it); +inf clamps to 1 and everything stays finite."""
  case = ("ms_noise", (45, 47, 2, 3), lc.MS_WEIGHTS[3], lc.MS_CLAMPS[0])
  x, t = lc.ms_inputs(case)
  x = x.clone()
  x[22, 30, 1] = bad
  ref = so.multiscale_terms(x.double(), t.double(), 3, case[2], case[3])
  torch_loss = F.mse_loss(x.double().clamp(0, 1), t.double()).item()
  assert math.isfinite(torch_loss) == math.isfinite(ref["loss"].item()) == (bad == float("inf"))
  got = _run_loss(x, t, case, fused=fused)
  want = torch.stack([ref["loss"], ref["l1"], ref["mse"]] + list(ref["ssim"]))
  assert all(_same_non_finite(g, w) for g, w in zip(got["metrics"].tolist(), want.tolist())), (got["metrics"], want)
  fine = torch.isfinite(ref["grad"])
  assert fine[..., 0].all() and fine.sum() > 0
  e = lc.ratio_max(lc.deviation(got["grad"], lc.MS_UPSTREAM * ref["grad"])[fine], lc.MS_UPSTREAM * ref["scale"][fine])
  print(f"CONTRACT non-finite-{bad} reference_loss grad at finite pixels: {e:.3e} (bound {lc.bound('ms_noise', 'grad'):.1e})")
  assert e <= lc.bound("ms_noise", "grad")
  if bad == float("inf"):
    _report(f"inf-{'fused' if fused else 'composed'}", "ms_noise", lc.ms_figures(got, ref, lc.MS_UPSTREAM))


@pytest.mark.parametrize("clamp", ((0.0, 1.0), None), ids=("clamped", "unclamped"))
@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_non_finite_pixel_through_pixel_losses(bad, clamp):
  """clamped_mse_loss / clamped_l1_loss: the loss is non-finite exactly when F.*_loss(image.clamp(...), t) is, and every
  other pixel's gradient is that expression's."""
  import splat_trainer_amd as sta
  g = torch.Generator().manual_seed(7)
  x0 = torch.rand(37, 5, generator=g) * 1.6 - 0.3
  t0 = torch.rand(37, 5, generator=g)
  x0[11, 2] = bad
  others = torch.ones_like(x0, dtype=torch.bool)
  others[11, 2] = False
  for fn, ref_fn in ((sta.clamped_mse_loss, F.mse_loss), (sta.clamped_l1_loss, F.l1_loss)):
    leaf = x0.clone().cuda().requires_grad_(True)
    loss = fn(leaf, t0.cuda(), clamp=clamp)
    loss.backward()
    xo = x0.double().requires_grad_(True)
    want = ref_fn(xo.clamp(*clamp) if clamp is not None else xo, t0.double())
    want.backward()
    assert _same_non_finite(loss.item(), want.item()), (fn.__name__, loss.item(), want.item())
    if math.isfinite(want.item()):
      assert abs(loss.item() - want.item()) <= 2e-6 * max(1.0, abs(want.item()))
    assert torch.allclose(leaf.grad.cpu().double()[others], xo.grad[others], rtol=1e-6, atol=1e-12)
