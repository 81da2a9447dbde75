"""The loss stage's contract on the CPU (loss_contract.py): the oracle's explicit terms against autograd, the NOISE table
re-measured (float32 oracle against float64 oracle, both forms, every case and seed), and planted deviations of a
float32 model of the stage, each of which has to leave its bound on a named case -- next to what the former global
criterion (largest gradient error over the image's largest gradient entry, 1e-4) makes of the same deviation.
profiles/r29_loss_contract.txt keeps a run's output."""
import math

import pytest
import torch
import torch.nn.functional as F

import loss_contract as lc
from oracle import ssim_oracle as so


def _ref_ssim(case, seed=0):
  x, y = lc.ssim_inputs(case, seed)
  return x, y, so.ssim_terms(x.double(), y.double(), lc.CROP[case[2]])


def _ref_ms(case, seed=0):
  x, t = lc.ms_inputs(case, seed)
  return x, t, so.multiscale_terms(x.double(), t.double(), case[1][3], case[2], case[3])


@pytest.mark.parametrize("form", lc.FORMS)
def test_explicit_gradient_is_autograds(form):
  """ssim_terms / multiscale_terms in fp64: gradient, mean and map against the differentiable oracle within 1e-12."""
  for case in (("noise", (2, 3, 19, 23), "same"), ("smooth", (2, 3, 19, 23), "valid"), ("outside", (1, 2, 11, 13), "valid")):
    x, y = lc.ssim_inputs(case)
    xg = x.double().requires_grad_(True)
    m = so.fused_ssim(xg, y.double(), case[2])
    m.backward()
    t = so.ssim_terms(x.double(), y.double(), lc.CROP[case[2]], form=form)
    assert (t["grad"] - xg.grad).abs().max().item() < 1e-12 and abs(t["mean"].item() - m.item()) < 1e-12
    assert (t["map"] - so.ssim_map(x.double(), y.double())).abs().max().item() < 1e-12
    assert (t["scale"] >= t["grad"].abs() * (1 - 1e-12)).all()
    outside = torch.ones_like(x, dtype=torch.bool)
    c = lc.CROP[case[2]]
    outside[:, :, c:x.shape[2] - c, c:x.shape[3] - c] = False
    assert all((t[k][outside] == 0).all() for k in ("d_mu1", "d_m11", "d_m12"))
  for case in (("ms_noise", (45, 47, 2, 3), (0.3, 2.0, 1.0), (0.0, 1.0)), ("ms_smooth", (23, 22, 4, 2), (0.3, 2.0, 1.0), (-0.5, 2.0))):
    x, t = lc.ms_inputs(case)
    xg = x.double().requires_grad_(True)
    img = xg.clamp(*case[3])
    ssim_l, s0 = so.multiscale_ssim_loss(img, t.double(), levels=case[1][3])
    w = case[2]
    loss = w[0] * F.l1_loss(img, t.double()) + w[1] * F.mse_loss(img, t.double()) + w[2] * ssim_l
    loss.backward()
    r = so.multiscale_terms(x.double(), t.double(), case[1][3], w, case[3], form=form)
    assert (r["grad"] - xg.grad).abs().max().item() < 1e-12 and abs(r["loss"].item() - loss.item()) < 1e-12
    assert abs(r["ssim"][0].item() - s0.item()) < 1e-12
    blocked = (x < case[3][0]) | (x > case[3][1])
    assert blocked.any() and (r["grad"][blocked] == 0).all() and (r["scale"][blocked] == 0).all()
    assert (r["scale"] >= r["grad"].abs() * (1 - 1e-12)).all()


def _measure_noise():
  worst, fixed = {}, {}

  def take(content, figs):
    for k, v in figs.items():
      if (content, k) in lc.NOISE:
        worst[(content, k)] = max(worst.get((content, k), 0.0), v)
      else:
        fixed[(content, k)] = max(fixed.get((content, k), 0.0), v)

  for seed in lc.SEEDS:
    for case in lc.SSIM_CASES:
      x, y, ref = _ref_ssim(case, seed)
      for form in lc.FORMS:
        take(case[0], lc.ssim_figures(so.ssim_terms(x, y, lc.CROP[case[2]], form=form), ref, lc.CROP[case[2]]))
    for case in lc.MS_CASES:
      x, t, ref = _ref_ms(case, seed)
      for form in lc.FORMS:
        got = so.multiscale_terms(x, t, case[1][3], case[2], case[3], form=form)
        metrics = torch.stack([got["loss"], got["l1"], got["mse"]] + list(got["ssim"]))
        take(case[0], lc.ms_figures(dict(grad=got["grad"], metrics=metrics), ref))
  for key in sorted(fixed):
    print(f"NOISE {key}: measured {fixed[key]:.3e}; fixed bound {lc.bound(*key):.1e}")
  return worst


def _round_up_two_digits(v: float) -> float:
  e = math.floor(math.log10(v)) - 1
  return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


def test_noise_table():
  """Every entry of NOISE covers what is measured now and is not more than four times it (a stale table)."""
  worst = _measure_noise()
  assert set(worst) == set(lc.NOISE)
  bad = []
  for key in sorted(lc.NOISE):
    print(f"NOISE {key}: measured {worst[key]:.3e} -> {_round_up_two_digits(worst[key]):.1e}, table {lc.NOISE[key]:.1e}, "
          f"bound {lc.bound(*key):.1e}")
    if not (lc.NOISE[key] / 4 <= worst[key] <= lc.NOISE[key]):
      bad.append((key, worst[key], lc.NOISE[key]))
  assert not bad, bad


# every deviation with the cases it is looked for on (the first that leaves a bound is named)
_S = lambda content, shape, pad: (content, shape, pad)
DEFECT_CASES = {
  "crop4": [_S("noise", (2, 3, 33, 47), "valid"), _S("smooth", (1, 2, 11, 75), "valid")],
  "crop6": [_S("noise", (2, 3, 33, 47), "valid")],
  "window9": [_S("noise", (2, 3, 33, 47), "same"), _S("smooth", (3, 2, 37, 32), "valid")],
  "unnormalised": [_S("noise", (2, 3, 33, 47), "same")],
  "planes_swapped": [_S("noise", (1, 3, 1, 1), "same"), _S("noise", (1, 1, 64, 65), "same"), _S("noise", (2, 3, 33, 47), "same")],
  "factor2": [_S("noise", (2, 3, 33, 47), "valid"), _S("identical", (3, 2, 37, 32), "same")],
  "tile_row": [_S("noise", (2, 2, 43, 31), "same"), _S("noise", (3, 2, 37, 32), "valid")],
  "level2_shift1": [("ms_noise", (88, 91, 3, 4), (0.3, 2.0, 1.0), (0.0, 1.0))],
  "pool_ceil": [("ms_noise", (88, 91, 3, 4), (0.0, 0.0, 1.0), (0.0, 1.0)), ("ms_noise", (45, 47, 2, 3), (0.3, 2.0, 1.0), (0.0, 1.0))],
  "exclusive_mask": [("ms_noise", (11, 11, 1, 1), (0.3, 2.0, 1.0), (0.0, 1.0))],
  "nan_to_lo": [("ms_noise", (23, 22, 4, 2), (0.3, 2.0, 1.0), (0.0, 1.0))],
}


def _defect_figures(defect, case):
  """(figures of the deviating model, of the sound model, the old criterion of the deviating model)."""
  if defect in lc.SSIM_DEFECTS:
    x, y, ref = _ref_ssim(case)
    crop = lc.CROP[case[2]]
    bad, good = lc.model_ssim(x, y, crop, defect), lc.model_ssim(x, y, crop)
    return lc.ssim_figures(bad, ref, crop), lc.ssim_figures(good, ref, crop), lc.old_criterion(bad["grad"], ref["grad"])
  x, t = lc.ms_inputs(case)
  if defect == "nan_to_lo":
    x[x.shape[0] // 2, x.shape[1] // 2, 0] = float("nan")
  ref = so.multiscale_terms(x.double(), t.double(), case[1][3], case[2], case[3])
  bad, good = (lc.model_loss(x, t, case[1][3], case[2], case[3], d) for d in (defect, None))
  up = lc.MS_UPSTREAM
  scaled = lambda m: dict(metrics=m["metrics"], grad=up * m["grad"])
  return lc.ms_figures(scaled(bad), ref, up), lc.ms_figures(scaled(good), ref, up), lc.old_criterion(up * bad["grad"], up * ref["grad"])


@pytest.mark.parametrize("defect", lc.SSIM_DEFECTS + lc.MS_DEFECTS)
def test_planted_defect_leaves_its_bound(defect):
  """The sound float32 model is inside every bound on the defect's cases; the deviating one leaves a bound on one."""
  caught = None
  for case in DEFECT_CASES[defect]:
    bad, good, old = _defect_figures(defect, case)
    assert not lc.outside(case[0], good), (case, lc.outside(case[0], good))
    for figure, v in bad.items():
      b = lc.bound(case[0], figure)
      share = v / b if b > 0 else (0.0 if v == 0 else math.inf)
      print(f"DEFECT {defect} {lc.case_id(case)} {figure}: {v:.3e} = {share:.3g} x bound {b:.1e}")
    print(f"DEFECT {defect} {lc.case_id(case)} old criterion: {old:.3e} ({'caught' if not old < 1e-4 else 'LET THROUGH'} at 1e-4)")
    if caught is None and lc.outside(case[0], bad):
      caught = (case, lc.outside(case[0], bad))
  assert caught is not None, defect
  print(f"DEFECT {defect} caught on {lc.case_id(caught[0])}: {[k for k, _, _ in caught[1]]}")
  if defect == "planes_swapped":          # with B = 1 or C = 1 the mix-up is invisible: what the former shapes were
    for case in DEFECT_CASES[defect][:2]:
      assert not lc.outside(case[0], _defect_figures(defect, case)[0])
