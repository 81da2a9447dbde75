"""CPU checks of the evaluation pass: the fp64 oracle of the colour fit against the reference's recorded results
(tests/golden/color_fit_ref.npz), the shared maths of csrc/gsr_eval.h through the host shim -- the moments, the
rank-revealing solve on full-rank and rank-deficient systems, the whole fit in the device's order of operations -- and
the argument checks of the Python layer."""
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

import color_fit_oracle as cfo
import hostmath
from helpers import PARITY_LOG

EPS = 0.5 / 255


@pytest.fixture(scope="module")
def fixtures(golden_dir):
  return cfo.load_golden(os.path.join(golden_dir, "color_fit_ref.npz"))


@pytest.fixture(scope="module")
def shim(built_libs):
  return hostmath.load(built_libs)


def _host_fit(shim, img, ref, num_iters=5):
  x, r = np.ascontiguousarray(img, np.float32), np.ascontiguousarray(ref, np.float32)
  out = np.zeros_like(x)
  shim.hm_color_fit(x, r, x.size // 3, num_iters, EPS, out)
  return out


def _host_solve(shim, sums):
  sums = np.ascontiguousarray(sums, np.float64)
  w = np.zeros(10)
  shim.hm_color_fit_solve(sums, w)
  return w


def test_fixtures_are_as_the_generator_promises(fixtures):
  assert [f["img"].shape for f in fixtures] == [(12, 11, 3), (24, 40, 3), (37, 53, 3)]
  for f in fixtures:
    clipped = np.mean((f["img"] < EPS) | (f["img"] > 1 - EPS))
    assert 0.10 <= clipped <= 0.15, clipped
    assert f["threshold_distance"] >= 1e-5 and f["eig_ratio"] >= 1e-6
    assert f["img"].dtype == np.float32 and f["out32"].dtype == np.float32 and f["out64"].dtype == np.float64
  tol = cfo.golden_tolerance(fixtures)
  assert 4 * 1e-7 < tol < 4 * 2e-6, tol          # the reference's own fp32 run sits a few 1e-7 from its fp64 run


@pytest.mark.parametrize("form", ["lstsq", "pinv"])
def test_oracle_equals_the_reference_in_fp64(fixtures, form):
  for f in fixtures:
    got, info = cfo.fit(f["img"], f["ref"], form=form)
    err = np.abs(got - f["out64"]).max()
    print(f"{f['img'].shape} {form}: max |oracle - golden fp64| {err:.2e}, threshold distance "
          f"{info['threshold_distance']:.2e}, eigenvalue ratio {info['eig_ratio']:.2e}")
    assert err <= 1e-12, err
    assert abs(info["threshold_distance"] - f["threshold_distance"]) <= 1e-12
    assert info["threshold_distance"] >= 1e-5


def test_host_moments_match_the_oracle(shim, fixtures):
  f = fixtures[1]
  x0 = np.ascontiguousarray(f["img"].reshape(-1, 3))
  ref = np.ascontiguousarray(f["ref"].reshape(-1, 3))
  x = np.ascontiguousarray(cfo.fit(f["img"], f["ref"], num_iters=2)[0].reshape(-1, 3).astype(np.float32))
  got = np.zeros((3, 45))
  shim.hm_color_fit_moments(x0, x, ref, x0.shape[0], EPS, got)
  want = cfo.moments(x0, x, ref, EPS)
  assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
  S, t = cfo.system_from_sums(got[0])
  assert np.array_equal(S, S.T) and S[9, 9] == round(S[9, 9]) and 0 < S[9, 9] <= x0.shape[0]     # S[9][9] counts the rows


def _systems(fixtures):
  """name -> (45 sums, number of eigenvalues the rule drops)."""
  f = fixtures[2]
  x0, ref = f["img"].reshape(-1, 3), f["ref"].reshape(-1, 3)
  grey = np.repeat(x0[:, :1], 3, axis=1)
  zero = x0.copy()
  zero[:, 1] = 0.0
  # a mask is taken on the channel itself, so the zero channel is looked at through channel 0's system
  return {"full": (cfo.moments(x0, x0, ref, EPS)[0], 0), "grey": (cfo.moments(grey, grey, ref, EPS)[0], 7),
          "zero_channel": (cfo.moments(zero, zero, ref, EPS)[0], 4)}


@pytest.mark.parametrize("name", ["full", "grey", "zero_channel"])
def test_host_solve_matches_pinv_with_the_same_cut(shim, fixtures, name):
  sums, n_dropped = _systems(fixtures)[name]
  S, t = cfo.system_from_sums(sums)
  d = np.diag(S)
  s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0)
  Ss = S * s[:, None] * s[None, :]
  lam = np.linalg.eigvalsh(Ss)
  dropped = lam[lam <= cfo.RANK_CUT * lam.max()]
  assert len(dropped) == n_dropped, (name, lam)
  # the cut is never ambiguous: what is dropped lies far below it, what is kept far above
  assert all(abs(v) < 1e-11 * lam.max() for v in dropped), (name, lam)
  assert lam[lam > cfo.RANK_CUT * lam.max()].min() > 1e-7 * lam.max(), (name, lam)
  want = s * (np.linalg.pinv(Ss, rcond=cfo.RANK_CUT, hermitian=True) @ (t * s))
  got = _host_solve(shim, sums)
  w_oracle, _, _ = cfo.solve_pinv(S, t)
  scale = np.abs(want).max()
  print(f"{name}: max |solve - pinv| / max|w| {np.abs(got - want).max() / scale:.2e}")
  assert np.isfinite(got).all()
  assert np.abs(got - want).max() <= 1e-9 * scale, (got, want)
  assert np.abs(w_oracle - want).max() <= 1e-9 * scale
  if name == "full":                                   # full rank: the least-squares solution itself
    assert np.abs(S @ got - t).max() <= 1e-9 * np.abs(t).max()


def test_host_solve_without_pixels_gives_zero(shim):
  assert np.array_equal(_host_solve(shim, np.zeros(45)), np.zeros(10))


def test_host_fit_matches_the_reference(shim, fixtures):
  tol = cfo.golden_tolerance(fixtures)
  worst = 0.0
  for f in fixtures:
    got = _host_fit(shim, f["img"], f["ref"])
    err = float(np.abs(got.astype(np.float64) - f["out64"]).max())
    worst = max(worst, err)
    print(f"{f['img'].shape}: max |hm_color_fit - golden fp64| {err:.2e} (tol {tol:.2e})")
    assert err <= tol, (err, tol)
    assert got.min() >= 0.0 and got.max() <= 1.0
  PARITY_LOG.append(("colour fit, host shim vs reference fp64 (absolute)", "image", worst, 0, 3, tol, 0))


def test_host_fit_zero_iterations_copies(shim, fixtures):
  f = fixtures[0]
  assert np.array_equal(_host_fit(shim, f["img"], f["ref"], num_iters=0), f["img"])


# ---- the Python layer's argument checks (no GPU needed: they come before any native call) ------------------------------
def test_fit_colors_rejects_bad_shapes_and_devices():
  import splat_trainer_amd as sta
  a = torch.rand(8, 9, 3)
  for img, ref in ((a, torch.rand(8, 9, 4)), (torch.rand(8, 9, 4), torch.rand(8, 9, 4)), (a, torch.rand(9, 8, 3)),
                   (a, a.clone())):                                                    # the last: on the CPU
    with pytest.raises(ValueError):
      sta.fit_colors_batch(img, ref)
  with pytest.raises(ValueError):
    sta.fit_colors(a, a.clone())


@dataclasses.dataclass
class _Rendering:
  image: torch.Tensor


def test_evaluation_rejects_bad_shapes_and_devices():
  import splat_trainer_amd as sta
  for img, src in ((torch.rand(16, 16, 3), torch.rand(16, 17, 3)), (torch.rand(16, 16, 4), torch.rand(16, 16, 4)),
                   (torch.rand(3, 16, 16), torch.rand(3, 16, 16)), (torch.rand(16, 16, 3), torch.rand(16, 16, 3))):
    ev = sta.Evaluation("a/b.png", _Rendering(img), src)
    assert ev.image_id == "a_b.png" and ev.image is img
    for name in ("psnr", "l1", "ssim", "metrics"):
      with pytest.raises(ValueError):
        getattr(ev, name)
  with pytest.raises(dataclasses.FrozenInstanceError):
    ev.filename = "c"


def test_compute_psnr_agrees_with_its_definition():
  import splat_trainer_amd as sta
  gen = torch.Generator().manual_seed(0)
  a, b = torch.rand(5, 7, 3, generator=gen, dtype=torch.float64), torch.rand(5, 7, 3, generator=gen, dtype=torch.float64)
  mse = ((a - b) ** 2).mean().item()
  assert abs(sta.compute_psnr(a, b).item() - 10 * math.log10(1 / mse)) < 1e-12
  assert abs(sta.mse_to_psnr(torch.tensor(0.01, dtype=torch.float64)).item() - 20.0) < 1e-12
  from splat_trainer_amd.evaluation import _metrics_dict
  assert _metrics_dict([0.01, 0.5, 0.25]) == dict(psnr=10 * math.log10(1 / 0.01), l1=0.5, ssim=0.25)
