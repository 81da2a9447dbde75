"""The evaluation pass on the GPU (splat_trainer_amd.evaluation, csrc/eval.hip): the native colour fit against the
reference's recorded results and the fp64 oracle, its defined behaviour on rank-deficient images, the one-call image
metrics against fp64 means and the SSIM oracle, ``Evaluation`` and ``evaluate_scene``."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import color_fit_oracle as cfo
import splat_trainer_amd as sta
from helpers import PARITY_LOG
from oracle import ssim_oracle
from splat_trainer_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

EPS = 0.5 / 255
METRIC_TOL = 2e-6           # tests/test_ssim.py: the valid-padding mean against the oracle


@pytest.fixture(scope="module")
def fixtures(golden_dir):
  return cfo.load_golden(os.path.join(golden_dir, "color_fit_ref.npz"))


@pytest.fixture(scope="module")
def tol(fixtures):
  return cfo.golden_tolerance(fixtures)


def _cuda(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_fit_colors_matches_the_reference_on_the_fixtures(fixtures, tol):
  worst = 0.0
  for f in fixtures:
    img, ref = _cuda(f["img"]), _cuda(f["ref"])
    got = sta.fit_colors(img, ref)
    assert got.shape == img.shape and got.dtype is torch.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - f["out64"]).max())
    worst = max(worst, err)
    print(f"{tuple(img.shape)}: max |fit_colors - golden fp64| {err:.2e} (tol {tol:.2e})")
    assert err <= tol, (err, tol)
    assert torch.equal(got, sta.fit_colors(img, ref))                              # no atomics: the same bits
    assert torch.equal(got, sta.fit_colors_batch(img.reshape(-1, 3), ref.reshape(-1, 3)).reshape(img.shape))
    assert torch.equal(sta.fit_colors_batch(img, ref, num_iters=0), img)
  PARITY_LOG.append(("colour fit, HIP vs reference fp64 (absolute)", "image", worst, 0, 3, tol, 0))


def _large_pair(seed):
  """520 x 512 = 266 240 pixels: more than the 1024 x 256 of the first stride, so the strided loop runs twice for some
  threads and every block slot is used.  With 4 M iterate entries no seed keeps a continuous image 1e-5 away from the
  thresholds, so the image is built to stay away: unclipped entries lie in [0.15, 0.85] and the distortion maps them into
  [0.1, 0.9], 12 % of the entries are exactly 0 or 1 and the distortion (gain 1.1, offset -0.05) sends those well outside
  [0, 1], where the clip returns them to exactly 0 or 1."""
  H, W = 520, 512
  rng = np.random.default_rng(seed)
  yy, xx = np.mgrid[0:H, 0:W]
  field = np.stack([0.5 + 0.5 * np.sin(xx / 37.0 + k) * np.cos(yy / 29.0 + 2 * k) for k in range(3)], axis=2)
  inner = 0.15 + 0.7 * np.clip(field + 0.03 * rng.standard_normal((H, W, 3)), 0, 1)
  pick = rng.random((H, W, 3))
  img = np.where(pick < 0.06, 0.0, np.where(pick > 0.94, 1.0, inner)).astype(np.float32)
  x = img.astype(np.float64)
  matrix = np.eye(3) + 0.02 * rng.standard_normal((3, 3))
  target = (1.1 * x - 0.05 + 0.05 * (x - 0.5) ** 2) @ matrix + 0.01 * rng.standard_normal((H, W, 3))
  ref = np.round(np.clip(target, 0, 1) * 255).astype(np.float32) / np.float32(255.0)
  return img, ref


def test_fit_colors_beyond_the_first_stride(tol):
  img, ref = _large_pair(seed=1)
  assert img.shape[0] * img.shape[1] == 266240 > 1024 * 256
  want, info = cfo.fit(img, ref)
  print(f"oracle: threshold distance {info['threshold_distance']:.2e}, eigenvalue ratio {info['eig_ratio']:.2e}")
  assert info["threshold_distance"] >= 1e-5, info["threshold_distance"]            # no mask decision can flip
  got = sta.fit_colors(_cuda(img), _cuda(ref))
  err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
  print(f"520 x 512: max |fit_colors - oracle fp64| {err:.2e} (tol {tol:.2e})")
  PARITY_LOG.append(("colour fit 520x512, HIP vs fp64 oracle (absolute)", "image", err, 0, 1, tol, 0))
  assert err <= tol, (err, tol)
  assert torch.equal(got, sta.fit_colors(_cuda(img), _cuda(ref)))


@pytest.mark.parametrize("kind", ["grey", "saturated_channel", "zero_channel"])
def test_fit_colors_is_defined_on_rank_deficient_images(fixtures, kind):
  """Finite, inside [0, 1] and no further from the target than the clipped input.  A channel without a single unclipped
  pixel has no equation at all and maps to 0 (the rule for lambda_max <= 0; the reference's lstsq on an all-zero system
  gives the same), so on such an image the overall MSE improves only as far as the other two channels gain more than
  that channel loses: it does on this fixture (target mean 0.46); against a brighter target it need not (on the
  24 x 40 fixture, target mean 0.73, the host shim gives 0.064 -> 0.197).  The other two channels improve on their own."""
  f = fixtures[2]
  img, ref = f["img"].copy(), f["ref"].astype(np.float64)
  dead = {"grey": None, "saturated_channel": 1, "zero_channel": 2}[kind]
  if kind == "grey":
    img = np.repeat(img[..., :1], 3, axis=2)
  elif kind == "saturated_channel":
    img[..., 1] = 1.0                                     # overexposed: columns g^2, g and 1 coincide, rg = r, gb = b
  else:
    img[..., 2] = 0.0
  got = sta.fit_colors(_cuda(img), _cuda(f["ref"])).cpu().numpy().astype(np.float64)
  assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
  clipped = np.clip(img.astype(np.float64), 0, 1)
  before, after = np.mean((clipped - ref) ** 2), np.mean((got - ref) ** 2)
  print(f"{kind}: mse to the target {before:.3e} -> {after:.3e}")
  assert after <= before, (before, after)
  if dead is not None:
    keep = [c for c in range(3) if c != dead]
    assert np.all(got[..., dead] == 0.0)
    assert np.mean((got[..., keep] - ref[..., keep]) ** 2) <= np.mean((clipped[..., keep] - ref[..., keep]) ** 2)


@pytest.mark.parametrize("index", [0, 1, 2])
def test_image_metrics_match_fp64(fixtures, index):
  f = fixtures[index]
  img, ref = _cuda(f["out32"]), _cuda(f["ref"])
  table = torch.full((4, 3), -7.0, device="cuda")
  row = sta.image_metrics(img, ref, out=table[2])
  assert row.data_ptr() == table[2].data_ptr()
  got = table.cpu().double()
  assert torch.all(got[[0, 1, 3]] == -7.0)                                         # the other rows are untouched
  a, b = torch.from_numpy(f["out32"]).double(), torch.from_numpy(f["ref"]).double()
  want = [((a - b) ** 2).mean().item(), (a - b).abs().mean().item(),
          ssim_oracle.fused_ssim(a.unsqueeze(0).permute(0, 3, 1, 2), b.unsqueeze(0).permute(0, 3, 1, 2), "valid").item()]
  for name, g, w in zip(("mse", "l1", "ssim"), got[2].tolist(), want):
    print(f"{tuple(img.shape)} {name}: {g:.9f} vs {w:.9f} ({abs(g - w):.2e})")
    assert abs(g - w) < METRIC_TOL, (name, g, w)
  assert torch.equal(sta.image_metrics(img, ref), table[2])


def test_evaluation_reads_its_metrics_with_one_native_call(fixtures):
  lib = _lib.load()
  native, calls = lib.gsr_image_metrics, []

  def counted(*args):
    calls.append(args)
    return native(*args)

  lib.gsr_image_metrics = counted
  try:
    for f in fixtures:
      calls.clear()
      src = _cuda(f["ref"])
      ev = sta.Evaluation("val/cam0/image.png", sta.Rendering(image=_cuda(f["img"]), camera=None, points=None), src)
      assert ev.image_id == "val_cam0_image.png"
      values = (ev.psnr, ev.l1, ev.ssim, ev.metrics)
      assert len(calls) == 1
      assert values[3] == dict(psnr=values[0], l1=values[1], ssim=values[2])
      mse = float(np.mean((f["img"].astype(np.float64) - f["ref"]) ** 2))
      assert abs(ev.psnr - 10 * np.log10(1 / mse)) < 1e-4
      cc = ev.color_corrected()
      assert isinstance(cc, sta.Evaluation) and cc.filename == ev.filename and cc.source_image is src
      assert isinstance(cc.rendering, sta.Rendering) and cc.image is not ev.image
      print(f"{tuple(src.shape)}: psnr {ev.psnr:.3f} -> colour corrected {cc.psnr:.3f}")
      assert cc.psnr > ev.psnr
      assert len(calls) == 2
  finally:
    lib.gsr_image_metrics = native


def test_evaluation_raises_what_fused_ssim_raises_on_a_small_image():
  img = torch.rand(10, 40, 3, device="cuda")
  with pytest.raises(ValueError) as native:
    sta.Evaluation("a", sta.Rendering(image=img, camera=None, points=None), img.clone()).metrics
  with pytest.raises(ValueError) as fused:
    sta.fused_ssim(img.unsqueeze(0).permute(0, 3, 1, 2), img.unsqueeze(0).permute(0, 3, 1, 2), padding="valid")
  assert str(native.value) == str(fused.value)


def test_evaluate_scene_equals_per_image_evaluations():
  g, cams = synthetic.scene_b(2000, 64, 48, sh_degree=0, seed=3, num_cameras=3)
  cams = [c.to("cuda") for c in cams]
  torch.manual_seed(11)
  config = sta.MLPSceneConfig(
      parameters=dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                      rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector")),
      reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
      color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=5, lr_diffuse=1e-2, lr_specular=1e-2),
      lr_glo_feature=0.1, image_features=32, point_features=16)
  scene = config.from_color_gaussians(g, 3, "cuda", seed=11)
  gen = torch.Generator().manual_seed(2)
  with torch.no_grad():
    sources = [(scene.render(c, i).image * 0.8 + 0.1 + 0.02 * torch.randn(48, 64, 3, generator=gen).cuda()).clamp(0, 1)
               for i, c in enumerate(cams)]
  views = [(f"cam/{i}.png", cams[i], i, sources[i]) for i in range(3)]
  options = dict(compute_visibility=True)
  metrics, metrics_cc = sta.evaluate_scene(scene, iter(views), color_correct=True, **options)
  assert sta.evaluate_scene(scene, views, **options) == metrics
  want, want_cc = {}, {}
  for name, cam, idx, src in views:
    with torch.no_grad():
      r = scene.render(cam, idx, render_median_depth=True, **options)
    assert r.median_depth_image is not None
    ev = sta.Evaluation(name, r.detach(), src)
    want[name], want_cc[name] = ev.metrics, ev.color_corrected().metrics
  assert metrics == want and metrics_cc == want_cc
  assert list(metrics) == [v[0] for v in views] and all(set(m) == {"psnr", "l1", "ssim"} for m in metrics.values())
  assert all(metrics_cc[k]["psnr"] > metrics[k]["psnr"] for k in metrics)
  assert sta.evaluate_scene(scene, []) == {}
