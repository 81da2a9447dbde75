"""Bilateral-grid colour correction on the GPU (csrc/bilagrid.hip, splat_trainer_amd.bilateral) against the fp64 torch
oracle (F.grid_sample + autograd, tests/bilagrid_recovery.py): parity of the image and both gradients, the TV value and
gradient, the identity rule, bit-reproducibility, slice isolation, edge cases, the drop-in flow after a render, and
recovery of known per-image colour transforms."""
import pytest
import torch

import bilagrid_recovery as br
import splat_trainer_amd as sta
from helpers import oracle, rel_err
from splat_trainer_amd import synthetic
from splat_trainer_amd.bilateral import BilateralCorrector, BilateralCorrectorConfig, BilateralGrid
from splat_trainer_amd.harness import MiniTrainer

pytestmark = pytest.mark.gpu


def _image(H, W, seed, lo=-0.2, hi=1.2):
  gen = torch.Generator().manual_seed(seed)
  return lo + (hi - lo) * torch.rand(H, W, 3, generator=gen)


def _oracle(grids, k, rgb, go):
  G = grids.detach().cpu().double().clone().requires_grad_(True)
  x = rgb.detach().cpu().double().clone().requires_grad_(True)
  out = br.oracle_slice(G[k], x)
  (out * go.cpu().double()).sum().backward()
  return out.detach(), x.grad, G.grad


def _hip(grids, k, rgb, go):
  G = grids.detach().cuda().clone().requires_grad_(True)
  x = rgb.detach().cuda().clone().requires_grad_(True)
  out = sta.bilateral_correct(G, k, x)
  (out * go.cuda()).sum().backward()
  torch.cuda.synchronize()
  return out.detach(), x.grad, G.grad


@pytest.mark.parametrize("H,W", [(48, 64), (217, 333), (1080, 1920)])
@pytest.mark.parametrize("shape", [(16, 16, 8), (8, 12, 4), (2, 2, 2), (32, 32, 16)])
def test_slice_matches_oracle(H, W, shape):
  grids = br.random_grids(3, shape, scale=0.2, seed=H + shape[0])
  rgb = _image(H, W, seed=W)
  go = torch.randn(H, W, 3, generator=torch.Generator().manual_seed(1))
  o_out, o_rgb, o_grid = _oracle(grids, 1, rgb, go)
  out, d_rgb, d_grid = _hip(grids, 1, rgb, go)
  # dA/dz jumps where z crosses a grid level: a pixel whose fp32 luma lands on the other side of a level from the fp64
  # one gets the neighbouring cell's guidance term.  Such pixels (z within 1e-5 of a level) are left out of d_rgb, and
  # they must be the only ones above the tolerance.
  z = (rgb.double() @ torch.tensor(br.LUMA, dtype=torch.float64)) * (shape[2] - 1)
  kink = ((z - z.round()).abs() < 1e-5) & (z > 0) & (z < shape[2] - 1)
  keep = (~kink).unsqueeze(-1).cuda()
  errs = (rel_err(out, o_out), rel_err(d_rgb * keep, o_rgb.cuda() * keep), rel_err(d_grid, o_grid))
  print(f"bilagrid {shape} {W}x{H}: out {errs[0]:.2e} d_rgb {errs[1]:.2e} d_grid {errs[2]:.2e}"
        f" ({int(kink.sum())} pixels on a level left out of d_rgb)")
  assert errs[0] < 1e-5 and errs[1] < 1e-4 and errs[2] < 1e-4, errs
  assert int(kink.sum()) <= 1e-4 * H * W + 4


@pytest.mark.parametrize("N", [1, 7, 300])
def test_tv_matches_oracle(N):
  grids = br.random_grids(N, (16, 16, 8), scale=0.3, seed=N)
  G = grids.double().clone().requires_grad_(True)
  o_tv = br.oracle_tv(G)
  o_tv.backward()
  Gd = grids.cuda().requires_grad_(True)
  tv = sta.bilateral_tv_loss(Gd)
  assert tv.dim() == 0 and tv.is_cuda
  tv.backward()
  assert abs(float(tv.detach()) - float(o_tv.detach())) <= 1e-5 * abs(float(o_tv.detach()))
  assert rel_err(Gd.grad, G.grad) < 1e-4


def test_identity_grid_returns_the_image_bit_for_bit():
  grids = br.identity(4, (16, 16, 8)).cuda()
  rgb = _image(217, 333, seed=3, lo=-0.5, hi=1.5).cuda()
  out = sta.bilateral_correct(grids, 2, rgb)
  assert torch.equal(out.view(torch.int32), rgb.view(torch.int32))


def test_two_runs_give_identical_bits():
  grids = br.random_grids(2, (16, 16, 8), seed=4)
  rgb = _image(1080, 1920, seed=4)
  go = torch.randn(1080, 1920, 3, generator=torch.Generator().manual_seed(4))
  a, b = _hip(grids, 0, rgb, go), _hip(grids, 0, rgb, go)
  for x, y in zip(a, b):
    assert torch.equal(x.view(torch.int32), y.view(torch.int32))
  big = br.random_grids(300, (16, 16, 8), seed=5).cuda().requires_grad_(True)
  t1 = sta.bilateral_tv_loss(big); t1.backward(); g1 = big.grad.clone(); big.grad = None
  t2 = sta.bilateral_tv_loss(big); t2.backward()
  assert torch.equal(t1.view(1).view(torch.int32), t2.view(1).view(torch.int32))
  assert torch.equal(g1.view(torch.int32), big.grad.view(torch.int32))


def test_only_the_sampled_slice_gets_a_gradient_and_batches_accumulate():
  grids = br.random_grids(5, (8, 12, 4), seed=6)
  imgs = [_image(61, 83, seed=s) for s in range(3)]
  gos = [torch.randn(61, 83, 3, generator=torch.Generator().manual_seed(10 + s)) for s in range(3)]
  order = [3, 1, 3]                                      # image 3 twice
  G = grids.cuda().requires_grad_(True)
  loss = sum((sta.bilateral_correct(G, k, x.cuda()) * go.cuda()).sum() for k, x, go in zip(order, imgs, gos))
  loss.backward()
  Go = grids.double().requires_grad_(True)
  sum((br.oracle_slice(Go[k], x.double()) * go.double()).sum() for k, x, go in zip(order, imgs, gos)).backward()
  assert rel_err(G.grad, Go.grad) < 1e-4
  untouched = [0, 2, 4]
  assert G.grad[untouched].abs().max().item() == 0
  # one image alone: only its slice
  G2 = grids.cuda().requires_grad_(True)
  (sta.bilateral_correct(G2, 4, imgs[0].cuda()) * gos[0].cuda()).sum().backward()
  assert G2.grad[:4].abs().max().item() == 0 and G2.grad[4].abs().max().item() > 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_strided_and_low_precision_images(dtype):
  grids = br.random_grids(2, (16, 16, 8), seed=7)
  base = _image(90, 70, seed=7).to(dtype)
  chw = base.permute(2, 0, 1).contiguous()               # (3, H, W) storage, (H, W, 3) view: non-contiguous
  x = chw.cuda().permute(1, 2, 0).requires_grad_(True)
  assert not x.is_contiguous()
  go = torch.randn(90, 70, 3, generator=torch.Generator().manual_seed(8))
  out = sta.bilateral_correct(grids.cuda(), 1, x)
  assert out.dtype is torch.float32
  (out * go.cuda()).sum().backward()
  assert x.grad.dtype is dtype and x.grad.shape == x.shape
  o_out, o_rgb, _ = _oracle(grids, 1, base.float(), go)
  assert rel_err(out, o_out) < 1e-5
  assert rel_err(x.grad.float(), o_rgb) < (1e-4 if dtype is torch.float32 else 1e-2)


def test_gradient_to_one_input_only():
  grids = br.random_grids(2, (16, 16, 8), seed=9)
  rgb = _image(50, 40, seed=9)
  go = torch.randn(50, 40, 3, generator=torch.Generator().manual_seed(9))
  _, o_rgb, o_grid = _oracle(grids, 0, rgb, go)
  G = grids.cuda().requires_grad_(True)
  (sta.bilateral_correct(G, 0, rgb.cuda()) * go.cuda()).sum().backward()
  assert rel_err(G.grad, o_grid) < 1e-4
  x = rgb.cuda().requires_grad_(True)
  (sta.bilateral_correct(grids.cuda(), 0, x) * go.cuda()).sum().backward()
  assert rel_err(x.grad, o_rgb) < 1e-4


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (13, 1), (3, 5), (17, 31)])
def test_tiny_and_odd_images(H, W):
  grids = br.random_grids(1, (16, 16, 8), seed=H * W)
  rgb = _image(H, W, seed=H + W, lo=-1.0, hi=2.0)          # values well outside [0, 1]
  go = torch.randn(H, W, 3, generator=torch.Generator().manual_seed(2))
  o = _oracle(grids, 0, rgb, go)
  h = _hip(grids, 0, rgb, go)
  assert rel_err(h[0], o[0]) < 1e-5 and rel_err(h[1], o[1]) < 1e-4 and rel_err(h[2], o[2]) < 1e-4


def test_value_errors():
  grids = br.identity(2, (16, 16, 8)).cuda()
  img = torch.rand(8, 8, 3, device="cuda")
  with pytest.raises(ValueError):
    sta.bilateral_correct(grids, 0, torch.rand(8, 8, 4, device="cuda"))        # C != 3
  for k in (-1, 2):
    with pytest.raises(ValueError):
      sta.bilateral_correct(grids, k, img)
  for shape in ((16, 16, 1), (65, 16, 8), (16, 1, 8)):
    with pytest.raises(ValueError):
      sta.bilateral_correct(br.identity(1, shape).cuda(), 0, img)
  with pytest.raises(ValueError):
    sta.bilateral_correct(grids.cpu(), 0, img.cpu())
  with pytest.raises(ValueError):
    sta.bilateral_correct(grids, 0, img.cpu())
  with pytest.raises(ValueError):
    sta.bilateral_tv_loss(grids.cpu())
  with pytest.raises(ValueError):
    BilateralGrid(1, grid_X=65)


def test_drop_in_flow_after_render():
  """render_gaussians(use_sh=True) -> BilateralCorrector.correct -> reference_loss -> backward: the splat gradients equal
  those of the same render back-propagated with the oracle's dL/dimage of the corrected loss."""
  g, cam = synthetic.scene_a(3000, 160, 120, sh_degree=1, seed=2, sigma_px=2.5)
  cfg = sta.RasterConfig()
  corr = BilateralCorrectorConfig().make_corrector(3, "cuda")
  with torch.no_grad():
    corr.bil_grids.grids.copy_(br.random_grids(3, (16, 16, 8), scale=0.1, seed=12).cuda())
  target = _image(120, 160, seed=13, lo=0.0, hi=1.0).cuda()

  def leaves():
    return sta.Gaussians3D(*(t.clone().cuda().requires_grad_(True) for t in
                             (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))

  gd = leaves()
  r = sta.render_gaussians(gd, cam.to("cuda"), cfg, use_sh=True)
  sta.reference_loss(corr.correct(r, 1), target).backward()

  # chain rule through the oracle: dL/dimage from fp64 autograd of reference_loss(oracle_slice(render))
  gd2 = leaves()
  r2 = sta.render_gaussians(gd2, cam.to("cuda"), cfg, use_sh=True)
  img = r2.image.detach().clone().requires_grad_(True)
  corrected = br.oracle_slice(corr.bil_grids.grids.detach()[1].double(), img.double())
  sta.reference_loss(corrected.float(), target).backward()
  r2.image.backward(img.grad)
  for a, b in ((gd.position, gd2.position), (gd.feature, gd2.feature), (gd.alpha_logit, gd2.alpha_logit),
               (gd.log_scaling, gd2.log_scaling), (gd.rotation, gd2.rotation)):
    assert rel_err(a.grad, b.grad) < 1e-4


def _recovery_data():
  g, cams = br.scene()
  cfg = sta.RasterConfig()
  gd = sta.Gaussians3D(*(t.cuda() for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
  with torch.no_grad():
    renders = [sta.render_gaussians(gd, c.to("cuda"), cfg, use_sh=True).image.clone() for c in cams[:br.NUM_IMAGES]]
  Gt = br.true_grids()
  targets = [br.oracle_slice(Gt[k].cuda(), r.double()).float() for k, r in enumerate(renders)]
  return g, cams[:br.NUM_IMAGES], renders, targets


def test_corrector_recovers_known_colour_transforms():
  _, _, renders, targets = _recovery_data()
  corr = BilateralCorrectorConfig(bilateral_grid_shape=br.SHAPE, tv_weight=br.TV_WEIGHT, lr=br.LR).make_corrector(
      br.NUM_IMAGES, "cuda")
  before, after = br.fit(lambda k, r: corr.correct(r, k), corr.step, renders, targets)
  print(f"bilagrid recovery: image mse {before:.3e} -> {after:.3e} ({before / after:.1f}x)")
  assert after < before / br.MIN_RATIO


def test_corrector_state_dict_round_trip():
  cfg = BilateralCorrectorConfig(bilateral_grid_shape=(8, 8, 4))
  corr = cfg.make_corrector(3, "cuda")
  x = _image(40, 30, seed=1).cuda()
  (corr.correct(x, 2) ** 2).mean().backward()
  tv = corr.step(0.5)
  assert tv.is_cuda and tv.dim() == 0
  sd = corr.state_dict()
  assert sd["num_images"] == 3 and set(sd["bil_grids"]) == {"grids", "rgb2gray_weight"}
  assert sd["bil_grids"]["grids"].shape == (3, 12, 4, 8, 8) and sd["bil_grids"]["rgb2gray_weight"].shape == (1, 3)
  back = cfg.from_state_dict(sd, "cuda")
  assert torch.equal(back.bil_grids.grids, corr.bil_grids.grids)


def test_mini_trainer_with_corrector_ends_lower():
  g, cams, _, targets = _recovery_data()
  cams = [c.to("cuda") for c in cams]
  cfg = sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True)
  finals = {}
  for name in ("plain", "corrected"):
    corr = None
    if name == "corrected":
      corr = BilateralCorrectorConfig(bilateral_grid_shape=br.SHAPE, tv_weight=br.TV_WEIGHT, lr=br.LR).make_corrector(
          len(cams), "cuda")
    tr = MiniTrainer(g.to("cuda"), cams, targets, cfg, lr=1e-3, densify_every=0, total_steps=60, seed=0, corrector=corr)
    log = tr.train(60)
    finals[name] = sum(log.losses[-5:]) / 5
  print("mini trainer final loss", finals)
  assert finals["corrected"] < finals["plain"]
