"""render_projected with 4..16 feature channels (the wide path: feature table + K6 / K7 wide) on the GPU: against the fp64
oracle on small scenes, bit for bit against the C <= 3 path at full size, channel bookkeeping, reproducibility and the
edge cases of the boundary."""
import math

import pytest
import torch

import splat_trainer_amd as sta
from helpers import observe, oracle, rel_err, small_scene
from splat_trainer_amd import synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-4
CFG = sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True)


def _projected(g, cam, cfg):
  gd = sta.Gaussians3D(*(t.cuda() for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
  with torch.no_grad():
    g2d, depth, idx = sta.project_to_image(gd, cam.to("cuda"), cfg)
  return g2d, depth, idx


def _render(idx, g2d, depth, feats, cam, cfg, wimg=None, median=False):
  """One render_projected + backward of sum(image * wimg); returns every output and gradient."""
  g2 = g2d.detach().clone().requires_grad_(True)
  f = feats.detach().clone().requires_grad_(True)
  r = sta.render_projected(idx, g2, f, depth, cam.to("cuda"), cfg, render_median_depth=median)
  if wimg is not None:
    (r.image * wimg).sum().backward()
  torch.cuda.synchronize()
  out = dict(image=r.image.detach(), final_T=r.final_transmittance.detach(), visibility=r.points.visibility.detach(),
             prune_cost=r.points.prune_cost.detach(), split_score=r.points.split_score.detach(),
             d_g2d=g2.grad, d_feat=f.grad)
  if median:
    out["median"] = r.median_depth_image.detach()
  return out


def _oracle(idx, g2d, depth, feats, cam, cfg, wimg, median=False):
  og = g2d.detach().cpu().double().requires_grad_(True)
  of = feats.detach().cpu().double().requires_grad_(True)
  W, H = cam.image_size
  out = oracle.rasterize(og, depth.detach().cpu().double(), of, (W, H), cfg, dL_dimage=wimg.cpu().double(),
                         want_median=median)
  (out.image * wimg.cpu().double()).sum().backward()
  return out, og.grad, of.grad


@pytest.mark.parametrize("C,vis", [(4, True), (5, False), (8, True), (12, True), (16, True), (16, False)])
def test_wide_matches_oracle(C, vis):
  g, cam = small_scene(1500, 128, 96, sh_degree=0, seed=11 + C, sigma_px=3.0)
  cfg = CFG if vis else sta.RasterConfig()
  g2d, depth, idx = _projected(g, cam, cfg)
  torch.manual_seed(C)
  feats = torch.rand(idx.shape[0], C, device="cuda")
  wimg = torch.rand(96, 128, C, device="cuda")
  hip = _render(idx, g2d, depth, feats, cam, cfg, wimg)
  out, d_g2d, d_feat = _oracle(idx, g2d, depth, feats, cam, cfg, wimg)
  assert hip["image"].shape == (96, 128, C)
  assert rel_err(hip["image"], out.image) < TOL
  assert rel_err(hip["d_g2d"], d_g2d) < TOL
  assert rel_err(hip["d_feat"], d_feat) < TOL
  assert rel_err(hip["prune_cost"], out.prune_cost) < TOL
  assert rel_err(hip["split_score"], out.split_score) < TOL
  if vis:
    assert rel_err(hip["visibility"], out.visibility) < TOL
  assert hip["image"].abs().max() > 0.1


def test_wide_median_depth_matches_c3():
  g, cam = small_scene(1200, 128, 96, sh_degree=0, seed=5, sigma_px=3.0)
  cfg = sta.RasterConfig(compute_visibility=True, segment_pairs=0)
  g2d, depth, idx = _projected(g, cam, cfg)
  torch.manual_seed(0)
  f16 = torch.rand(idx.shape[0], 16, device="cuda")
  wide = _render(idx, g2d, depth, f16, cam, cfg, median=True)
  narrow = _render(idx, g2d, depth, f16[:, :3].contiguous(), cam, cfg, median=True)
  assert torch.equal(wide["median"], narrow["median"]) and wide["median"].abs().max() > 0


def _full_size_bitwise(g, cam, label, segmented_c3_check=False):
  cfg0 = sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True, segment_pairs=0)
  g2d, depth, idx = _projected(g, cam, cfg0)
  W, H = cam.image_size
  torch.manual_seed(1)
  f16 = torch.rand(idx.shape[0], 16, device="cuda")
  f16[:, 3:] = 0.0
  w16 = torch.zeros(H, W, 16, device="cuda")
  w16[..., :3] = torch.rand(H, W, 3, device="cuda")
  wide = _render(idx, g2d, depth, f16, cam, cfg0, w16)
  narrow = _render(idx, g2d, depth, f16[:, :3].contiguous(), cam, cfg0, w16[..., :3].contiguous())
  assert torch.equal(wide["image"][..., :3], narrow["image"]), label
  assert wide["image"][..., 3:].abs().max() == 0
  assert torch.equal(wide["final_T"], narrow["final_T"]), label
  assert torch.equal(wide["visibility"], narrow["visibility"]), label
  # geometry gradients / heuristics: the two K7s form the colour term differently (3 vs 16 fused terms)
  for k in ("d_g2d", "prune_cost", "split_score"):
    e = rel_err(wide[k], narrow[k])
    observe(label + " wide vs C=3", k, wide[k], narrow[k], TOL)
    assert e < TOL, (label, k, e)
  assert rel_err(wide["d_feat"][:, :3], narrow["d_feat"]) < TOL
  assert wide["d_feat"][:, 3:].abs().max() == 0
  if segmented_c3_check:
    seg = _render(idx, g2d, depth, f16[:, :3].contiguous(), cam, CFG, w16[..., :3].contiguous())
    assert rel_err(wide["image"][..., :3], seg["image"]) < TOL
    assert rel_err(wide["d_g2d"], seg["d_g2d"]) < TOL
  return idx.shape[0]


def test_wide_bitwise_equals_c3_at_c2_size():
  g, cam = synthetic.scene_a(500_000, 1920, 1080, sh_degree=0, seed=0)
  assert _full_size_bitwise(g, cam, "c2 500k 1080p") > 100_000


def test_wide_bitwise_equals_c3_on_clustered_scene():
  g, cam = synthetic.scene_a(20_000, 320, 240, sh_degree=0, seed=0)
  k = 10_000
  gen = torch.Generator().manual_seed(1)
  fx = 320 / (2.0 * math.tan(math.radians(30.0)))
  z = g.position[:k, 2]
  g.position[:k, 0] = ((0.5 + 0.1 * (torch.rand(k, generator=gen) - 0.5)) * 320 - 160) * z / fx
  g.position[:k, 1] = ((0.5 + 0.1 * (torch.rand(k, generator=gen) - 0.5)) * 240 - 120) * z / fx
  r = sta.render_gaussians(sta.Gaussians3D(*(t.cuda() for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit,
                                                                   g.feature))), cam.to("cuda"), CFG, use_sh=True)
  assert r.num_overlaps > 20_000                 # ~10k splats on the central 10 % of the frame: tiles of thousands of pairs
  _full_size_bitwise(g, cam, "clustered 20k 320x240", segmented_c3_check=True)


def test_channel_permutation_and_split():
  g, cam = small_scene(2000, 128, 96, sh_degree=0, seed=21, sigma_px=3.0)
  g2d, depth, idx = _projected(g, cam, CFG)
  torch.manual_seed(2)
  f8 = torch.rand(idx.shape[0], 8, device="cuda")
  w8 = torch.rand(96, 128, 8, device="cuda")
  full = _render(idx, g2d, depth, f8, cam, CFG, w8)
  perm = torch.randperm(8, device="cuda")
  p = _render(idx, g2d, depth, f8[:, perm].contiguous(), cam, CFG, w8[..., perm].contiguous())
  assert torch.equal(p["image"], full["image"][..., perm])
  assert torch.equal(p["d_feat"], full["d_feat"][:, perm])
  a = _render(idx, g2d, depth, f8[:, :4].contiguous(), cam, CFG, w8[..., :4].contiguous())
  b = _render(idx, g2d, depth, f8[:, 4:].contiguous(), cam, CFG, w8[..., 4:].contiguous())
  assert torch.equal(torch.cat([a["image"], b["image"]], -1), full["image"])
  assert torch.equal(torch.cat([a["d_feat"], b["d_feat"]], -1), full["d_feat"])
  s = a["d_g2d"] + b["d_g2d"]
  assert ((s - full["d_g2d"]).abs().max() / full["d_g2d"].abs().max()).item() < 1e-6


def test_wide_is_reproducible():
  g, cam = synthetic.scene_a(100_000, 640, 480, sh_degree=0, seed=3)
  g2d, depth, idx = _projected(g, cam, CFG)
  torch.manual_seed(4)
  f = torch.rand(idx.shape[0], 16, device="cuda")
  w = torch.rand(480, 640, 16, device="cuda")
  a = _render(idx, g2d, depth, f, cam, CFG, w)
  b = _render(idx, g2d, depth, f, cam, CFG, w)
  for k in a:
    assert torch.equal(a[k], b[k]), k


def test_wide_edge_cases():
  g, cam = small_scene(300, 64, 48, sh_degree=0, seed=3)
  g2d, depth, idx = _projected(g, cam, CFG)
  c = cam.to("cuda")
  # no splats
  f0 = torch.zeros(0, 6, device="cuda", requires_grad=True)
  r = sta.render_projected(idx[:0], g2d[:0], f0, depth[:0], c, CFG)
  assert r.image.shape == (48, 64, 6) and r.image.abs().max() == 0
  # every splat off screen (O = 0)
  g_off = g2d.clone()
  g_off[:, 0] += 10_000.0
  fo = torch.rand(idx.shape[0], 6, device="cuda", requires_grad=True)
  r = sta.render_projected(idx, g_off, fo, depth, c, CFG)
  assert r.image.shape == (48, 64, 6) and r.image.abs().max() == 0 and r.num_overlaps == 0
  r.image.sum().backward()
  assert fo.grad.abs().max() == 0
  # fp16 features from autocast
  f8 = torch.rand(idx.shape[0], 8, device="cuda").half().requires_grad_(True)
  r = sta.render_projected(idx, g2d, f8, depth, c, CFG)
  r.image.sum().backward()
  assert r.image.dtype == torch.float32 and f8.grad.dtype == torch.float16 and f8.grad.abs().max() > 0
  ref = sta.render_projected(idx, g2d, f8.detach().float(), depth, c, CFG)
  assert torch.equal(r.image, ref.image)
  # eval mode
  with torch.no_grad():
    r = sta.render_projected(idx, g2d, torch.rand(idx.shape[0], 12, device="cuda"), depth, c, CFG)
  assert not r.image.requires_grad and r.image.shape == (48, 64, 12)
  # out of range
  with pytest.raises(ValueError, match="1..16"):
    sta.render_projected(idx, g2d, torch.rand(idx.shape[0], 17, device="cuda"), depth, c, CFG)


def test_rgb_plus_depth_channel():
  g, cam = small_scene(1500, 128, 96, sh_degree=0, seed=9, sigma_px=3.0)
  g2d, depth, idx = _projected(g, cam, CFG)
  torch.manual_seed(6)
  rgb = torch.rand(idx.shape[0], 3, device="cuda")
  d = depth.detach().clone().reshape(-1, 1).requires_grad_(True)
  target = torch.rand(96, 128, device="cuda")
  r = sta.render_projected(idx, g2d, torch.cat([rgb, d], 1), depth, cam.to("cuda"), CFG)
  (r.image[..., 3] - target).square().sum().backward()
  od = depth.detach().cpu().double().reshape(-1, 1).requires_grad_(True)
  out = oracle.rasterize(g2d.detach().cpu().double(), depth.detach().cpu().double(),
                         torch.cat([rgb.cpu().double(), od], 1), (128, 96), CFG)
  (out.image[..., 3] - target.cpu().double()).square().sum().backward()
  assert rel_err(r.image[..., 3], out.image[..., 3]) < TOL
  assert rel_err(d.grad, od.grad) < TOL
