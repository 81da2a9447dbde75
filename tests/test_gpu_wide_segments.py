"""Segmented wide frames (render_projected with 4..16 channels under a segment plan: wide_ckpt_fwd, passes A / C / D wide
and the segment blocks of composite_bwd_wide) on the GPU: against the fp64 oracle under forced segments, bit for bit
against the unsegmented walk where only the backward pass is split, bit for bit against the C <= 3 path under the same
plan, channel bookkeeping, and the edge cases of the boundary."""
import functools
import math

import pytest
import torch

import splat_trainer_amd as sta
from helpers import observe, oracle, rel_err, small_scene
from splat_trainer_amd import synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-4
ORACLE_KEYS = ("image", "final_T", "visibility", "prune_cost", "split_score", "d_g2d", "d_feat")


def _cfg(seg, seg_min=None):
  return sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True, segment_pairs=seg,
                          segment_min_pairs=seg if seg_min is None else seg_min)


def _projected(g, cam):
  gd = sta.Gaussians3D(*(t.cuda() for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
  with torch.no_grad():
    g2d, depth, idx = sta.project_to_image(gd, cam.to("cuda"), _cfg(0))
  return g2d, depth, idx


def _render(idx, g2d, depth, feats, cam, cfg, wimg, median=False):
  """One render_projected + backward of sum(image * wimg); returns every output and gradient."""
  g2 = g2d.detach().clone().requires_grad_(True)
  f = feats.detach().clone().requires_grad_(True)
  r = sta.render_projected(idx, g2, f, depth, cam.to("cuda"), cfg, render_median_depth=median)
  (r.image * wimg).sum().backward()
  torch.cuda.synchronize()
  out = dict(image=r.image.detach(), final_T=r.final_transmittance.detach(), visibility=r.points.visibility.detach(),
             prune_cost=r.points.prune_cost.detach(), split_score=r.points.split_score.detach(),
             d_g2d=g2.grad, d_feat=f.grad)
  if median:
    out["median"] = r.median_depth_image.detach()
  return out


def _oracle(g2d, depth, feats, cam, wimg, median=False):
  """The fp64 oracle's outputs and gradients under the same loss (it walks whole lists: segmentation does not exist there)."""
  og = g2d.detach().cpu().double().requires_grad_(True)
  of = feats.detach().cpu().double().requires_grad_(True)
  w = wimg.cpu().double()
  out = oracle.rasterize(og, depth.detach().cpu().double(), of, cam.image_size, _cfg(0), dL_dimage=w, want_median=median)
  (out.image * w).sum().backward()
  ref = dict(image=out.image.detach(), final_T=out.final_T, visibility=out.visibility, prune_cost=out.prune_cost,
             split_score=out.split_score, d_g2d=og.grad, d_feat=of.grad)
  if median:
    ref["median"] = out.median_depth
  return ref


def _inputs(g, cam, C, seed):
  g2d, depth, idx = _projected(g, cam)
  W, H = cam.image_size
  torch.manual_seed(seed)
  return idx, g2d, depth, torch.rand(idx.shape[0], C, device="cuda"), torch.rand(H, W, C, device="cuda")


def _against_oracle(label, hip, ref, median=False):
  for k in ORACLE_KEYS:
    worst, _ = observe(label, k, hip[k], ref[k], TOL)
    print(f"{label}: {k} {worst:.3e}")
    assert worst < TOL, (label, k, worst)
  if median:
    e = rel_err(hip["median"], ref["median"])
    print(f"{label}: median {e:.3e}")
    assert e < 1e-5, (label, e)


@functools.lru_cache(maxsize=None)
def _forced_case(C):
  """Scene, inputs and the oracle's answer, computed once for all segment lengths."""
  n, w, h, seed = (500, 64, 48, 11) if C == 4 else (900, 50, 37, 13)
  g, cam = small_scene(n, w, h, sh_degree=0, seed=seed, sigma_px=3.0)
  inp = _inputs(g, cam, C, seed=C)
  median = C == 16
  return cam, inp, median, _oracle(inp[1], inp[2], inp[3], cam, inp[4], median)


@pytest.mark.parametrize("seg", [1, 8, 64])
@pytest.mark.parametrize("C", [4, 16])
def test_forced_segments_match_oracle(C, seg):
  """Tiny segments with segment_min_pairs = segment_pairs force every tile longer than `seg` through passes A / C / D
  wide and the segment blocks of the backward launch."""
  cam, (idx, g2d, depth, feats, wimg), median, ref = _forced_case(C)
  hip = _render(idx, g2d, depth, feats, cam, _cfg(seg), wimg, median)
  _against_oracle(f"wide segments C={C} seg={seg}", hip, ref, median)


@pytest.mark.parametrize("seg", [4, 32])
def test_checkpointed_backward(seg):
  """Tiles longer than `seg` but never heavy: the forward pass is the one-wave walk (same bits as without segments) that
  leaves (T, C colours) at every segment end; the backward pass runs one wave per segment from those checkpoints."""
  g, cam = small_scene(900, 50, 37, sh_degree=0, seed=13, sigma_px=3.0)
  idx, g2d, depth, feats, wimg = _inputs(g, cam, 8, seed=8)
  cfg = _cfg(seg, seg_min=10 ** 9)
  cut = _render(idx, g2d, depth, feats, cam, cfg, wimg, median=True)
  whole = _render(idx, g2d, depth, feats, cam, _cfg(0), wimg, median=True)
  again = _render(idx, g2d, depth, feats, cam, cfg, wimg, median=True)
  for k in ("image", "final_T", "visibility", "median"):
    assert torch.equal(cut[k], whole[k]), k
  for k in ("d_g2d", "d_feat", "prune_cost", "split_score"):
    worst, _ = observe(f"wide checkpointed backward seg={seg} vs one wave per tile", k, cut[k], whole[k], 1e-5)
    print(f"seg={seg}: {k} {worst:.3e}")
    assert worst < 2e-5, (k, worst)
    assert cut[k].abs().max() > 0
  for k in cut:
    assert torch.equal(cut[k], again[k]), k


@pytest.mark.parametrize("seg,seg_min", [(8, 8), (16, 32)])
def test_heavy_segments_equal_the_narrow_path_bit_for_bit(seg, seg_min):
  """Under the same plan the wide render of 16 channels gives, on its first three, the bits of the C = 3 render: the
  same T_in product, the same walk, the same colour sum in segment order."""
  g, cam = small_scene(1500, 96, 80, sh_degree=0, seed=5, sigma_px=3.0)
  idx, g2d, depth, f16, w16 = _inputs(g, cam, 16, seed=1)
  f3, w3 = f16[:, :3].contiguous(), w16[..., :3].contiguous()
  cfg = _cfg(seg, seg_min)
  narrow = _render(idx, g2d, depth, f3, cam, cfg, w3, median=True)
  narrow_whole = _render(idx, g2d, depth, f3, cam, _cfg(0), w3, median=True)
  # the segmented narrow image must differ from the unsegmented one somewhere, or the comparison below proves nothing
  assert not torch.equal(narrow["image"], narrow_whole["image"])
  wide = _render(idx, g2d, depth, f16, cam, cfg, w16, median=True)
  assert torch.equal(wide["image"][..., :3], narrow["image"])
  for k in ("final_T", "visibility", "median"):
    assert torch.equal(wide[k], narrow[k]), k
  assert wide["image"][..., 3:].abs().max() > 0.1


def test_saturating_stack_of_opaque_splats():
  """Many opaque splats on one tile: pixels die inside early segments and later segments must be skipped."""
  g, cam = small_scene(600, 32, 32, sh_degree=0, seed=2, sigma_px=6.0)
  g.alpha_logit[:] = 4.0                                          # opacity 0.98
  idx, g2d, depth, feats, wimg = _inputs(g, cam, 8, seed=3)
  hip = _render(idx, g2d, depth, feats, cam, _cfg(8), wimg)
  _against_oracle("wide segments, saturating opaque stack", hip, _oracle(g2d, depth, feats, cam, wimg))
  assert float(hip["final_T"].max()) < 1e-3


def test_channel_split_under_heavy_segments():
  g, cam = small_scene(2000, 128, 96, sh_degree=0, seed=21, sigma_px=3.0)
  idx, g2d, depth, f8, w8 = _inputs(g, cam, 8, seed=2)
  cfg = _cfg(8, 8)
  full = _render(idx, g2d, depth, f8, cam, cfg, w8)
  a = _render(idx, g2d, depth, f8[:, :4].contiguous(), cam, cfg, w8[..., :4].contiguous())
  b = _render(idx, g2d, depth, f8[:, 4:].contiguous(), cam, cfg, w8[..., 4:].contiguous())
  assert torch.equal(torch.cat([a["image"], b["image"]], -1), full["image"])
  assert torch.equal(torch.cat([a["d_feat"], b["d_feat"]], -1), full["d_feat"])
  s = a["d_g2d"] + b["d_g2d"]
  assert ((s - full["d_g2d"]).abs().max() / full["d_g2d"].abs().max()).item() < 1e-6


def _clustered(n, w, h, frac, region, seed=0):
  """tests/test_gpu_segments.py's construction: `frac` of the splats packed into the central `region` of the image."""
  g, cam = synthetic.scene_a(n, w, h, sh_degree=0, seed=seed)
  k = int(frac * n)
  gen = torch.Generator().manual_seed(1)
  fx = w / (2.0 * math.tan(math.radians(30.0)))
  z = g.position[:k, 2]
  u = (0.5 + region * (torch.rand(k, generator=gen) - 0.5)) * w
  v = (0.5 + region * (torch.rand(k, generator=gen) - 0.5)) * h
  g.position[:k, 0] = (u - w / 2) * z / fx
  g.position[:k, 1] = (v - h / 2) * z / fx
  return g, cam


def test_clustered_scene_matches_oracle_with_default_thresholds():
  """Half of 20k splats in the central 10 % x 10 % of a 320x240 image: a few tiles carry lists of thousands of pairs and
  are segmented by the default thresholds."""
  g, cam = _clustered(20_000, 320, 240, 0.5, 0.1)
  idx, g2d, depth, feats, wimg = _inputs(g, cam, 4, seed=4)
  cfg = sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True)
  hip = _render(idx, g2d, depth, feats, cam, cfg, wimg)
  _against_oracle("wide clustered 20k 320x240 (default segments)", hip, _oracle(g2d, depth, feats, cam, wimg))


def test_edge_cases_under_forced_segments():
  g, cam = small_scene(300, 64, 48, sh_degree=0, seed=3)
  g2d, depth, idx = _projected(g, cam)
  c, cfg = cam.to("cuda"), _cfg(8)
  # no splats (M = 0)
  f0 = torch.zeros(0, 6, device="cuda", requires_grad=True)
  r = sta.render_projected(idx[:0], g2d[:0], f0, depth[:0], c, cfg)
  assert r.image.shape == (48, 64, 6) and r.image.abs().max() == 0
  r.image.sum().backward()
  # every splat off screen (O = 0): the backward pass runs and leaves zeros
  g_off = g2d.clone()
  g_off[:, 0] += 10_000.0
  fo = torch.rand(idx.shape[0], 6, device="cuda", requires_grad=True)
  r = sta.render_projected(idx, g_off, fo, depth, c, cfg)
  assert r.image.shape == (48, 64, 6) and r.image.abs().max() == 0 and r.num_overlaps == 0
  r.image.sum().backward()
  assert fo.grad.shape == (idx.shape[0], 6) and fo.grad.abs().max() == 0
