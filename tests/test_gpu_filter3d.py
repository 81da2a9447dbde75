"""The 3-D smoothing filter on the GPU (splat_trainer_amd.filter3d, csrc/filter3d.hip) against tests/filter3d_oracle.py:
the sampling rate inside its fp64 sandwich over lane, block and camera-group tails; the fused forward / backward against
the plain fp64 definition, bounded by four times the host restatement's own error on the same rows; the autograd wiring
through the rasteriser, bit for bit; and ``MLPScene`` with the filter on.  Every figure is printed before it is asserted
(run with -s to keep them: the filter's observed errors and bounds in profiles/r17_filter3d.txt are that output)."""
import functools

import numpy as np
import pytest
import torch

import filter3d_oracle as fo
import splat_trainer_amd as sta
import visibility_oracle as vo
from helpers import small_scene
from splat_trainer_amd import _lib, synthetic, visibility as vis

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 257, 1000, 4099]        # lane and block tails: 64 lanes, 4 points per lane, 1024 points per block
VS = [1, 3, 4, 5, 64, 65]                    # records fetched four at a time; the frustum kernel's tile of 64, plus one
MARGINS = [0.0, 0.15]
MARGIN = fo.MARGIN


def _note(line: str):
  print(line)


# -------------------------------------------------------------------------------------------------------------- rate
@functools.lru_cache(maxsize=None)
def _ring(V):
  """The ring scene of V cameras and its cloud of 4099 points (every smaller N is a prefix); the oracle reads the float32
  records and focals the kernel reads."""
  cams = fo.ring_cameras(V)
  batch = vo.camera_batch(vis, cams, "cuda")
  records = batch.records().cpu().numpy()
  focal = batch.intrinsics[:, :2].max(dim=1).values.cpu().numpy()
  assert np.array_equal(focal, fo.focal_of(cams[1]))
  return batch, records, focal, fo.ring_points(max(NS), seed=V)


@functools.lru_cache(maxsize=None)
def _bounds(V, margin):
  _, records, focal, points = _ring(V)
  return fo.rate_bounds_fp64(points, records, focal, margin)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("V", VS)
def test_rate_sits_in_the_fp64_sandwich(V, margin):
  batch, records, _, points = _ring(V)
  b = _bounds(V, margin)
  unsampled, undecided = float(np.mean(b["U"] == 0)), float(np.mean(b["L"] != b["U"]))
  behind = float(np.mean((records[:, None, 8:11] * points[None]).sum(-1) + records[:, None, 11] < 0))
  _note(f"rate V={V} margin={margin}: unsampled {unsampled:.3f}  behind a camera {behind:.3f} of the pairs  "
        f"L != U {undecided:.2e}  band pairs {b['band']}")
  assert undecided <= 1e-3 and behind > 0 and unsampled > 0
  if V >= 64:
    assert 0.10 <= unsampled <= 0.30
  device_points = torch.from_numpy(points).cuda()
  for N in NS:
    rate = sta.sampling_rate(batch, device_points[:N], margin=margin, unseen="zero")
    assert rate.shape == (N,) and rate.dtype is torch.float32
    inside = fo.inside_sandwich(rate.cpu().numpy(), {k: v[:N] for k, v in b.items() if k != "band"})
    assert inside.all(), (N, int((~inside).sum()))


def test_rate_on_the_scene_far_from_every_bound():
  batch, records, focal, _ = _ring(65)
  points = fo.far_from_every_bound(1000)
  b = fo.rate_bounds_fp64(points, records, focal, 0.15)
  assert b["band"] == 0 and np.array_equal(b["L"], b["U"])
  rate = sta.sampling_rate(batch, torch.from_numpy(points).cuda(), unseen="zero").cpu().numpy()
  assert fo.inside_sandwich(rate, b).all()
  assert np.array_equal(rate == 0, b["U"] == 0) and 0.4 < np.mean(rate == 0) < 0.6


def test_rate_is_a_function_of_its_inputs():
  batch, _, _, points = _ring(65)
  p = torch.from_numpy(points).cuda()
  first = sta.sampling_rate(batch, p, unseen="zero")
  assert torch.equal(first, sta.sampling_rate(batch, p, unseen="zero"))
  perm = torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(0)).cuda()
  assert torch.equal(sta.sampling_rate(batch, p[perm], unseen="zero"), first[perm])


def test_unseen_points_take_the_lowest_rate_without_a_host_wait():
  batch, _, _, points = _ring(5)
  p = torch.from_numpy(points).cuda()
  zero = sta.sampling_rate(batch, p, unseen="zero")
  batch.records()
  torch.cuda.synchronize()
  previous = torch.cuda.get_sync_debug_mode()
  torch.cuda.set_sync_debug_mode("error")
  try:
    lowest = sta.sampling_rate(batch, p, unseen="min")
  finally:
    torch.cuda.set_sync_debug_mode(previous)
  seen = zero > 0
  assert 0 < int(seen.sum()) < p.shape[0]
  assert torch.equal(lowest[seen], zero[seen])
  assert bool((lowest[~seen] == zero[seen].min()).all())
  nowhere = torch.full((7, 3), 1e4, device="cuda")
  assert sta.sampling_rate(batch, nowhere, unseen="min").abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------------------ filter
def _gaussians(ls, a):
  n = ls.shape[0]
  leaf = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda().requires_grad_(True)
  return sta.Gaussians3D(position=torch.zeros(n, 3, device="cuda"), rotation=torch.zeros(n, 4, device="cuda"),
                         log_scaling=leaf(ls), alpha_logit=leaf(a[:, None]), feature=torch.zeros(n, 3, device="cuda"))


def _vjp(g, out, g_ls, g_a):
  d_ls, d_a = torch.autograd.grad([out.log_scaling, out.alpha_logit],
                                  [g.log_scaling, g.alpha_logit],
                                  [torch.from_numpy(g_ls).cuda(), torch.from_numpy(g_a[:, None]).cuda()], retain_graph=True)
  return d_ls.cpu().numpy(), d_a[:, 0].cpu().numpy()


@pytest.mark.parametrize("N", NS)
def test_filter_matches_the_fp64_definition(N):
  """Bound: four times the error of the host restatement (numpy float32, the kernels' order of operations) against the
  same fp64 values on the same rows -- the device's log1p / expm1 / exp / log are not correctly rounded and their error
  here is unmeasured, so the bound is set by what float32 arithmetic of this form costs, not by a constant."""
  ls, a, rate = fo.random_rows(N, seed=100 + N)
  keep = rate == 0
  c32, c64 = fo.variance_f32(rate), fo.variance_fp64(rate)
  want_ls, want_a = fo.smooth_fp64(ls, a, c64)
  want_p = fo.partials_fp64(ls, a, c64)
  rng = np.random.default_rng(N)
  g_ls, g_a = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
  want_dls, want_da, scale = fo.backward_fp64(ls, a, c64, g_ls, g_a)

  host_ls, host_a = fo.smooth_f32(ls, a, c32)
  host_dls, host_da = fo.backward_f32(ls, a, c32, g_ls, g_a)
  host = dict(zip(("ls'", "a'"), (fo.out_error(host_ls, want_ls), fo.out_error(host_a, want_a))))
  host.update(zip(("d ls'/d ls", "d a'/d a", "d a'/d ls"), fo.partial_errors(fo.partials_f32(ls, a, c32), want_p)))
  host.update({"vjp d_ls": fo.error_on(host_dls, want_dls, scale), "vjp d_a": fo.error_on(host_da, want_da)})

  g = _gaussians(ls, a)
  out = sta.smooth_gaussians(g, torch.from_numpy(rate).cuda(), fo.STRENGTH)
  assert out.position is g.position and out.rotation is g.rotation and out.feature is g.feature
  got_ls, got_a = out.log_scaling.detach().cpu().numpy(), out.alpha_logit.detach()[:, 0].cpu().numpy()
  ones3, zeros3 = np.ones((N, 3), np.float32), np.zeros((N, 3), np.float32)
  ones1, zeros1 = np.ones(N, np.float32), np.zeros(N, np.float32)
  dls_dls, _ = _vjp(g, out, ones3, zeros1)
  da_dls, da_da = _vjp(g, out, zeros3, ones1)
  got_dls, got_da = _vjp(g, out, g_ls, g_a)
  assert all(np.isfinite(t).all() for t in (got_ls, got_a, dls_dls, da_dls, da_da, got_dls, got_da))
  dev = dict(zip(("ls'", "a'"), (fo.out_error(got_ls, want_ls), fo.out_error(got_a, want_a))))
  dev.update(zip(("d ls'/d ls", "d a'/d a", "d a'/d ls"), fo.partial_errors((dls_dls, da_da, da_dls), want_p)))
  dev.update({"vjp d_ls": fo.error_on(got_dls, want_dls, scale), "vjp d_a": fo.error_on(got_da, want_da)})
  _note(f"filter N={N} ({int(keep.sum())} rows with c = 0): " +
          "  ".join(f"{k} device {dev[k]:.2e} bound {MARGIN * host[k]:.2e}" for k in dev))

  # rows without added variance: the input's bits, and the incoming gradient's bits
  assert got_ls[keep].tobytes() == ls[keep].tobytes() and got_a[keep].tobytes() == a[keep].tobytes()
  assert got_dls[keep].tobytes() == g_ls[keep].tobytes() and got_da[keep].tobytes() == g_a[keep].tobytes()
  if (~keep).any():
    assert not np.array_equal(got_ls[~keep], ls[~keep])
  for k in dev:
    assert dev[k] <= MARGIN * host[k], (N, k, dev[k], MARGIN * host[k])


def test_filter_arguments_and_strength_zero():
  ls, a, rate = fo.random_rows(65, seed=9)
  g = _gaussians(ls, a)
  r = torch.from_numpy(rate).cuda()
  assert sta.smooth_gaussians(g, r, 0.0) is g
  with pytest.raises(sta.GsplatHipError, match="HIP device only"):
    sta.smooth_gaussians(g, r.cpu())
  with pytest.raises(ValueError, match="shape"):
    sta.smooth_gaussians(g, r[:64])
  with pytest.raises(ValueError, match="float32"):
    sta.smooth_gaussians(g, r.double())
  # a rate that is not 16-byte aligned (a view) is copied, not misread
  padded = torch.cat([r.new_zeros(1), r])
  shifted = sta.smooth_gaussians(g, padded[1:], fo.STRENGTH)
  assert torch.equal(shifted.log_scaling, sta.smooth_gaussians(g, r, fo.STRENGTH).log_scaling)


# ------------------------------------------------------------------------------------------------------- composition
def _filter_backward(ls, a, rate, strength, g_ls, g_a):
  lib = _lib.load()
  d_ls, d_a = torch.empty_like(ls), torch.empty_like(a)
  _lib.check(lib.gsr_filter3d_backward(ls.data_ptr(), a.data_ptr(), rate.data_ptr(), ls.shape[0], strength,
                                       g_ls.data_ptr(), g_a.data_ptr(), d_ls.data_ptr(), d_a.data_ptr(),
                                       _lib.current_stream_ptr()), "gsr_filter3d_backward")
  return d_ls, d_a


def test_autograd_wiring_through_the_rasteriser():
  """render(smooth(g)) is the render of the materialised smoothed parameters, and the gradients that reach g are the
  filter's backward applied to that render's gradients: bit for bit, so rasteriser parity is not re-derived here."""
  g0, cam = small_scene(300, 64, 48, sh_degree=1, seed=11)
  cam = cam.to("cuda")
  leaves = lambda: sta.Gaussians3D(*(t.clone().cuda().requires_grad_(True) for t in
                                     (g0.position, g0.rotation, g0.log_scaling, g0.alpha_logit, g0.feature)))
  rate = sta.sampling_rate([cam], g0.position.cuda())
  assert bool((rate > 0).all())
  g = leaves()
  image = sta.render_gaussians(sta.smooth_gaussians(g, rate, fo.STRENGTH), cam, use_sh=True).image
  ((image - 0.5) ** 2).mean().backward()

  m = leaves()
  with torch.no_grad():
    smoothed = sta.smooth_gaussians(m, rate, fo.STRENGTH)
  assert not torch.equal(smoothed.log_scaling, m.log_scaling) and not torch.equal(smoothed.alpha_logit, m.alpha_logit)
  s = sta.Gaussians3D(position=m.position, rotation=m.rotation, log_scaling=smoothed.log_scaling.clone().requires_grad_(True),
                      alpha_logit=smoothed.alpha_logit.clone().requires_grad_(True), feature=m.feature)
  image_m = sta.render_gaussians(s, cam, use_sh=True).image
  ((image_m - 0.5) ** 2).mean().backward()
  assert torch.equal(image, image_m)
  assert s.log_scaling.grad.abs().max().item() > 0 and s.alpha_logit.grad.abs().max().item() > 0
  d_ls, d_a = _filter_backward(m.log_scaling.detach(), m.alpha_logit.detach(), rate, fo.STRENGTH,
                               s.log_scaling.grad.contiguous(), s.alpha_logit.grad.contiguous())
  assert torch.equal(g.log_scaling.grad, d_ls) and torch.equal(g.alpha_logit.grad, d_a)
  for name in ("position", "rotation", "feature"):
    assert torch.equal(getattr(g, name).grad, getattr(m, name).grad), name


# -------------------------------------------------------------------------------------------------------------- scene
PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))


def _scene(g, num_images, filter_3d):
  config = sta.MLPSceneConfig(parameters=PARAMETERS, reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
                              color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=3), image_features=8,
                              point_features=8, filter_3d=filter_3d)
  torch.manual_seed(5)                                   # the colour model's initial weights
  scene = config.from_color_gaussians(g, num_images, "cuda", seed=5)
  with torch.no_grad():
    scene.color_table.weight.copy_(0.5 * torch.randn(scene.color_table.weight.shape, generator=torch.Generator().manual_seed(6)))
  return scene


def _by_hand(scene, gaussians, cam, image_idx):
  """MLPScene.render as it stands without the filter, on the given Gaussians."""
  config = sta.pop_raster_config({})
  prefetch = {}
  g2d, depth, idx = sta.project_to_image(gaussians, cam, config, prefetch=prefetch)
  colors = scene.eval_colors(idx, cam, image_idx)
  r = sta.render_projected(idx, g2d, colors.total(1.0), depth, cam, config, _depth_order=prefetch.get("depth_order"))
  return scene.color_model.post_activation(r.image)


def test_scene_with_the_filter():
  g, cams = synthetic.scene_b(500, 64, 48, sh_degree=0, seed=9, num_cameras=3)
  cams = [c.to("cuda") for c in cams]
  plain, scene = _scene(g, 3, 0.0), _scene(g, 3, 0.2)
  with pytest.raises(RuntimeError, match="update_filter"):
    scene.render(cams[0], image_idx=0)
  with pytest.raises(RuntimeError, match="update_filter"):
    scene.query_visibility(cams[0])
  scene.update_filter(cams)
  rate = scene.points.filter_rate
  assert rate.shape == (500,) and bool((rate > 0).all()) and not rate.requires_grad
  assert torch.equal(rate, sta.sampling_rate(cams, scene.points.position.detach()))
  with torch.no_grad():
    filtered = scene.render(cams[0], image_idx=0).image
    unfiltered = plain.render(cams[0], image_idx=0).image
    assert not torch.equal(filtered, unfiltered)
    # filter_3d = 0 is today's scene; filter_3d > 0 is the same pipeline on the smoothed Gaussians
    assert torch.equal(unfiltered, _by_hand(plain, plain.gaussians, cams[0], 0))
    assert torch.equal(filtered, _by_hand(plain, sta.smooth_gaussians(plain.gaussians, rate, 0.2), cams[0], 0))
  assert scene.gaussians.log_scaling is scene.points.log_scaling          # the property stays raw
  assert "filter_rate" not in plain.points.tensors
  assert sorted(plain.state_dict()["points"]["tensors"]) == ["alpha_logit", "feature", "log_scaling", "position",
                                                              "rotation", "visible"]

  # a training step reaches the raw parameters through the filter
  r = scene.render(cams[1], image_idx=1, compute_visibility=True)
  ((r.image - 0.3).pow(2).mean() + scene.reg_loss(r)).backward()
  assert scene.points.log_scaling.grad.abs().max().item() > 0 and scene.points.alpha_logit.grad.abs().max().item() > 0
  scene.add_rendering(1, r)
  scene.step()
  assert torch.equal(scene.points.filter_rate, rate)

  # save / load carries the column
  loaded = scene.config.from_state_dict(scene.state_dict(), 3)
  assert torch.equal(loaded.points.filter_rate, rate) and loaded.points.filter_rate.data_ptr() != rate.data_ptr()
  with torch.no_grad():
    assert torch.equal(loaded.render(cams[2], image_idx=2).image, scene.render(cams[2], image_idx=2).image)

  # the export bakes the filter in
  exported = scene.to_sh_gaussians(cams, [0, 1, 2], epochs=1, sh_degree=1, generator=torch.Generator().manual_seed(0))
  with torch.no_grad():
    smoothed = sta.smooth_gaussians(scene.gaussians, rate, 0.2)
  assert torch.equal(exported.log_scaling, smoothed.log_scaling) and torch.equal(exported.alpha_logit, smoothed.alpha_logit)
  assert not exported.log_scaling.requires_grad and exported.feature.shape == (500, 3, 4)

  # densify keeps the column aligned: kept rows keep their rate, the two children of a split row carry its rate
  gen = torch.Generator().manual_seed(1)
  keep_mask = (torch.rand(500, generator=gen) < 0.7).cuda()
  split_idx = (~keep_mask).nonzero().squeeze(1)[::2]
  scene.split_and_prune(keep_mask, split_idx, generator=torch.Generator(device="cuda").manual_seed(2))
  n_keep = int(keep_mask.sum())
  assert scene.num_points == n_keep + 2 * split_idx.shape[0]
  assert torch.equal(scene.points.filter_rate[:n_keep], rate[keep_mask])
  assert torch.equal(scene.points.filter_rate[n_keep:], rate[split_idx].repeat_interleave(2))
  with torch.no_grad():
    assert torch.isfinite(scene.render(cams[0], image_idx=0).image).all()
  scene.update_filter(cams)
  assert scene.points.filter_rate.shape == (scene.num_points,)
