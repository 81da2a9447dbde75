"""The per-splat and sort kernels of a frame request their loads before the device count is known, at positions clamped
to the capacity (prims.hip: rs_hist / rs_scatter; geometry.hip: cull_count / cull_write / project_sh_fwd; binning.hip:
tile_count; reduce_grad batches its chunk loads).  What that can get wrong shows at the edges: one element, sizes around a wave span and a block's
tile, a count far below the capacity (zero included), a last block that is not full.  Everything here is bit-exact
against a CPU reference or against the other call form, which runs none of the fused kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

import splat_trainer_amd as sta
from helpers import hip_render_and_grads, oracle, rel_err
from splat_trainer_amd import _lib, synthetic

pytestmark = pytest.mark.gpu


def _ptr(t):
  return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a: np.ndarray) -> torch.Tensor:
  return torch.from_numpy(a.view(np.int32).copy()).cuda()


def _host(t: torch.Tensor) -> np.ndarray:
  return t.cpu().numpy().view(np.uint32)


def _sort(keys, bits, two, count=None):
  """Sorts `keys` (every buffer holds exactly len(keys) words: a read behind the capacity leaves the allocation) with
  iota values and, `two`, a second random value array; returns the first `count` sorted (keys, vals, vals2) and the
  stable CPU reference of the same prefix."""
  lib = _lib.load()
  cap = keys.shape[0]
  n = cap if count is None else count
  rng = np.random.default_rng(cap * 31 + bits)
  vals2 = rng.integers(0, 2 ** 32, size=cap, dtype=np.uint64).astype(np.uint32)
  ka, v2a = _dev(keys), _dev(vals2) if two else None
  va, kb, vb = (torch.zeros_like(ka) for _ in range(3))
  v2b = torch.zeros_like(ka) if two else None
  n_dev = torch.tensor([count], dtype=torch.int32, device="cuda") if count is not None else None
  nbytes = lib.gsr_sort_workspace_bytes(cap)
  ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
  if two:
    where = _lib.check(lib.gsr_sort_pairs2_u32(_ptr(ka), _ptr(va), _ptr(v2a), _ptr(kb), _ptr(vb), _ptr(v2b), cap, 1, 0,
                                               bits, _ptr(ws), nbytes, _ptr(n_dev), _stream()), "sort2")
  else:
    where = _lib.check(lib.gsr_sort_pairs_u32(_ptr(ka), _ptr(va), _ptr(kb), _ptr(vb), cap, 1, 0, bits, _ptr(ws), nbytes,
                                              _ptr(n_dev), _stream()), "sort")
  k, v, v2 = (kb, vb, v2b) if where == 1 else (ka, va, v2a)
  order = np.argsort(keys[:n], kind="stable")
  got = (_host(k)[:n], _host(v)[:n], _host(v2)[:n] if two else None)
  want = (keys[:n][order], order.astype(np.uint32), vals2[:n][order] if two else None)
  return got, want


def _keys(n, bits, seed):
  rng = np.random.default_rng(seed)
  keys = rng.integers(0, 2 ** bits, size=n, dtype=np.uint64).astype(np.uint32)
  keys[rng.integers(0, n, size=n // 3)] = keys[0]            # plenty of ties: stability is visible
  return keys


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("bits", [27, 13])                   # three 9-bit passes / two 8-bit passes
@pytest.mark.parametrize("n", [1, 64, 1023, 1024, 1025, 4097])
def test_sort_at_the_edges_of_wave_and_tile(n, bits, two):
  got, want = _sort(_keys(n, bits, n + bits), bits, two)
  for g, w in zip(got, want):
    if w is not None:
      assert np.array_equal(g, w)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("bits", [27, 13])
@pytest.mark.parametrize("count", [0, 1, 1500])
def test_sort_with_a_device_count_below_the_capacity(count, bits, two):
  """Capacity 2048 = two tiles; the count leaves the second tile empty (0, 1) or partly filled (1500).  The slack holds
  plausible keys, which must not reach the counted prefix."""
  got, want = _sort(_keys(2048, bits, count + bits), bits, two, count=count)
  for g, w in zip(got, want):
    if w is not None:
      assert np.array_equal(g, w)


@pytest.fixture(scope="module")
def cull_scene():
  g, cams = synthetic.scene_b(5000, 640, 360, sh_degree=0, seed=2, radius=1.2)    # ~40 % in view
  return g.position, cams[3]


@pytest.mark.parametrize("view", ["all", "none", "half"])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5000])
def test_cull_at_the_edges_of_the_wave_span(cull_scene, n, view):
  pos, cam = cull_scene
  cfg = sta.RasterConfig()
  p = pos[:n].clone()
  if view == "all":
    centre = torch.linalg.inv(cam.T_camera_world) @ torch.tensor([0., 0., 0.5 * (cam.near_plane + cam.far_plane), 1.])
    p = 1e-3 * p + centre[:3]                                  # a small cloud on the optical axis
  elif view == "none":
    p = p + 1000.0
  idx = sta.frustum_cull(p.cuda(), cam.to("cuda"), cfg).cpu()
  want = oracle.frustum_cull(p, cam.T_camera_world, cam.projection, cam.image_size, cam.near_plane, cam.far_plane,
                             cfg.margin_tiles * cfg.tile_size)
  assert idx.dtype == torch.int64
  if idx.numel() > 1:
    assert (idx[1:] > idx[:-1]).all()
  if view == "all":
    assert want.numel() == n and torch.equal(idx, want)
  elif view == "none":
    assert want.numel() == 0 and idx.numel() == 0
  else:
    if n >= 1023:
      assert 0.1 * n < want.numel() < 0.9 * n
    assert len(set(idx.tolist()) ^ set(want.tolist())) <= 1, n   # an fp32 tie exactly on a frustum plane


CFG = sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True)
GRADS = ("d_position", "d_log_scaling", "d_rotation", "d_alpha_logit", "d_feature")


def _per_visible(t, idx, n):
  """A per-point output as one value per visible splat: the one-call form returns N rows, the three-call form M."""
  t = t.detach().reshape(t.shape[0], -1)
  return t[idx] if t.shape[0] == n and idx.numel() != n else t


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [300, 1000])
def test_partly_visible_frame_equals_the_three_call_form(n, deg):
  """A camera that sees part of the scene (M < N, the last block of the per-splat kernels not full).  The one-call form
  runs the fused projection + SH kernel behind the cull's device count; the three-call form knows M on the host and runs
  the separate projection and SH kernels.
  Bit for bit: the image, everything the composite kernels leave per point (visibility, prune cost, split score), depths,
  screen scales and the colour gradient.  The four geometry gradients: to 1e-6 of the tensor's largest magnitude, the
  bound tests/test_gpu_render.py sets for the two forms -- they come out of differently fused sweeps (K2 backward alone
  against K2 backward + the colour gradient's position term), same arithmetic, other fma contractions: a few fp32
  roundings (6e-8 each) on terms of the size of the result."""
  g, cams = synthetic.scene_b(n, 64, 48, sh_degree=deg, seed=7 + deg, radius=0.6, sigma_px=2.5)   # camera inside the cloud
  cam = cams[3]
  one = hip_render_and_grads(g, cam, CFG, use_sh=True)
  three = hip_render_and_grads(g, cam, CFG, use_sh=True, three_call=True)
  idx = one["idx"]
  m = idx.numel()
  print(f"N {n} M {m} overlaps {one['num_overlaps']}")
  assert 0 < m < n and m % 256 != 0
  assert torch.equal(idx, three["idx"])
  assert one["image"].abs().max() > 0
  for k in GRADS[:4]:
    print(f"  {k:14s} rel err one-call vs three-call {rel_err(one[k], three[k]):.3e}")
  for k in ("image", "d_feature"):
    assert torch.equal(one[k], three[k]), k
  for k in ("screen_scale", "depth", "visibility", "prune_cost", "split_score"):
    assert torch.equal(_per_visible(one[k], idx, n), _per_visible(three[k], idx, n)), k
  for k in GRADS[:4]:
    assert rel_err(one[k], three[k]) < 1e-6, k
  # rows the camera did not see: exactly zero gradient in every tensor
  unseen = torch.ones(n, dtype=torch.bool, device="cuda")
  unseen[idx] = False
  for k in GRADS:
    assert one[k][unseen].abs().max().item() == 0, k


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [300, 1000])
def test_one_call_sh_gradient_equals_the_dense_sh_backward(n, deg):
  """The one-call backward's d_sh against gsr_sh_backward_dense applied to the same frame's colour gradient -- taken from
  the three-call form, whose image and composite backward are the same bits -- through the inverse map of the same
  indexes.  Bit for bit: whichever kernel forms d_sh inside the frame's backward has to give the dense kernel's bits."""
  lib = _lib.load()
  g, cams = synthetic.scene_b(n, 64, 48, sh_degree=deg, seed=7 + deg, radius=0.6, sigma_px=2.5)
  cam = cams[3]
  one = hip_render_and_grads(g, cam, CFG, use_sh=True)
  gd = sta.Gaussians3D(*(t.clone().cuda().requires_grad_(True) for t in
                         (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
  camd = cam.to("cuda")
  g2d, depth, idx = sta.project_to_image(gd, camd, CFG)
  feats = sta.evaluate_sh_at(gd.feature, gd.position, idx, camd.camera_position)
  feats.retain_grad()
  r = sta.render_projected(idx, g2d, feats, depth, camd, CFG)
  ((r.image.clamp(0, 1) - 0.5) ** 2).mean().backward()
  assert torch.equal(r.image.detach(), one["image"])
  dcol = feats.grad.contiguous()
  m, k = idx.numel(), (deg + 1) ** 2
  assert dcol.shape == (m, 3) and 0 < m < n and dcol.abs().max() > 0
  inv = torch.empty(n, dtype=torch.int32, device="cuda")
  _lib.check(lib.gsr_inverse_map(_ptr(idx), m, n, _ptr(inv), _stream()), "inverse map")
  d_sh = torch.full((n, 3, k), float("nan"), device="cuda")
  pos, sh, cam_pos = gd.position.detach().contiguous(), gd.feature.detach().contiguous(), camd.camera_position.contiguous()
  _lib.check(lib.gsr_sh_backward_dense(_ptr(dcol), _ptr(sh), _ptr(pos), _ptr(inv), m, n, k, _ptr(cam_pos), None, _ptr(d_sh),
                                       None, _stream()), "sh backward dense")
  assert torch.equal(one["d_feature"], d_sh)
