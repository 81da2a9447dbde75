"""The forward composite hands its per-pair visibility over once per 64 list positions (counted from where a walk
begins) and wherever a walk ends; the backward composite loads its entry state at clamped addresses.  The smallest
shapes at which either can go wrong: one 16x16 tile and a 24x20 image (partial tiles on the right and at the bottom),
list lengths around the multiples of 4 and of 64, segment lengths that do not divide 64, and an opaque stack that ends
the walk in the middle of a 64-block.  Every case is held against the fp64 oracle at 1e-4, must be bit-reproducible,
must deliver the same visibility before and after backward(), and -- DESIGN.md section 4, "forward results
bit-identical" -- must give the same forward bits with and without checkpoints."""
import math

import pytest
import torch

import splat_trainer_amd as sta
from helpers import compare_to_oracle, hip_render_and_grads, oracle_render_and_grads, small_scene

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4, 5, 63, 64, 65, 67, 128, 130)
IMAGES = ((16, 16), (24, 20))
CHECKPOINTED = (4, 20, 60, 64)           # segment_pairs next to 0; 4, 20 and 60 do not divide 64
HUGE = 10 ** 9
EXACT = ("image", "final_T", "visibility", "prune_cost", "split_score", "d_position", "d_log_scaling", "d_rotation",
         "d_alpha_logit", "d_feature")


def _cfg(seg, seg_min=HUGE):
  return sta.RasterConfig(compute_visibility=True, compute_point_heuristic=True, segment_pairs=seg,
                          segment_min_pairs=seg_min)


def _stack(n, w, h, opacity, sigma_px, seed):
  """n splats stacked around the image centre, all of one opacity, at distinct depths."""
  g, cam = small_scene(n, w, h, sh_degree=0, seed=seed, sigma_px=sigma_px)
  gen = torch.Generator().manual_seed(1000 + seed)
  fx = w / (2.0 * math.tan(math.radians(30.0)))
  z = g.position[:, 2]
  u = w / 2 + 3.0 * (torch.rand(n, generator=gen) - 0.5)
  v = h / 2 + 3.0 * (torch.rand(n, generator=gen) - 0.5)
  g.position[:, 0] = (u - w / 2) * z / fx
  g.position[:, 1] = (v - h / 2) * z / fx
  g.alpha_logit[:] = math.log(opacity / (1.0 - opacity))
  return g, cam


def _last(hip):
  """The per-pixel last-contributor index of the frame (kept by the autograd node for the backward pass)."""
  st = hip["rendering"].image.grad_fn.st
  if isinstance(st.last, torch.Tensor):
    return st.last.clone()
  arena = st.segment_buffers[0]                       # the frame driver keeps kernel-only buffers as device addresses
  first = (st.last - arena.data_ptr()) // 4
  return arena.view(torch.int32)[first:first + st.H * st.W].view(st.H, st.W).clone()


def _visibility_read_early(g, cam, cfg):
  gd = sta.Gaussians3D(*(t.clone().cuda().requires_grad_(True) for t in
                         (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
  r = sta.render_gaussians(gd, cam.to("cuda"), cfg, use_sh=True)
  before = r.points.visibility.clone()                 # (what points.visible is cut from)
  visible = r.points.visible.visibility.clone()
  ((r.image.clamp(0, 1) - 0.5) ** 2).mean().backward()
  return before, visible, r.points.visibility.clone()


def _check(label, g, cam, orc, cfg):
  hip = hip_render_and_grads(g, cam, cfg, use_sh=True)
  compare_to_oracle(label, hip, orc, 1e-4)
  again = hip_render_and_grads(g, cam, cfg, use_sh=True)
  for k in EXACT:
    assert torch.equal(hip[k], again[k]), (label, k)            # two renders: the same bits
  assert torch.equal(_last(hip), _last(again)), label
  before, visible, after = _visibility_read_early(g, cam, cfg)
  assert torch.equal(before, after), label                       # read before backward() == what backward delivers
  assert torch.equal(visible, after[after > 0]), label
  assert torch.equal(after, hip["visibility"]), label            # ... and reading early changes nothing
  return hip


def _check_all_settings(label, g, cam, heavy=()):
  orc = oracle_render_and_grads(g, cam, _cfg(0), use_sh=True)
  whole = _check(f"{label} seg=0", g, cam, orc, _cfg(0))
  whole_last = _last(whole)
  for seg in CHECKPOINTED:
    cut = _check(f"{label} seg={seg}", g, cam, orc, _cfg(seg))
    for k in ("image", "final_T", "visibility"):                 # the checkpointed walk is the same walk, bit for bit
      assert torch.equal(cut[k], whole[k]), (label, seg, k)
    assert torch.equal(_last(cut), whole_last), (label, seg)
  for seg, seg_min in heavy:                                     # passes A / C / D
    _check(f"{label} seg={seg} min={seg_min}", g, cam, orc, _cfg(seg, seg_min))
  return whole


@pytest.mark.parametrize("w,h", IMAGES)
@pytest.mark.parametrize("n", LENGTHS)
def test_low_opacity_stack(n, w, h):
  """No pixel saturates: every walk runs to the end of its range, whatever the length."""
  g, cam = _stack(n, w, h, opacity=0.03, sigma_px=2.0, seed=n)
  # the 130-pair list also as a heavy tile: 33 segments of 4 pairs, and (automatic length) segments of 64, 64 and 2
  heavy = ((4, 8), (-1, 8)) if n == 130 else ()
  whole = _check_all_settings(f"handover n={n} {w}x{h}", g, cam, heavy)
  if (w, h) == (16, 16):
    assert whole["num_overlaps"] == n                            # one tile: its list is the n splats
  else:
    assert whole["num_overlaps"] >= n
  assert float(whole["final_T"].min()) > 1e-3


@pytest.mark.parametrize("w,h", IMAGES)
def test_opaque_stack_ends_the_walk_inside_a_block(w, h):
  """Opacity at the clamp (0.99), splats wider than the image: every pixel saturates after a few pairs, the walk breaks
  in the middle of its first 64-block and hands over only the positions it reached.  (Not above the clamp: two clamped
  alphas in a row leave T = 0.01^2, which IS the T_eps of 1e-4 -- on one side of it in fp32, on the other in the fp64
  oracle, whatever the kernel does.)"""
  g, cam = _stack(100, w, h, opacity=0.99, sigma_px=16.0, seed=7)
  whole = _check_all_settings(f"handover opaque {w}x{h}", g, cam, heavy=((4, 8),))
  assert float(whole["final_T"].max()) < 1e-4
  last = _last(whole)
  assert 0 < int(last.max()) < 64                                # the walk ended inside the first block
  assert int((whole["visibility"] > 0).sum()) <= int(last.max())
