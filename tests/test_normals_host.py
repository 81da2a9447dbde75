"""The normal-consistency oracle (tests/normals_oracle.py) against facts it does not define -- the depth map of an analytic
plane gives the plane's normal at every interior pixel; autograd's numerical check of the loss and of the splat normals --
and the conditions the GPU tests' input builders keep.  No GPU."""
import pytest
import torch

import normals_oracle as no
from helpers import oracle


@pytest.mark.parametrize("W,H", no.DEPTH_SIZES)
def test_plane_gives_its_own_normal(W, H):
  proj = no.pinhole(W, H).double()
  d, n0 = no.plane_depth(W, H, proj)
  assert bool((d > 0).all())
  n, valid, _ = no.depth_normals(d, proj)
  interior = max(W - 2, 0) * max(H - 2, 0)
  assert int(valid.sum()) == interior
  if interior:
    err = (n[1:-1, 1:-1] - n0).abs().max().item()
    print(f"plane {W}x{H}: fp64 max error {err:.2e}")
    assert err < 1e-12
  border = torch.ones(H, W, dtype=torch.bool)
  border[1:-1, 1:-1] = False
  assert n[border].abs().max().item() == 0 if border.any() else True


def test_fronto_parallel_faces_the_camera():
  proj = no.pinhole(9, 7).double()
  n, valid, _ = no.depth_normals(torch.full((7, 9), 2.5, dtype=torch.float64), proj)
  assert bool(valid[1:-1, 1:-1].all())
  assert (n[1:-1, 1:-1] - torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)).abs().max().item() < 1e-14


def test_fp32_stencil_error_grows_with_the_focal_length():
  """Why the GPU tests take their bound from the oracle's own fp32 error and not from a constant."""
  errs = {}
  for W, H in ((3, 3), (130, 67)):
    proj = no.pinhole(W, H)
    d, n0 = no.plane_depth(W, H, proj.double())
    n32, _, _ = no.depth_normals(d.float(), proj)
    errs[(W, H)] = (n32[1:-1, 1:-1].double() - n0).abs().max().item()
  print("fp32 plane errors", errs)
  assert errs[(3, 3)] < 2e-6 and errs[(3, 3)] < errs[(130, 67)] < 1e-4


def test_punched_pixels_lose_exactly_their_neighbourhood():
  W, H = 17, 5
  proj = no.pinhole(W, H).double()
  d = no.random_depth(W, H, seed=1).double()
  n, valid, _ = no.depth_normals(d, proj)
  dp, lost = no.punched(d)
  n_p, valid_p, _ = no.depth_normals(dp, proj)
  assert torch.equal(valid_p, valid & ~lost)
  assert torch.equal(n_p[~lost], n[~lost]) and n_p[lost].abs().max().item() == 0


def test_thin_axis_takes_the_lowest_index_on_ties():
  ls = torch.tensor([[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [1.0, 2.0, 1.0], [1.0, 1.0, 2.0], [3.0, 2.0, 1.0]])
  assert no.thin_axis(ls).tolist() == [0, 1, 0, 0, 2]


def test_splat_normals_face_the_camera_and_are_columns():
  rot, ls, pos, T = no.splat_inputs(257, seed=2)
  idx = torch.arange(0, 257, 3)
  n = no.splat_normals(rot.double(), ls.double(), pos.double(), idx, T.double())
  p = pos.double()[idx] @ T.double()[:3, :3].t() + T.double()[:3, 3]
  assert bool(((n * p).sum(1) <= 0).all())
  assert (n.norm(dim=1) - 1).abs().max().item() < 1e-6            # (the pose is float32: orthonormal to its rounding)
  cols = T.double()[:3, :3] @ oracle.quat_to_rotmat_xyzw(rot.double()[idx])          # (M, 3, 3): camera-space columns
  k = ls[idx].argmin(dim=1)
  picked = cols[torch.arange(idx.shape[0]), :, k]
  assert ((n - picked).abs().max(dim=1).values.minimum((n + picked).abs().max(dim=1).values)).max().item() < 1e-12


def test_gradcheck_splat_normals():
  rot, ls, pos, T = no.splat_inputs(7, seed=3)
  idx = torch.tensor([0, 2, 3, 6])
  r = rot.double().requires_grad_(True)
  f = lambda r_: no.splat_normals(r_, ls.double(), pos.double(), idx, T.double())     # noqa: E731
  assert torch.autograd.gradcheck(f, (r,), eps=1e-6, atol=1e-7)


def test_gradcheck_loss():
  W, H = 7, 6
  G = no.geometry_image(W, H, seed=4).double()
  G[2, 3, 4] = 0.2                                    # an unseen pixel in the middle: its neighbours lose their normal
  G.requires_grad_(True)
  proj = no.pinhole(W, H).double()
  f = lambda g: no.normal_loss(g, proj, no.ALPHA_MIN)[0]                               # noqa: E731
  assert torch.autograd.gradcheck(f, (G,), eps=1e-6, atol=1e-7)
  L, n_d, valid = no.normal_loss(G, proj, no.ALPHA_MIN)
  L.backward()
  assert 0 < int(valid.sum()) < (W - 2) * (H - 2)
  assert G.grad[~no.touched(valid)].abs().max().item() == 0


def test_loss_is_zero_where_splat_and_depth_normals_agree():
  W, H = 17, 9
  proj = no.pinhole(W, H).double()
  d, n0 = no.plane_depth(W, H, proj)
  A = torch.full((H, W, 1), 0.8, dtype=torch.float64)
  G = torch.cat([n0.expand(H, W, 3) * A, d[..., None] * A, A], -1)
  L, _, valid = no.normal_loss(G, proj, no.ALPHA_MIN)
  assert int(valid.sum()) == (W - 2) * (H - 2) and abs(L.item()) < 1e-13


def test_entry_points_refuse_before_they_launch(built_libs):
  """The argument checks of the header, in its order; every case returns before the device is touched."""
  from splat_trainer_amd import _lib
  lib = _lib.load()
  OK, INVALID, UNSUPPORTED = (_lib.CONSTANTS[k] for k in ("GSR_OK", "GSR_ERR_INVALID_ARGUMENT", "GSR_ERR_UNSUPPORTED"))
  P = 0x10000                                            # a stand-in device address, never read
  assert _lib.ABI_VERSION == 38                          # additive: no signature changed
  assert lib.gsr_normal_loss_blocks(1080, 1920) == 60 * 135 and lib.gsr_normal_loss_blocks(0, 5) == 0
  assert lib.gsr_depth_normals(P, -1, 4, P, P, None) == INVALID
  assert lib.gsr_depth_normals(P, 4, 32769, P, P, None) == UNSUPPORTED
  assert lib.gsr_depth_normals(None, 0, 4, None, None, None) == OK
  assert lib.gsr_depth_normals(P, 4, 4, None, P, None) == INVALID
  assert lib.gsr_normal_loss_forward(P, 4, 4, P, float("nan"), P, P, P, None) == INVALID
  assert lib.gsr_normal_loss_forward(P, 4, 4, P, 0.5, P, None, P, None) == INVALID
  assert lib.gsr_normal_loss_forward(None, 4, 0, None, 0.5, None, None, None, None) == OK
  assert lib.gsr_normal_loss_backward(P, 40000, 4, P, 0.5, P, P, None) == UNSUPPORTED
  assert lib.gsr_normal_loss_backward(P, 4, 4, P, 0.5, None, P, None) == INVALID
  assert lib.gsr_splat_normals_forward(P, P, P, 8, P, -1, P, None, P, None) == INVALID
  assert lib.gsr_splat_normals_forward(None, None, None, 8, None, 0, None, None, None, None) == OK
  assert lib.gsr_splat_normals_forward(P + 4, P, P, 8, P, 4, P, None, P, None) == INVALID
  assert lib.gsr_splat_normals_backward(P, P, P, 8, P, 4, P, P, 4, P, None, None) == INVALID
  assert lib.gsr_splat_normals_backward(P, P, P, 8, P, 4, P, P, 3, P, P, None) == INVALID
  assert lib.gsr_splat_normals_backward(P, P, P, 8, P, 4, P, P, 5, None, P, None) == INVALID


# ---- the builders keep their conditions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", no.SPLAT_N)
def test_splat_builder_conditions(N):
  rot, ls, pos, T = no.splat_inputs(N, seed=10 + N)
  assert bool(no.splat_conditions(rot, ls, pos, T).all())
  two = ls.double().sort(dim=1).values
  assert (two[:, 1] - two[:, 0]).min().item() >= no.SCALE_GAP
  R = T.double()[:3, :3]
  assert (R @ R.t() - torch.eye(3, dtype=torch.float64)).abs().max().item() < 1e-6


@pytest.mark.parametrize("W,H", no.LOSS_SIZES)
def test_geometry_builder_conditions(W, H):
  G = no.geometry_image(W, H, seed=W)
  assert no.geometry_conditions(G)
  _, _, valid = no.normal_loss(G.double(), no.pinhole(W, H).double(), no.ALPHA_MIN)
  assert 0 < int(valid.sum()) < (W - 2) * (H - 2)


def test_small_scene_alpha_shares():
  """The two scenes of the rasteriser tests: the sparse one has between 20 % and 80 % of its pixels at A >= alpha_min; the
  dense one has no pixel within 1e-3 of alpha_min."""
  import splat_trainer_amd as sta
  from helpers import small_scene
  cfg = sta.RasterConfig()
  shares = {}
  for n, seed in ((80, 5), (400, 3)):
    g, cam = small_scene(n, 64, 48, seed=seed)
    pos, ls, rot, al = (t.double() for t in (g.position, g.log_scaling, g.rotation, g.alpha_logit))
    T, proj = cam.T_camera_world.double(), cam.projection.double()
    idx = oracle.frustum_cull(pos, T, proj, cam.image_size, cam.near_plane, cam.far_plane, cfg.margin_tiles * cfg.tile_size)
    g2d, depth, _ = oracle.project(pos, ls, rot, al, idx, T, proj, cfg)
    out = oracle.rasterize(g2d, depth, torch.ones(idx.shape[0], 1, dtype=torch.float64), cam.image_size, cfg)
    A = out.image[..., 0]
    shares[n] = ((A >= no.ALPHA_MIN).double().mean().item(), (A - no.ALPHA_MIN).abs().min().item())
  print("alpha shares", shares)
  assert 0.2 <= shares[80][0] <= 0.8
  assert shares[400][1] > 1e-3
