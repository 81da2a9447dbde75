"""The normal-consistency kernels (csrc/normals.hip) on the GPU against the fp64 oracle (tests/normals_oracle.py), then
through the rasteriser stage by stage, end to end, and through MLPScene and Trainer.

Tolerance of a kernel against the fp64 oracle, per output tensor: 4 x the largest error of the oracle's own formulas
evaluated in fp32 on the CPU on the same inputs, plus 2^-22 max|oracle| (``normals_oracle.bound``): measured from the
oracle, never from the kernel.  Every figure is printed before it is asserted."""
import pytest
import torch

import normals_oracle as no
import splat_trainer_amd as sta
from helpers import oracle, rel_err, small_scene
from test_gpu_trainer import _config, dataset  # noqa: F401  (the tiny TensorDataset and its training configuration)

pytestmark = pytest.mark.gpu
CFG = sta.RasterConfig()


def within(label: str, got: torch.Tensor, fp32: torch.Tensor, ref: torch.Tensor) -> None:
  got, ref = got.detach().double().cpu(), ref.detach().double()
  err = (got - ref).abs().max().item() if ref.numel() else 0.0
  limit = no.bound(fp32, ref)
  print(f"{label}: max error {err:.3e}  bound {limit:.3e}  max|oracle| {ref.abs().max().item() if ref.numel() else 0:.3e}")
  assert err <= limit, (label, err, limit)


def bit_zero(t: torch.Tensor) -> bool:
  return not bool(t.contiguous().view(torch.int32).bitwise_and(0x7FFFFFFF).any())      # +0 or -0, no NaN


def _gaussians(rot, ls, pos, requires_grad=True):
  N = rot.shape[0]
  return sta.Gaussians3D(position=pos.cuda(), rotation=rot.clone().cuda().requires_grad_(requires_grad),
                         log_scaling=ls.cuda(), alpha_logit=torch.zeros(N, 1, device="cuda"),
                         feature=torch.zeros(N, 1, device="cuda"))


def _camera(T, W=64, H=48):
  return sta.CameraParams(T_camera_world=T.cuda(), projection=no.pinhole(W, H).cuda(), image_size=(W, H))


# ---- splat normals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("N", no.SPLAT_N)
def test_splat_normals(N, every):
  rot, ls, pos, T = no.splat_inputs(N, seed=10 + N)
  assert bool(no.splat_conditions(rot, ls, pos, T).all())
  idx = torch.arange(0, N, every)
  g = torch.randn(idx.shape[0], 3, generator=torch.Generator().manual_seed(N))
  gd = _gaussians(rot, ls, pos)
  n = sta.splat_normals(gd, idx.cuda(), _camera(T))
  (n * g.cuda()).sum().backward()
  results = {}
  for dtype in (torch.float64, torch.float32):
    r = rot.detach().clone().to(dtype).requires_grad_(True)
    o = no.splat_normals(r, ls.to(dtype), pos.to(dtype), idx, T.to(dtype))
    (o * g.to(dtype)).sum().backward()
    results[dtype] = (o.detach(), r.grad)
  label = f"splat normals N={N} every={every}"
  assert n.shape == (idx.shape[0], 3) and gd.rotation.grad.shape == (N, 4)
  within(label + " forward", n, results[torch.float32][0], results[torch.float64][0])
  within(label + " d_rotation", gd.rotation.grad, results[torch.float32][1], results[torch.float64][1])
  outside = torch.ones(N, dtype=torch.bool)
  outside[idx] = False
  assert bit_zero(gd.rotation.grad[outside.cuda()])
  assert gd.rotation.grad[idx.cuda()].abs().max() > 0


def test_geometry_features_are_the_normals_the_depth_and_one():
  rot, ls, pos, T = no.splat_inputs(257, seed=5)
  idx = torch.arange(0, 257, 3).cuda()
  cam = _camera(T)
  gd = _gaussians(rot, ls, pos)
  depth = (1.0 + torch.rand(idx.shape[0], 1, generator=torch.Generator().manual_seed(1))).cuda().requires_grad_(True)
  f = sta.geometry_features(gd, idx, depth, cam)
  g = torch.randn(idx.shape[0], 5, generator=torch.Generator().manual_seed(2)).cuda()
  (f * g).sum().backward()
  gd3 = _gaussians(rot, ls, pos)
  n = sta.splat_normals(gd3, idx, cam)
  (n * g[:, :3]).sum().backward()
  assert f.shape == (idx.shape[0], 5)
  assert torch.equal(f[:, :3], n) and torch.equal(f[:, 3:4], depth) and bool((f[:, 4] == 1).all())
  assert torch.equal(gd.rotation.grad, gd3.rotation.grad) and torch.equal(depth.grad, g[:, 3:4])


def test_scale_ties_take_the_lowest_index():
  rot, _, pos, T = no.splat_inputs(4, seed=6)
  ls = torch.tensor([[-1.0, -1.0, -1.0], [0.5, -1.0, -1.0], [-1.0, 0.5, -1.0], [-1.0, -1.0, 0.5]])
  n = sta.splat_normals(_gaussians(rot, ls, pos, requires_grad=False), torch.arange(4).cuda(), _camera(T)).cpu().double()
  cols = T.double()[:3, :3] @ oracle.quat_to_rotmat_xyzw(rot.double())                  # (4, 3, 3): camera-space columns
  distance = torch.minimum((cols - n[:, :, None]).abs().amax(1), (cols + n[:, :, None]).abs().amax(1))      # (4, 3) per axis
  print("tie rule: distance of the output to each column\n", distance)
  assert distance.argmin(1).tolist() == [0, 1, 0, 0]
  assert distance.min(1).values.max().item() < 1e-5 and distance.sort(1).values[:, 1].min().item() > 1e-2


def test_splat_normals_without_rows():
  rot, ls, pos, T = no.splat_inputs(5, seed=7)
  gd = _gaussians(rot, ls, pos)
  empty = torch.zeros(0, dtype=torch.int64, device="cuda")
  assert sta.splat_normals(gd, empty, _camera(T)).shape == (0, 3)
  assert sta.geometry_features(gd, empty, torch.zeros(0, 1, device="cuda"), _camera(T)).shape == (0, 5)
  with pytest.raises(sta.GsplatHipError, match="HIP device only"):
    sta.splat_normals(gd, torch.arange(5), _camera(T))


# ---- depth normals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", no.DEPTH_SIZES)
def test_depth_normals_of_a_plane(W, H):
  proj = no.pinhole(W, H)
  d, n0 = no.plane_depth(W, H, proj.double())
  d32 = d.float()
  n = sta.depth_normals(d32.cuda(), proj.cuda()).cpu()
  assert n.shape == (H, W, 3)
  border = torch.ones(H, W, dtype=torch.bool)
  border[1:-1, 1:-1] = False
  assert bit_zero(n[border])
  if W < 3 or H < 3:
    assert bit_zero(n)
    return
  n32, valid32, _ = no.depth_normals(d32, proj)
  n64, valid64, _ = no.depth_normals(d32.double(), proj.double())
  assert bool(valid64[1:-1, 1:-1].all())
  within(f"plane {W}x{H} against n0", n[1:-1, 1:-1], n32[1:-1, 1:-1], n0.expand(H - 2, W - 2, 3))
  within(f"plane {W}x{H} against the oracle", n, n32, n64)


@pytest.mark.parametrize("W,H", [s for s in no.DEPTH_SIZES if min(s) >= 3])
def test_depth_normals_with_holes(W, H):
  proj = no.pinhole(W, H)
  d = no.random_depth(W, H, seed=W + H)
  dp, lost = no.punched(d)
  n = sta.depth_normals(d.cuda(), proj.cuda()).cpu()
  n_p = sta.depth_normals(dp.cuda(), proj.cuda()).cpu()
  n32, _, _ = no.depth_normals(d, proj)
  n64, valid, _ = no.depth_normals(d.double(), proj.double())
  within(f"random depth {W}x{H}", n, n32, n64)
  assert torch.equal(n.abs().sum(-1) > 0, valid)
  print(f"holes {W}x{H}: {int(lost.sum())} pixels lose their normal")
  assert bit_zero(n_p[lost]) and torch.equal(n_p[~lost], n[~lost])


def test_depth_normals_of_an_empty_image():
  assert sta.depth_normals(torch.zeros(0, 7, device="cuda"), no.pinhole(7, 1).cuda()).shape == (0, 7, 3)


# ---- the loss ------------------------------------------------------------------------------------------------------------
def _loss_on_gpu(G: torch.Tensor, proj: torch.Tensor, scale: float = 1.7):
  Gc = G.detach().cuda().requires_grad_(True)
  L, n_d = sta.normal_consistency_loss(Gc, proj.cuda(), alpha_min=no.ALPHA_MIN, return_normals=True)
  (L * scale).backward()
  return L.detach().cpu(), n_d.cpu(), Gc.grad.cpu()


def _loss_oracle(G: torch.Tensor, proj: torch.Tensor, dtype, scale: float = 1.7):
  Go = G.detach().clone().to(dtype).requires_grad_(True)
  L, n_d, valid = no.normal_loss(Go, proj.to(dtype), no.ALPHA_MIN)
  (L * scale).backward()
  return L.detach(), n_d.detach(), Go.grad, valid


def _check_loss(label: str, G: torch.Tensor, proj: torch.Tensor):
  L, n_d, grad = _loss_on_gpu(G, proj)
  L32, n32, g32, _ = _loss_oracle(G, proj, torch.float32)
  L64, n64, g64, valid = _loss_oracle(G, proj, torch.float64)
  print(f"{label}: {int(valid.sum())} valid pixels of {valid.numel()}, L = {L.item():.8f}")
  within(label + " L", L.reshape(1), L32.reshape(1), L64.reshape(1))
  within(label + " n_d", n_d, n32, n64)
  for c, name in enumerate(("dN^x", "dN^y", "dN^z", "dD", "dA")):
    within(f"{label} {name}", grad[..., c], g32[..., c], g64[..., c])
  assert torch.equal(n_d.abs().sum(-1) > 0, valid)
  assert bit_zero(grad[~no.touched(valid)])
  return L, n_d, grad, valid


@pytest.mark.parametrize("W,H", no.LOSS_SIZES)
def test_loss_matches_the_oracle(W, H):
  G = no.geometry_image(W, H, seed=W)
  assert no.geometry_conditions(G)
  proj = no.pinhole(W, H)
  L, n_d, grad, valid = _check_loss(f"loss {W}x{H}", G, proj)
  assert 0 < int(valid.sum()) < (W - 2) * (H - 2) and bool((~no.touched(valid)).any())
  again = _loss_on_gpu(G, proj)
  assert torch.equal(L, again[0]) and torch.equal(n_d, again[1]) and torch.equal(grad, again[2])


def test_loss_of_an_empty_image():
  G = torch.zeros(0, 4, 5, device="cuda", requires_grad=True)
  L, n_d = sta.normal_consistency_loss(G, no.pinhole(4, 1).cuda(), return_normals=True)
  assert L.item() == 0 and n_d.shape == (0, 4, 3)
  with pytest.raises(ValueError, match="geometry_image must be"):
    sta.normal_consistency_loss(torch.zeros(4, 4, 3, device="cuda"), no.pinhole(4, 4).cuda())


# ---- through the rasteriser ------------------------------------------------------------------------------------------------
def _on_gpu(g):
  return sta.Gaussians3D(*(t.clone().cuda().requires_grad_(True) for t in
                           (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))


def _rgb(M: int) -> torch.Tensor:
  return torch.rand(M, 3, generator=torch.Generator().manual_seed(8))


def test_geometry_image_stage_by_stage():
  g, cam = small_scene(80, 64, 48, seed=5)
  W, H = cam.image_size
  gd, camd = _on_gpu(g), cam.to("cuda")
  with torch.no_grad():
    g2d, depth, idx = sta.project_to_image(gd, camd, CFG)
    feats = torch.cat([_rgb(idx.shape[0]).cuda(), sta.geometry_features(gd, idx, depth, camd)], 1)
    r = sta.render_projected(idx, g2d, feats, depth, camd, CFG)
  assert r.image.shape == (H, W, 8)
  out = oracle.rasterize(g2d.cpu().double(), depth.cpu().double(), feats.cpu().double(), (W, H), CFG)
  share = (out.image[..., 7] >= no.ALPHA_MIN).double().mean().item()
  e_image, e_alpha = rel_err(r.image, out.image), rel_err(r.image[..., 7], 1.0 - out.final_T)
  e_alpha_gpu = rel_err(r.image[..., 7], 1.0 - r.final_transmittance)
  print(f"stage: share of pixels at A >= {no.ALPHA_MIN}: {share:.3f}; rel err of the 8-channel image {e_image:.2e}, of A "
        f"against 1 - final T {e_alpha:.2e} (oracle) {e_alpha_gpu:.2e} (GPU)")
  assert 0.2 <= share <= 0.8
  assert e_image < 1e-4 and e_alpha < 1e-4 and e_alpha_gpu < 1e-4
  _, _, _, valid = _check_loss("stage: loss of the GPU's geometry image", r.image[..., 3:8].cpu().contiguous(),
                               cam.projection.float())
  assert int(valid.sum()) > 100


def test_end_to_end_gradients():
  g, cam = small_scene(400, 64, 48, seed=3)
  W, H = cam.image_size
  gd, camd = _on_gpu(g), cam.to("cuda")
  g2d, depth, idx = sta.project_to_image(gd, camd, CFG)
  rgb = _rgb(idx.shape[0])
  r = sta.render_projected(idx, g2d, torch.cat([rgb.cuda(), sta.geometry_features(gd, idx, depth, camd)], 1), depth, camd, CFG)
  L = sta.normal_consistency_loss(r.image[..., 3:8], camd.projection, alpha_min=no.ALPHA_MIN)
  L.backward()

  pos, rot, ls, al = (t.clone().double().requires_grad_(True) for t in (g.position, g.rotation, g.log_scaling, g.alpha_logit))
  T, proj = cam.T_camera_world.double(), cam.projection.double()
  oidx = oracle.frustum_cull(pos, T, proj, cam.image_size, cam.near_plane, cam.far_plane, CFG.margin_tiles * CFG.tile_size)
  assert torch.equal(oidx, idx.cpu())
  og2d, odepth, _ = oracle.project(pos, ls, rot, al, oidx, T, proj, CFG)
  ofeats = torch.cat([rgb.double(), no.geometry_features(rot, ls, pos, oidx, odepth, T)], 1)
  out = oracle.rasterize(og2d, odepth, ofeats, (W, H), CFG)
  oL, _, valid = no.normal_loss(out.image[..., 3:8], proj, no.ALPHA_MIN)
  oL.backward()
  margin = (out.image[..., 7].detach() - no.ALPHA_MIN).abs().min().item()
  errs = dict(L=abs(L.item() - oL.item()) / abs(oL.item()), rotation=rel_err(gd.rotation.grad, rot.grad),
              position=rel_err(gd.position.grad, pos.grad), log_scaling=rel_err(gd.log_scaling.grad, ls.grad),
              alpha_logit=rel_err(gd.alpha_logit.grad, al.grad))
  print(f"end to end: L = {L.item():.6f} (oracle {oL.item():.6f}), {int(valid.sum())} valid pixels, nearest A to alpha_min "
        f"{margin:.3e}; rel errs {({k: f'{v:.2e}' for k, v in errs.items()})}")
  assert margin > 1e-3
  for t in (rot.grad, pos.grad, ls.grad, al.grad):
    assert t.abs().max() > 0
  assert all(v < 1e-4 for v in errs.values()), errs


# ---- MLPScene and Trainer --------------------------------------------------------------------------------------------------
PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))


def test_scene_renders_a_geometry_image():
  g, cam = small_scene(400, 64, 48, seed=3)
  config = sta.MLPSceneConfig(parameters=PARAMETERS, reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
                              color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=3), image_features=8,
                              point_features=8)
  torch.manual_seed(3)
  scene = config.from_color_gaussians(g, 2, "cuda", seed=3)
  camd = cam.to("cuda")
  plain = scene.render(camd, 0)
  again = scene.render(camd, 0)
  geo = scene.render(camd, 0, render_geometry=True)
  assert plain.geometry_image is None and torch.equal(plain.image, again.image)
  assert geo.image.shape == (48, 64, 3) and 0 <= geo.image.min() and geo.image.max() <= 1
  assert geo.geometry_image.shape == (48, 64, 5) and geo.geometry_image.requires_grad
  e = rel_err(geo.image, plain.image)
  print(f"scene: colour of the 8-channel render against the 3-channel one, rel err {e:.2e}")
  assert e < 1e-4
  sta.normal_consistency_loss(geo.geometry_image, camd.projection).backward()
  assert scene.points.tensors["rotation"].grad.abs().max() > 0
  assert geo.detach().geometry_image is not None and not geo.detach().geometry_image.requires_grad


class _Values(sta.NullLogger):
  def __init__(self):
    self.values = {}

  def log_values(self, name, data):
    self.values.setdefault(name, []).append(dict(data))


def _two_steps(config, data, spy=None):
  torch.manual_seed(2)
  logger = _Values()
  trainer = sta.Trainer.initialize(config, data, logger)
  if spy is not None:
    step = trainer.scene.step

    def spied():
      spy.append(trainer.scene.points.tensors["rotation"].grad.abs().max().item())
      step()
    trainer.scene.step = spied
  for i in (0, 2):
    trainer.training_step(trainer.load_batch(torch.tensor([i])))
  torch.cuda.synchronize()
  return trainer, logger


def test_trainer_adds_the_normal_term(dataset, tmp_path):   # noqa: F811
  grads = []
  trainer, logger = _two_steps(_config(tmp_path, save_output=False, log_interval=1, log_details=False, normal_weight=0.05,
                                       normal_from=0.0), dataset, spy=grads)
  losses = logger.values["train/loss"]
  print("trainer: logged losses", losses, "largest |d rotation| before each step", grads)
  assert len(losses) == 2 and all(torch.isfinite(torch.tensor(entry["normal"])) and entry["normal"] > 0 for entry in losses)
  assert list(losses[0]) == ["l1", "mse", "ssim", "reg", "normal", "total"]
  assert len(grads) == 2 and all(v > 0 for v in grads)


def test_trainer_without_the_term_is_unchanged(dataset, tmp_path):   # noqa: F811
  from test_gpu_trainer import _tree_equal
  base = dict(save_output=False, log_interval=1, log_details=False)
  plain, plain_log = _two_steps(_config(tmp_path / "a", **base), dataset)
  off, off_log = _two_steps(_config(tmp_path / "b", **base, normal_weight=0.0, normal_from=0.0, normal_alpha_min=0.3), dataset)
  late, _ = _two_steps(_config(tmp_path / "c", **base, normal_weight=0.05, normal_from=0.9), dataset)
  _tree_equal(plain.scene.state_dict(), off.scene.state_dict(), "state")
  _tree_equal(plain.scene.state_dict(), late.scene.state_dict(), "state (before normal_from)")
  assert plain_log.values["train/loss"] == off_log.values["train/loss"] and "normal" not in off_log.values["train/loss"][0]
