"""The neural colour model on the GPU (csrc/color_model.hip, splat_trainer_amd.color_model) against the fp64 restatement
(tests/color_model_oracle.py): the forward against the oracle with the kernels' f16 operand rounding, the forward and
every gradient against plain fp64 next to the reference's own fp16-autocast path, the golden data made from the
reference's modules, one-sided upstream gradients, the underflow guard, the camera gradient, bit-reproducibility, M = 0,
the error cases, the MLPScene.render + reg_loss flow through project_to_image / render_projected, and a short fit."""
import os

import numpy as np
import pytest
import torch

import color_model_oracle as cmo
import splat_trainer_amd as sta
from splat_trainer_amd import synthetic
from splat_trainer_amd.color_model import ColorModel, ColorModelConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "color_model_ref.npz"))
CONFIGS = {0: (16, 32, 32, 1, 5), 1: (16, 32, 32, 2, 3)}       # (P, G, H, L, S) of the golden configs


def _model(c, seed=0):
  P, G, H, L, S = CONFIGS[c]
  torch.manual_seed(seed)
  m = ColorModel(ColorModelConfig(hidden_features=H, hidden_layers=L, sh_degree=S), glo_features=G, point_features=P)
  with torch.no_grad():
    for k, p in m.named_parameters():
      if k.endswith("bias"):
        p.uniform_(-0.5, 0.5)
  return m.cuda()


def _inputs(c, M, seed=1):
  P, G = CONFIGS[c][:2]
  gen = torch.Generator().manual_seed(seed)
  pf = torch.randn(M, P, generator=gen)
  pos = torch.randn(M, 3, generator=gen) * 2
  cam = torch.tensor([0.3, -0.2, 0.5])
  glo = torch.randn(1, G, generator=gen) * 0.5
  dd = torch.randn(M, 3, generator=gen)
  ds = torch.randn(M, 3, generator=gen)
  return pf, pos, cam, glo, dd, ds


def _native(model, pf, pos, cam, glo, dd, ds, cam_grad=True):
  model.zero_grad(set_to_none=True)
  x = pf.cuda().requires_grad_(True)
  cp = cam.cuda().requires_grad_(cam_grad)
  g = glo.cuda().requires_grad_(True)
  col = model(x, pos.cuda(), cp, g)
  loss = 0
  if dd is not None:
    loss = loss + (col.diffuse * dd.cuda()).sum()
  if ds is not None:
    loss = loss + (col.specular * ds.cuda()).sum()
  loss.backward()
  torch.cuda.synchronize()
  out = dict(diffuse=col.diffuse.detach(), specular=col.specular.detach(), point_features=x.grad, glo=g.grad,
             cam_pos=cp.grad if cam_grad else None)
  for k, p in model.named_parameters():
    out[k] = p.grad
  return out


def _reference(params, pf, pos, cam, glo, dd, ds, L, S, mode):
  """mode: 'fp64' (CPU), 'round16' (CPU fp64 with the kernels' operand rounding) or 'autocast' (the reference's path)."""
  if mode == "autocast":
    dev, dt = "cuda", torch.float32
  else:
    dev, dt = "cpu", torch.float64
  P = {k: v.detach().to(dev, dt).clone().requires_grad_(True) for k, v in params.items()}
  x = pf.to(dev, dt).requires_grad_(True)
  cp = cam.to(dev, dt).requires_grad_(True)
  g = glo.to(dev, dt).requires_grad_(True)
  if mode == "autocast":
    dif, spec = cmo.autocast_restatement(P, x, pos.to(dev, dt), cp, g, L, S)
  else:
    dif, spec = cmo.forward(P, x, pos.to(dev, dt), cp, g, L, S, round16=(mode == "round16"))
  loss = 0
  if dd is not None:
    loss = loss + (dif * dd.to(dev, dt)).sum()
  if ds is not None:
    loss = loss + (spec * ds.to(dev, dt)).sum()
  loss.backward()
  out = dict(diffuse=dif.detach(), specular=spec.detach(), point_features=x.grad, glo=g.grad, cam_pos=cp.grad)
  for k, p in P.items():
    out[k] = p.grad
  return out


def _err(a, b):
  """max |a - b| relative to max |b|"""
  a, b = a.detach().double().cpu(), b.detach().double().cpu()
  return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _params(model):
  return {k: v.detach() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 1000, 100_003])
def test_forward_matches_rounded_oracle(c, M):
  model = _model(c)
  pf, pos, cam, glo, *_ = _inputs(c, M)
  with torch.no_grad():
    col = model(pf.cuda(), pos.cuda(), cam.cuda(), glo.cuda())
  L, S = CONFIGS[c][3:]
  ref = cmo.forward({k: v.cpu().double() for k, v in _params(model).items()}, pf.double(), pos.double(), cam.double(),
                    glo.double(), L, S, round16=True)
  for name, a, b in (("diffuse", col.diffuse, ref[0]), ("specular", col.specular, ref[1])):
    d = (a.cpu().double() - b).abs()
    scale = b.abs().max().item()
    med, mx = d.median().item() / scale, d.max().item() / scale
    print(f"c{c} M={M} {name}: median {med:.2e} max {mx:.2e} of {scale:.3g}")
    assert med < 2e-6, (name, med)            # fp32 level: the same rounded operands, fp32 vs fp64 arithmetic
    assert mx < 8e-3, (name, mx)              # a hidden activation that rounds to the neighbouring f16: a few ulps


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("M", [1, 33, 1000, 100_003])
def test_forward_and_gradients_vs_fp64_and_autocast(c, M):
  model = _model(c)
  L, S = CONFIGS[c][3:]
  pf, pos, cam, glo, dd, ds = _inputs(c, M)
  nat = _native(model, pf, pos, cam, glo, dd, ds)
  params = _params(model)
  ref = _reference(params, pf, pos, cam, glo, dd, ds, L, S, "fp64")
  ac = _reference(params, pf, pos, cam, glo, dd, ds, L, S, "autocast")
  worst = []
  for k in ref:
    e_nat, e_ac = _err(nat[k], ref[k]), _err(ac[k], ref[k])
    worst.append((k, e_nat, e_ac))
    assert e_nat < 3e-2, (k, e_nat)                        # f16 level
    assert e_nat <= 1.5 * e_ac + 2e-4, (k, e_nat, e_ac)    # no worse than the reference's own fp16 path
  print(f"c{c} M={M}: " + ", ".join(f"{k.split('.')[-1] if '.' in k else k} {a:.1e}/{b:.1e}" for k, a, b in worst))


@pytest.mark.parametrize("c", [0, 1])
def test_golden_through_native(c):
  P, G, H, L, S = (int(v) for v in GOLDEN[f"c{c}_cfg"])
  model = ColorModel(ColorModelConfig(hidden_features=H, hidden_layers=L, sh_degree=S), glo_features=G,
                     point_features=P).cuda()
  sd = {k.split("::")[1]: torch.tensor(GOLDEN[k]).float() for k in GOLDEN.files if k.startswith(f"c{c}_param::")}
  model.load_state_dict(sd)
  t = lambda n: torch.tensor(GOLDEN[f"c{c}_{n}"]).float()
  nat = _native(model, t("point_features"), t("positions"), t("cam_pos"), t("glo"), t("d_diffuse"), t("d_specular"))
  assert _err(nat["diffuse"], torch.tensor(GOLDEN[f"c{c}_diffuse"])) < 1e-2
  assert _err(nat["specular"], torch.tensor(GOLDEN[f"c{c}_specular"])) < 1e-2
  for k in GOLDEN.files:
    if k.startswith(f"c{c}_grad::"):
      name = k.split("::")[1]
      e = _err(nat[name], torch.tensor(GOLDEN[k]))
      assert e < 3e-2, (name, e)


@pytest.mark.parametrize("side", ["diffuse", "specular", "both"])
def test_one_sided_upstream_gradients(side):
  c = 0
  model = _model(c)
  L, S = CONFIGS[c][3:]
  pf, pos, cam, glo, dd, ds = _inputs(c, 5000)
  dd = dd if side in ("diffuse", "both") else None
  ds = ds if side in ("specular", "both") else None
  nat = _native(model, pf, pos, cam, glo, dd, ds)
  ref = _reference(_params(model), pf, pos, cam, glo, dd, ds, L, S, "fp64")
  for k in ref:
    if ref[k] is None:
      assert nat[k] is None or nat[k].abs().max().item() == 0, k
      continue
    if ref[k].abs().max().item() == 0:
      assert nat[k].abs().max().item() == 0, k
      continue
    assert _err(nat[k], ref[k]) < 3e-2, (k, _err(nat[k], ref[k]))


def test_tiny_upstream_gradients_do_not_underflow():
  c = 0
  model = _model(c)
  pf, pos, cam, glo, dd, ds = _inputs(c, 20_000)
  L, S = CONFIGS[c][3:]
  a = _native(model, pf, pos, cam, glo, dd, ds)
  b = _native(model, pf, pos, cam, glo, dd * 1e-8, ds * 1e-8)
  ref = _reference(_params(model), pf, pos, cam, glo, dd * 1e-8, ds * 1e-8, L, S, "fp64")
  for k in a:
    if k in ("diffuse", "specular"):
      continue
    # 1e-8 is not a power of two, so the scaled gradients round to other f16 values: equal at f16 level, not bitwise
    e = _err(b[k] * 1e8, a[k])
    assert e < 5e-3, (k, e)
    assert _err(b[k], ref[k]) < 3e-2, (k, _err(b[k], ref[k]))


def test_camera_gradient_and_no_camera_work():
  c = 1
  model = _model(c)
  L, S = CONFIGS[c][3:]
  pf, pos, cam, glo, dd, ds = _inputs(c, 3000)
  nat = _native(model, pf, pos, cam, glo, dd, ds, cam_grad=True)
  ref = _reference(_params(model), pf, pos, cam, glo, dd, ds, L, S, "fp64")
  assert _err(nat["cam_pos"], ref["cam_pos"]) < 3e-2
  off = _native(model, pf, pos, cam, glo, dd, ds, cam_grad=False)
  assert off["cam_pos"] is None
  for k in off:                                            # the rest does not depend on the camera path
    if k != "cam_pos":
      assert torch.equal(off[k], nat[k]), k


def test_bit_reproducible():
  c = 0
  model = _model(c)
  args = _inputs(c, 70_001)
  a = _native(model, *args)
  b = _native(model, *args)
  for k in a:
    assert torch.equal(a[k], b[k]), k


def test_empty_rows():
  c = 0
  model = _model(c)
  pf, pos, cam, glo, dd, ds = _inputs(c, 0)
  nat = _native(model, pf, pos, cam, glo, dd, ds)
  assert nat["diffuse"].shape == (0, 3) and nat["specular"].shape == (0, 3)
  assert nat["point_features"].shape == (0, 16)
  for k, v in nat.items():
    if v is not None and v.numel():
      assert v.abs().max().item() == 0, k


def test_error_cases():
  model = _model(0)
  pf, pos, cam, glo, *_ = _inputs(0, 10)
  with pytest.raises(sta.GsplatHipError):
    model(pf, pos.cuda(), cam.cuda(), glo.cuda())
  with pytest.raises(sta.GsplatHipError):
    model.cpu()(pf, pos, cam, glo)
  model.cuda()
  with pytest.raises(ValueError):
    model(pf.cuda().double(), pos.cuda(), cam.cuda(), glo.cuda())
  with pytest.raises(ValueError):
    model(pf.cuda()[:, :8], pos.cuda(), cam.cuda(), glo.cuda())
  with pytest.raises(ValueError):
    model(pf.cuda(), pos.cuda(), cam.cuda(), glo.cuda()[:, :3])


def test_same_inside_autocast():
  c = 0
  model = _model(c)
  pf, pos, cam, glo, *_ = _inputs(c, 1000)
  with torch.no_grad():
    a = model(pf.cuda(), pos.cuda(), cam.cuda(), glo.cuda())
    with torch.autocast(device_type="cuda", dtype=torch.float16):
      b = model(pf.cuda(), pos.cuda(), cam.cuda(), glo.cuda())
  assert b.diffuse.dtype == torch.float32
  assert torch.equal(a.diffuse, b.diffuse) and torch.equal(a.specular, b.specular)


class _OracleColorModel(torch.nn.Module):
  """The flow's reference colour model: the fp32 torch restatement with the native model's parameters."""

  def __init__(self, native):
    super().__init__()
    self.params = {k: v.detach().clone().requires_grad_(True) for k, v in native.state_dict().items()}
    self.L, self.S = native.config.hidden_layers, native.config.sh_degree

  def __call__(self, pf, pos, cam, glo):
    d, s = cmo.forward(self.params, pf, pos, cam, glo, self.L, self.S)
    return sta.Colors(d, s)


def _flow(colour_model, g, cam, glo, pwf):
  """MLPScene.render + reg_loss: project -> colour the visible points -> render -> loss + specular term."""
  cfg = sta.RasterConfig(compute_visibility=True)
  g2d, depth, idx = sta.project_to_image(g, cam, cfg)
  colours = colour_model(pwf[idx], g.position[idx], cam.camera_position, glo)
  r = sta.render_projected(idx, g2d, colours.total(), depth, cam, cfg)
  points = r.points.replace(attributes=colours)
  loss = (r.image - 0.3).pow(2).mean() + 1e-2 * points.visible.attributes.specular.mean()
  loss.backward()
  torch.cuda.synchronize()


def test_dropin_render_flow():
  g, cam = synthetic.scene_a(3000, 160, 120, sh_degree=0, seed=3, sigma_px=2.5)
  native = _model(0)
  camc = cam.to("cuda")
  gen = torch.Generator().manual_seed(5)
  pf0 = torch.randn(g.position.shape[0], 16, generator=gen)
  glo0 = torch.randn(1, 32, generator=gen) * 0.5
  runs = []
  for model in (native, _OracleColorModel(native)):
    gd = sta.Gaussians3D(*(t.clone().cuda().requires_grad_(True) for t in
                           (g.position, g.rotation, g.log_scaling, g.alpha_logit, g.feature)))
    pf = pf0.cuda().requires_grad_(True)
    glo = glo0.cuda().requires_grad_(True)
    _flow(model, gd, camc, glo, pf)
    pgrads = ([p.grad for _, p in native.named_parameters()] if model is native else
              [model.params[k].grad for k, _ in native.named_parameters()])
    runs.append(dict(position=gd.position.grad, log_scaling=gd.log_scaling.grad, alpha_logit=gd.alpha_logit.grad,
                     point_features=pf.grad, glo=glo.grad, params=pgrads))
  a, b = runs
  for k in ("position", "log_scaling", "alpha_logit", "point_features", "glo"):
    e = _err(a[k], b[k])
    print(f"flow {k}: {e:.2e}")
    assert e < 5e-2, (k, e)
  for i, (x, y) in enumerate(zip(a["params"], b["params"])):
    assert _err(x, y) < 5e-2, (i, _err(x, y))


def test_short_fit_converges_like_torch():
  """Adam on the colour model's parameters towards fixed target colours: the native model's loss falls as the fp32
  torch restatement's does."""
  c = 0
  M = 4096
  pf, pos, cam, glo, *_ = _inputs(c, M, seed=7)
  target = torch.rand(M, 3, generator=torch.Generator().manual_seed(8)).cuda()
  losses = []
  for use_native in (True, False):
    model = _model(c, seed=11)
    params = list(model.parameters())
    oracle = _OracleColorModel(model)
    if not use_native:
      params = list(oracle.params.values())
    opt = torch.optim.Adam(params, lr=1e-2)
    for _ in range(300):
      opt.zero_grad()
      col = (model if use_native else oracle)(pf.cuda(), pos.cuda(), cam.cuda(), glo.cuda())
      loss = (col.total() - target).pow(2).mean()
      loss.backward()
      opt.step()
    losses.append(loss.item())
  first = _model(c, seed=11)(pf.cuda(), pos.cuda(), cam.cuda(), glo.cuda())
  start = (first.total() - target).pow(2).mean().item()
  print(f"fit: start {start:.4f} native {losses[0]:.4f} torch {losses[1]:.4f}")
  assert losses[0] < 0.5 * start
  assert losses[0] < 1.2 * losses[1] + 1e-3
