"""CPU checks of the neural colour model: the fp64 oracle (tests/color_model_oracle.py) reproduces the golden data made
from the reference's own modules, ColorModel's state_dict matches the reference's keys and shapes, the shared row maths
(csrc/gsr_color.h through the host shim) match the oracle, and unsupported configurations raise the documented
ValueError."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import color_model_oracle as cmo
import hostmath
from splat_trainer_amd.color_model import SUPPORTED, ColorModel, ColorModelConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "color_model_ref.npz"))


@pytest.mark.parametrize("c", [0, 1])
def test_oracle_reproduces_golden(c):
  P, G, H, L, S = (int(v) for v in GOLDEN[f"c{c}_cfg"])
  params = {k.split("::")[1]: torch.tensor(GOLDEN[k]).requires_grad_(True) for k in GOLDEN.files
            if k.startswith(f"c{c}_param::")}
  t = lambda n: torch.tensor(GOLDEN[f"c{c}_{n}"])
  pf, cam, glo = t("point_features").requires_grad_(True), t("cam_pos").requires_grad_(True), t("glo").requires_grad_(True)
  dif, spec = cmo.forward(params, pf, t("positions"), cam, glo, L, S)
  assert torch.allclose(dif, t("diffuse"), rtol=0, atol=1e-12)
  assert torch.allclose(spec, t("specular"), rtol=0, atol=1e-12)
  ((dif * t("d_diffuse")).sum() + (spec * t("d_specular")).sum()).backward()
  grads = dict(point_features=pf.grad, cam_pos=cam.grad, glo=glo.grad, **{k: p.grad for k, p in params.items()})
  for k in GOLDEN.files:
    if k.startswith(f"c{c}_grad::"):
      name = k.split("::")[1]
      ref = torch.tensor(GOLDEN[k])
      assert (grads[name] - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item()), name


@pytest.mark.parametrize("c", [0, 1])
def test_state_dict_matches_reference_keys(c):
  P, G, H, L, S = (int(v) for v in GOLDEN[f"c{c}_cfg"])
  m = ColorModel(ColorModelConfig(hidden_features=H, hidden_layers=L, sh_degree=S), glo_features=G, point_features=P)
  ours = {k: tuple(v.shape) for k, v in m.state_dict().items()}
  ref = {k.split("::")[1]: GOLDEN[k].shape for k in GOLDEN.files if k.startswith(f"c{c}_param::")}
  assert ours == ref
  sd = {k: torch.tensor(GOLDEN[f"c{c}_param::{k}"]).float() for k in ref}
  m.load_state_dict(sd)
  assert sorted(cmo.param_keys(L)) == sorted(ref)


def test_shipped_config_parameter_count():
  m = ColorModelConfig(hidden_features=32, hidden_layers=1, sh_degree=5).create_model(glo_features=32, point_features=16)
  assert sum(p.numel() for p in m.parameters()) == 10088


def test_shim_sh_basis_matches_golden(built_libs):
  lib = hostmath.load(built_libs)
  d = np.ascontiguousarray(GOLDEN["dirs"], dtype=np.float32)
  out = np.zeros((len(d), 36), np.float32)
  assert lib.hm_cm_rsh(5, d, len(d), out, None, None) == 0
  ref = GOLDEN["rsh_cart_5"]
  assert np.abs(out - ref).max() < 4e-6 * np.abs(ref).max()
  for S in range(6):          # lower degrees are the leading columns
    o = np.zeros((len(d), (S + 1) ** 2), np.float32)
    lib.hm_cm_rsh(S, d, len(d), o, None, None)
    assert np.abs(o - ref[:, :(S + 1) ** 2]).max() < 4e-6 * np.abs(ref).max()


def test_shim_row_maths_match_oracle(built_libs):
  lib = hostmath.load(built_libs)
  rng = np.random.default_rng(0)
  n = 200
  # SH vector-Jacobian product (also at d = 0, a point at the camera)
  for S in (2, 3, 4, 5):
    K = (S + 1) ** 2
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d[0] = 0
    dsh = rng.standard_normal((n, K)).astype(np.float32)
    dd = np.zeros((n, 3), np.float32)
    lib.hm_cm_rsh(S, d, n, None, dsh, dd)
    dt = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    (cmo.rsh(dt, S) * torch.tensor(dsh, dtype=torch.float64)).sum().backward()
    assert np.abs(dd - dt.grad.numpy()).max() < 1e-5 * np.abs(dt.grad.numpy()).max()
  # LayerNorm
  F_ = 48
  u = rng.standard_normal((n, F_)).astype(np.float32)
  dy = rng.standard_normal((n, F_)).astype(np.float32)
  y, du = np.zeros_like(u), np.zeros_like(u)
  lib.hm_cm_layernorm(u, n, F_, dy, y, du)
  ut = torch.tensor(u, dtype=torch.float64, requires_grad=True)
  yt = F.layer_norm(ut, (F_,), eps=1e-5)
  (yt * torch.tensor(dy, dtype=torch.float64)).sum().backward()
  assert np.abs(y - yt.detach().numpy()).max() < 1e-5 and np.abs(du - ut.grad.numpy()).max() < 1e-5
  # GLU
  a, b, dh = (rng.standard_normal(n).astype(np.float32) * 3 for _ in range(3))
  h, da, db = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
  lib.hm_cm_glu(a, b, dh, n, h, da, db)
  at, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (a, b))
  ht = F.glu(torch.cat([at[:, None], bt[:, None]], 1), dim=1)[:, 0]
  (ht * torch.tensor(dh, dtype=torch.float64)).sum().backward()
  assert np.abs(h - ht.detach().numpy()).max() < 1e-5 and np.abs(da - at.grad.numpy()).max() < 1e-5
  assert np.abs(db - bt.grad.numpy()).max() < 1e-5
  # luminance activation, both intensity biases
  for bias in (0.0, -2.0):
    o = rng.standard_normal((n, 4)).astype(np.float32)
    dout = rng.standard_normal((n, 3)).astype(np.float32)
    out, do = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32)
    lib.hm_cm_lum(o, n, bias, dout, out, do)
    ot = torch.tensor(o, dtype=torch.float64, requires_grad=True)
    lt = cmo.lum(ot, bias)
    (lt * torch.tensor(dout, dtype=torch.float64)).sum().backward()
    assert np.abs(out - lt.detach().numpy()).max() < 1e-5 * np.abs(out).max()
    assert np.abs(do - ot.grad.numpy()).max() < 1e-5 * np.abs(do).max()
  # F.normalize, including a zero vector (eps branch)
  v = rng.standard_normal((n, 3)).astype(np.float32)
  v[0] = 0
  ddv = rng.standard_normal((n, 3)).astype(np.float32)
  dn, dv = np.zeros_like(v), np.zeros_like(v)
  lib.hm_cm_normalize(v, ddv, n, dn, dv)
  vt = torch.tensor(v, dtype=torch.float64, requires_grad=True)
  nt = F.normalize(vt, dim=1)
  (nt * torch.tensor(ddv, dtype=torch.float64)).sum().backward()
  assert np.abs(dn - nt.detach().numpy()).max() < 1e-6
  assert np.allclose(dv[1:], vt.grad.numpy()[1:], rtol=1e-4, atol=1e-5)
  assert np.allclose(dv[0], vt.grad.numpy()[0], rtol=1e-5)


@pytest.mark.parametrize("kw,gf,pf", [(dict(hidden_features=64), 32, 16), (dict(hidden_layers=3), 32, 16),
                                      (dict(hidden_layers=0), 32, 16), (dict(sh_degree=6), 32, 16),
                                      (dict(sh_degree=1), 32, 16), (dict(color_channels=4), 32, 16), ({}, 48, 17),
                                      ({}, 0, 0)])
def test_unsupported_config_raises(kw, gf, pf):
  with pytest.raises(ValueError, match="supported: hidden_features = 32"):
    ColorModel(ColorModelConfig(**kw), glo_features=gf, point_features=pf)
  assert "sh_degree in 2..5" in SUPPORTED


@pytest.mark.parametrize("gf,pf,L", [(32, 16, 1), (16, 16, 2), (8, 8, 2), (0, 1, 1), (64, 0, 2)])
def test_supported_configs_construct(gf, pf, L):
  ColorModel(ColorModelConfig(hidden_layers=L), glo_features=gf, point_features=pf)
