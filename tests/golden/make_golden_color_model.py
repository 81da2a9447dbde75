"""Writes tests/golden/color_model_ref.npz from the reference's own modules (splat-trainer checkout given by --reference):
scene/mlp/rsh.py and scene/mlp/torch_mlp.py are loaded by file path (scene/color_model.py itself imports omegaconf, so
the ColorModel is rebuilt from the loaded MLP / AffineMLP exactly as ColorModel.__init__ / forward do).  Only the .npz is
kept in this repository.

    python tests/golden/make_golden_color_model.py --reference /path/to/splat-trainer

Contents: ``dirs`` / ``rsh_cart_5`` on fixed directions; for each config c in {0: the shipped scene/mlp.yaml (P 16, G 32,
H 32, L 1, S 5), 1: L 2, S 3}: ``c{c}_cfg`` = (P, G, H, L, S), ``c{c}_param::<state_dict key>`` (seeded), fp64 inputs
``c{c}_point_features``, ``c{c}_positions``, ``c{c}_cam_pos``, ``c{c}_glo``, outputs ``c{c}_diffuse``, ``c{c}_specular``,
fixed upstream gradients ``c{c}_d_diffuse``, ``c{c}_d_specular`` and the fp64 gradients ``c{c}_grad::<name>`` of
sum(d_diffuse diffuse) + sum(d_specular specular) for every parameter, point_features, cam_pos and glo.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "color_model_ref.npz")
CONFIGS = [(16, 32, 32, 1, 5), (16, 32, 32, 2, 3)]
M = 257


def load_reference(root):
  beartype = types.ModuleType("beartype")
  beartype.beartype = lambda f: f
  sys.modules["beartype"] = beartype
  for name in ("splat_trainer", "splat_trainer.scene", "splat_trainer.scene.mlp"):
    pkg = types.ModuleType(name)
    pkg.__path__ = []
    sys.modules[name] = pkg
  mods = {}
  for name in ("rsh", "torch_mlp"):
    full = f"splat_trainer.scene.mlp.{name}"
    spec = importlib.util.spec_from_file_location(full, os.path.join(root, "splat_trainer", "scene", "mlp", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[full] = mod
    setattr(sys.modules["splat_trainer.scene.mlp"], name, mod)
    spec.loader.exec_module(mod)
    mods[name] = mod
  return mods["rsh"], mods["torch_mlp"]


class RefColorModel(nn.Module):
  """ColorModel.__init__ / forward of scene/color_model.py with the loaded MLP and AffineMLP."""

  def __init__(self, tm, P, G, H, L, S):
    super().__init__()
    Fs = P + G
    self.norm = nn.LayerNorm(Fs, elementwise_affine=False)
    self.directional_model = tm.AffineMLP(inputs=Fs, outputs=4, hidden_layers=L, hidden=H, proj_hidden_layers=0,
                                          sh_degree=S)
    self.base_model = tm.MLP(inputs=Fs, outputs=4, hidden=H, hidden_layers=L)

  def forward(self, point_features, positions, cam_pos, glo_feature):
    glo = glo_feature.expand(positions.shape[0], glo_feature.shape[1])
    feature = self.norm(torch.cat([point_features, glo], dim=1))

    def lum(o, bias=0.0):
      return o[:, 1:].sigmoid() * (o[:, 0:1] + bias).exp()

    diffuse = lum(self.base_model(feature))
    d = F.normalize(positions.detach() - cam_pos.unsqueeze(0), dim=1)
    specular = lum(self.directional_model(d, feature), -2.0)
    return diffuse, specular


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reference", required=True, help="root of a splat-trainer checkout")
  args = ap.parse_args()
  rsh, tm = load_reference(args.reference)
  out = {}
  g = torch.Generator().manual_seed(0)
  dirs = F.normalize(torch.randn(64, 3, generator=g, dtype=torch.float64), dim=1)
  dirs = torch.cat([dirs, torch.eye(3, dtype=torch.float64), -torch.eye(3, dtype=torch.float64)])
  out["dirs"] = dirs.numpy()
  out["rsh_cart_5"] = rsh.rsh_cart_5(dirs).numpy()
  for c, (P, G, H, L, S) in enumerate(CONFIGS):
    torch.manual_seed(100 + c)
    model = RefColorModel(tm, P, G, H, L, S).double()
    with torch.no_grad():                      # biases away from nn.Linear's small default, so every path matters
      for k, p in model.named_parameters():
        if k.endswith("bias"):
          p.uniform_(-0.5, 0.5)
    gi = torch.Generator().manual_seed(200 + c)
    pf = torch.randn(M, P, generator=gi, dtype=torch.float64).requires_grad_(True)
    pos = torch.randn(M, 3, generator=gi, dtype=torch.float64) * 2
    cam = torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64).requires_grad_(True)
    glo = (torch.randn(1, G, generator=gi, dtype=torch.float64) * 0.5).requires_grad_(True)
    diffuse, specular = model(pf, pos, cam, glo)
    dd = torch.randn(M, 3, generator=gi, dtype=torch.float64)
    ds = torch.randn(M, 3, generator=gi, dtype=torch.float64)
    ((diffuse * dd).sum() + (specular * ds).sum()).backward()
    out[f"c{c}_cfg"] = np.array([P, G, H, L, S])
    for k, p in model.state_dict().items():
      out[f"c{c}_param::{k}"] = p.numpy()
    for k, p in model.named_parameters():
      out[f"c{c}_grad::{k}"] = p.grad.numpy()
    for name, t in (("point_features", pf), ("positions", pos), ("cam_pos", cam), ("glo", glo)):
      out[f"c{c}_{name}"] = t.detach().numpy()
    out[f"c{c}_grad::point_features"] = pf.grad.numpy()
    out[f"c{c}_grad::cam_pos"] = cam.grad.numpy()
    out[f"c{c}_grad::glo"] = glo.grad.numpy()
    out[f"c{c}_diffuse"] = diffuse.detach().numpy()
    out[f"c{c}_specular"] = specular.detach().numpy()
    out[f"c{c}_d_diffuse"] = dd.numpy()
    out[f"c{c}_d_specular"] = ds.numpy()
  np.savez_compressed(OUT, **out)
  print(f"wrote {OUT}: {len(out)} arrays")


if __name__ == "__main__":
  main()
