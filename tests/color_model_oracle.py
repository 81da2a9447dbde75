"""fp64 restatement of the reference's ColorModel forward (scene/color_model.py, scene/mlp/torch_mlp.py) on torch CPU or
GPU tensors, differentiable by autograd.  Parameters come as a dict in the reference's state_dict key names.

round16=True mirrors the kernels' numerics contract (DESIGN.md "Colour model"): the input activation and the weight of
every Linear are rounded once to f16 (round to nearest even) before an exact product; everything else stays fp64.
autocast_restatement() is the reference's own path, the torch modules under fp16 autocast.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

SH_K = [[math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m)) * (math.sqrt(2) if m else 1)
         for m in range(l + 1)] for l in range(6)]


def rsh(d: torch.Tensor, degree: int) -> torch.Tensor:
  """Real SH up to `degree`, index l(l+1)+m, Condon-Shortley phase, (M, (degree+1)^2): associated Legendre recurrence in z
  times Re/Im (x + iy)^m."""
  x, y, z = d[:, 0], d[:, 1], d[:, 2]
  out = [None] * ((degree + 1) ** 2)
  Cm, Sm = torch.ones_like(x), torch.zeros_like(x)
  for m in range(degree + 1):
    if m > 0:
      Cm, Sm = Cm * x - Sm * y, Sm * x + Cm * y
    qmm = (-1) ** m * math.prod(range(1, 2 * m, 2))
    q2, q1 = None, None
    for l in range(m, degree + 1):
      if l == m:
        q = torch.full_like(z, float(qmm))
      elif l == m + 1:
        q = (2 * m + 1) * z * q1
      else:
        q = ((2 * l - 1) * z * q1 - (l + m - 1) * q2) / (l - m)
      q2, q1 = q1, q
      k = SH_K[l][m]
      if m == 0:
        out[l * (l + 1)] = k * q
      else:
        out[l * (l + 1) + m] = k * q * Cm
        out[l * (l + 1) - m] = k * q * Sm
  return torch.stack(out, 1)


def _r16(t: torch.Tensor, on: bool) -> torch.Tensor:
  return t.to(torch.float16).to(t.dtype) if on else t


def linear(x, w, b, round16):
  # rounding of a value that needs a gradient: straight-through (the f16 rounding is not differentiated)
  xr = x + (_r16(x.detach(), round16) - x.detach())
  wr = w + (_r16(w.detach(), round16) - w.detach())
  return xr @ wr.t() + b


def mlp(x, params, prefix, L, round16):
  for i in range(L):
    y = linear(x, params[f"{prefix}.layers.{i}.m.weight"], params[f"{prefix}.layers.{i}.m.bias"], round16)
    a, g = y.chunk(2, dim=1)
    x = a * torch.sigmoid(g)
  return linear(x, params[f"{prefix}.layers.{L}.weight"], params[f"{prefix}.layers.{L}.bias"], round16)


def lum(o, bias=0.0):
  return torch.sigmoid(o[:, 1:]) * torch.exp(o[:, 0:1] + bias)


def forward(params, point_features, positions, cam_pos, glo_feature, L, S, round16=False):
  """(diffuse, specular), both (M, 3), in the dtype of the inputs."""
  M = positions.shape[0]
  feat = torch.cat([point_features, glo_feature.expand(M, glo_feature.shape[1])], 1)
  x = F.layer_norm(feat, (feat.shape[1],), eps=1e-5)
  diffuse = lum(mlp(x, params, "base_model", L, round16))
  d = F.normalize(positions.detach() - cam_pos.reshape(1, 3), dim=1)
  e = linear(rsh(d, S), params["directional_model.encode_dir.mlp.layers.0.weight"],
             params["directional_model.encode_dir.mlp.layers.0.bias"], round16)
  a, b = e.chunk(2, dim=1)
  specular = lum(mlp(x * a + b, params, "directional_model.mlp", L, round16), -2.0)
  return diffuse, specular


def param_keys(L: int):
  keys = []
  for prefix in ("base_model", "directional_model.mlp"):
    for i in range(L):
      keys += [f"{prefix}.layers.{i}.m.weight", f"{prefix}.layers.{i}.m.bias"]
    keys += [f"{prefix}.layers.{L}.weight", f"{prefix}.layers.{L}.bias"]
  keys += ["directional_model.encode_dir.mlp.layers.0.weight", "directional_model.encode_dir.mlp.layers.0.bias"]
  return keys


def autocast_restatement(params, point_features, positions, cam_pos, glo_feature, L, S):
  """The reference's call form on the GPU: fp32 inputs and parameters, the forward under fp16 autocast (LayerNorm and the
  SH basis in fp32, the Linears in f16, the activations on f16 outputs).  Returns fp32 (diffuse, specular)."""
  with torch.autocast(device_type="cuda", dtype=torch.float16):
    M = positions.shape[0]
    feat = torch.cat([point_features, glo_feature.expand(M, glo_feature.shape[1])], 1)
    x = F.layer_norm(feat, (feat.shape[1],), eps=1e-5)

    def amlp(x, prefix):
      for i in range(L):
        y = F.linear(x, params[f"{prefix}.layers.{i}.m.weight"], params[f"{prefix}.layers.{i}.m.bias"])
        x = F.glu(y, dim=-1)
      return F.linear(x, params[f"{prefix}.layers.{L}.weight"], params[f"{prefix}.layers.{L}.bias"])

    diffuse = lum(amlp(x, "base_model"))
    d = F.normalize(positions.detach() - cam_pos.reshape(1, 3), dim=1)
    e = F.linear(rsh(d, S).to(d.dtype), params["directional_model.encode_dir.mlp.layers.0.weight"],
                 params["directional_model.encode_dir.mlp.layers.0.bias"])
    a, b = torch.split(e, e.shape[1] // 2, dim=1)
    specular = lum(amlp(x * a + b, "directional_model.mlp"), -2.0)
  return diffuse.float(), specular.float()
