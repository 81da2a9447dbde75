"""The reference's neural colour model (``splat_trainer.scene.color_model``: ``ColorModelConfig``, ``Colors``,
``ColorModel``) on fused HIP kernels (csrc/color_model.hip).  Same constructor, submodule names and ``state_dict`` keys as
the reference, so a reference checkpoint's ``color_model`` entry loads as it is.

Per row: ``x = LayerNorm([point_features, glo])``; ``diffuse = lum(base_model(x))``; ``d = normalize(position -
cam_pos)``; ``[a, b] = encode_dir(rsh_S(d))``; ``specular = lum(directional_model.mlp(x a + b), -2)``.  Every Linear
rounds its input and weight to f16 once (round to nearest even) and adds its fp32 bias to fp32 products; everything else
is fp32 (DESIGN.md "Colour model").  Supported: ``hidden_features = 32``, ``hidden_layers`` 1 or 2, ``sh_degree`` 2..5,
``1 <= glo_features + point_features <= 64``, ``color_channels = 3``; anything else raises ValueError at construction.
Inputs are float32 tensors on the HIP device; a CPU tensor raises GsplatHipError (there is no CPU fallback).  Positions
get no gradient (the reference detaches them).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import _lib
from ._args import on_one_device, require
from ._lib import ptr as _ptr

SUPPORTED = "hidden_features = 32, hidden_layers in {1, 2}, sh_degree in 2..5, 1 <= glo_features + point_features <= 64, " \
            "color_channels = 3"


@dataclass
class ColorModelConfig:
  hidden_features: int = 32
  hidden_layers: int = 2
  sh_degree: int = 5
  lr_diffuse: float = 1e-3
  lr_specular: float = 1e-3
  color_channels: int = 3
  hdr: bool = False

  def create_model(self, glo_features: int, point_features: int) -> "ColorModel":
    return ColorModel(config=self, glo_features=glo_features, point_features=point_features)


class Colors:
  """``diffuse`` and ``specular`` (M, 3); ``total(w) = diffuse + w specular``.  Rows index like a tensor (an index, a
  slice, an index tensor or a mask), as ``RenderedPoints.visible`` does with its ``attributes``."""

  def __init__(self, diffuse: torch.Tensor, specular: torch.Tensor, batch_size=None):
    if diffuse.shape != specular.shape:
      raise ValueError(f"diffuse {tuple(diffuse.shape)} and specular {tuple(specular.shape)} differ")
    self.diffuse = diffuse
    self.specular = specular

  def total(self, specular_weight: float = 1.0) -> torch.Tensor:
    return self.diffuse + self.specular * specular_weight

  def __getitem__(self, idx) -> "Colors":
    return Colors(self.diffuse[idx], self.specular[idx])

  def __len__(self) -> int:
    return self.diffuse.shape[0]

  @property
  def batch_size(self) -> torch.Size:
    return self.diffuse.shape[:1]

  @property
  def shape(self) -> torch.Size:
    return self.batch_size

  def __repr__(self) -> str:
    return f"Colors(batch_size={tuple(self.batch_size)}, device={self.diffuse.device})"


class _GLULayer(nn.Module):
  def __init__(self, in_features: int, out_features: int):
    super().__init__()
    self.m = nn.Linear(in_features, out_features * 2)
    self.act = nn.GLU()

  def forward(self, x):
    return self.act(self.m(x))


class _MLP(nn.Module):
  def __init__(self, inputs: int, outputs: int, hidden: int, hidden_layers: int):
    super().__init__()
    sizes = [inputs] + [hidden] * hidden_layers
    self.layers = nn.ModuleList([_GLULayer(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1)])
    self.layers.append(nn.Linear(sizes[-1], outputs))


class _ProjectSH(nn.Module):
  def __init__(self, out_features: int, sh_degree: int, hidden: int):
    super().__init__()
    self.mlp = _MLP((sh_degree + 1) ** 2, out_features, hidden, 0)


class _AffineMLP(nn.Module):
  def __init__(self, inputs: int, outputs: int, hidden: int, hidden_layers: int, sh_degree: int):
    super().__init__()
    self.mlp = _MLP(inputs, outputs, hidden, hidden_layers)
    self.encode_dir = _ProjectSH(inputs * 2, sh_degree, hidden)


def _check_config(config: ColorModelConfig, glo_features: int, point_features: int):
  F = glo_features + point_features
  ok = (config.hidden_features == 32 and config.hidden_layers in (1, 2) and 2 <= config.sh_degree <= 5 and
        glo_features >= 0 and point_features >= 0 and 1 <= F <= 64 and config.color_channels == 3)
  if not ok:
    raise ValueError(f"unsupported colour model: hidden_features={config.hidden_features}, hidden_layers="
                     f"{config.hidden_layers}, sh_degree={config.sh_degree}, glo_features={glo_features}, point_features="
                     f"{point_features}, color_channels={config.color_channels}; supported: {SUPPORTED}")


class _ColorFn(torch.autograd.Function):
  @staticmethod
  def forward(ctx, model_c, L, pf, pos, cam, glo, *params):
    M = pos.shape[0]
    dev = pos.device
    with _lib.on_device(dev) as stream:
      diffuse = torch.empty((M, 3), dtype=torch.float32, device=dev)
      specular = torch.empty((M, 3), dtype=torch.float32, device=dev)
      ws = _lib.workspace(_lib.load().gsr_color_forward_workspace_bytes(C.byref(model_c)), dev)
      _lib.call("gsr_color_forward", C.byref(model_c), _ptr(pf), _ptr(pos), _ptr(cam), _ptr(glo), M, _ptr(diffuse),
                _ptr(specular), _ptr(ws), ws.numel(), stream)
    ctx.model_c = model_c
    ctx.L = L
    ctx.set_materialize_grads(False)         # an unused output's gradient arrives as None: that branch is skipped
    ctx.save_for_backward(pf, pos, cam, glo, *params)
    return diffuse, specular

  @staticmethod
  def backward(ctx, d_diffuse, d_specular):
    pf, pos, cam, glo, *params = ctx.saved_tensors
    M = pos.shape[0]
    dev = pos.device
    with _lib.on_device(dev) as stream:
      dd = None if d_diffuse is None else d_diffuse.float().contiguous()
      ds = None if d_specular is None else d_specular.float().contiguous()
      d_pf = torch.empty_like(pf)
      d_params = [torch.empty_like(p) for p in params]
      d_glo = torch.empty_like(glo)
      want_cam = ctx.needs_input_grad[4]
      d_cam = torch.empty_like(cam) if want_cam else None
      grads = _lib.GsrColorGrads()
      for i, layer in enumerate(_layer_slots(ctx.L)):
        grads.d_weight[layer] = d_params[2 * i].data_ptr()
        grads.d_bias[layer] = d_params[2 * i + 1].data_ptr()
      grads.d_glo = d_glo.data_ptr()
      grads.d_cam_pos = _ptr(d_cam)
      ws = _lib.workspace(_lib.load().gsr_color_backward_workspace_bytes(C.byref(ctx.model_c), M), dev)
      _lib.call("gsr_color_backward", C.byref(ctx.model_c), _ptr(pf), _ptr(pos), _ptr(cam), _ptr(glo), M, _ptr(dd), _ptr(ds),
                _ptr(d_pf), C.byref(grads), _ptr(ws), ws.numel(), stream)
    return (None, None, d_pf if ctx.needs_input_grad[2] else None, None, d_cam,
            d_glo if ctx.needs_input_grad[5] else None, *d_params)


def _layer_slots(L: int):
  """ABI parameter index of each Linear in ColorModel._linears() order."""
  return [0, 1, 2, 3, 4, 5, 6] if L == 2 else [0, 2, 3, 4, 6]


class ColorModel(nn.Module):
  def __init__(self, config: ColorModelConfig, glo_features: int = 16, point_features: int = 16):
    super().__init__()
    _check_config(config, glo_features, point_features)
    self.config = config
    self.glo_features = glo_features
    self.point_features = point_features
    self.feature_size = glo_features + point_features
    self.norm = nn.LayerNorm(self.feature_size, elementwise_affine=False)
    n_out = config.color_channels + 1
    self.directional_model = _AffineMLP(self.feature_size, n_out, config.hidden_features, config.hidden_layers,
                                        config.sh_degree)
    self.base_model = _MLP(self.feature_size, n_out, config.hidden_features, config.hidden_layers)

  def _linears(self):
    L = self.config.hidden_layers
    base = [self.base_model.layers[i].m for i in range(L)] + [self.base_model.layers[L]]
    dirm = [self.directional_model.mlp.layers[i].m for i in range(L)] + [self.directional_model.mlp.layers[L]]
    return base + [self.directional_model.encode_dir.mlp.layers[0]] + dirm

  def _check_inputs(self, point_features, positions, cam_pos, glo_feature):
    inputs = dict(point_features=point_features, positions=positions, cam_pos=cam_pos, glo_feature=glo_feature)
    for name, t in inputs.items():
      require(name, t, what="the colour model")             # (this module looks at the device before the dtype)
      require(name, t, dtype=torch.float32)
    M = positions.shape[0]
    if point_features.dim() != 2 or point_features.shape != (M, self.point_features):
      raise ValueError(f"point_features must be (M, {self.point_features}) with M = {M}, got {tuple(point_features.shape)}")
    if positions.dim() != 2 or positions.shape[1] != 3:
      raise ValueError(f"positions must be (M, 3), got {tuple(positions.shape)}")
    if cam_pos.numel() != 3:
      raise ValueError(f"cam_pos must hold 3 values, got {tuple(cam_pos.shape)}")
    if glo_feature.dim() != 2 or glo_feature.shape != (1, self.glo_features):
      raise ValueError(f"glo_feature must be (1, {self.glo_features}), got {tuple(glo_feature.shape)}")
    for i, p in enumerate(self.parameters()):
      inputs[f"parameter {i}"] = require("colour model parameters", p, dtype=torch.float32)
    on_one_device(inputs)

  def forward(self, point_features: torch.Tensor, positions: torch.Tensor, cam_pos: torch.Tensor,
              glo_feature: torch.Tensor) -> Colors:
    self._check_inputs(point_features, positions, cam_pos, glo_feature)
    params = []
    for lin in self._linears():
      params += [lin.weight, lin.bias]
    model_c = _lib.GsrColorModel()
    model_c.P, model_c.G = self.point_features, self.glo_features
    model_c.H, model_c.L, model_c.S = self.config.hidden_features, self.config.hidden_layers, self.config.sh_degree
    model_c.color_channels = self.config.color_channels
    contiguous = [p if p.is_contiguous() else p.contiguous() for p in params]
    for i, layer in enumerate(_layer_slots(self.config.hidden_layers)):
      model_c.weight[layer] = contiguous[2 * i].data_ptr()
      model_c.bias[layer] = contiguous[2 * i + 1].data_ptr()
    with torch.autocast(device_type="cuda", enabled=False):
      diffuse, specular = _ColorFn.apply(model_c, self.config.hidden_layers, point_features.contiguous(),
                                         positions.detach().contiguous(), cam_pos.reshape(3).contiguous(),
                                         glo_feature.contiguous(), *contiguous)
    return Colors(diffuse, specular)

  def post_activation(self, image: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    if not self.config.hdr:
      return image[..., :3].clamp(0, 1)
    return image

  def optimizer(self, t: float = 0.) -> torch.optim.Optimizer:
    """The reference's two Adam groups, ``spec`` (directional model) and ``base`` (base model and norm), at lr 0: the
    learning-rate schedules (``Varying``) stay with the caller."""
    groups = [dict(params=list(self.directional_model.parameters()), lr=0.0, name="spec"),
              dict(params=[*self.base_model.parameters(), *self.norm.parameters()], lr=0.0, name="base")]
    return torch.optim.Adam(groups, betas=(0.9, 0.999))
