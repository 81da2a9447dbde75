"""fp64 restatement of the reference's ColorModel forward (scene/color_model.py, scene/mlp/torch_mlp.py) on torch CPU or
GPU tensors, differentiable by autograd.  Parameters come as a dict in the reference's state_dict key names.

round16=True mirrors the kernels' numerics contract (DESIGN.md "Colour model"): the input activation and the weight of
every Linear are rounded once to f16 (round to nearest even) before an exact product; everything else stays fp64.
autocast_restatement() is the reference's own path, the torch modules under fp16 autocast.

backward() is the hand-written backward of the same model (no autograd).  With round16=True it restates the backward
kernel's contract (csrc/color_model.hip: cm_mlp_bwd, cm_dw, cm_dx, cm_scale_for, cm_backward_kernel): rows in
consecutive tiles of 16, and per tile and Linear the upstream dy enters as f16(dy 2^k) / 2^k with k = 15 - exponent of
the tile's largest |dy|; dx = dyq W16, dW = dyq^T in16 and d_bias = sum dyq use that one quantised dy, the f16 weight and
the f16 layer input; everything else is unrounded.  With round16=False it is the exact backward.
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


# ---- the hand-written backward ------------------------------------------------------------------------------------

TILE_ROWS = 16           # rows of one wave: the unit of the dy scale
SCALE_TOP = 15           # the tile's largest |dy| 2^k lies in [2^14, 2^15)
SCALE_CLAMP = 120
NORM_EPS = 1e-12         # F.normalize
LN_EPS = 1e-5
# Deliberately wrong variants of the contract, for the sensitivity test only (tests/test_color_model_contract_host.py)
PERTURBATIONS = ("scale64", "no_dy_rounding", "pad_leak", "dw_col_leak", "bias_drop_tail")


class _Dual:
  """Value (M,) and gradient (M, 3) with respect to the direction: forward-mode derivative of the SH polynomials, as
  GsrDual3 in csrc/gsr_color.h."""

  def __init__(self, v, g):
    self.v, self.g = v, g

  def __add__(self, o):
    return _Dual(self.v + o.v, self.g + o.g)

  def __sub__(self, o):
    return _Dual(self.v - o.v, self.g - o.g)

  def __mul__(self, o):
    if isinstance(o, _Dual):
      return _Dual(self.v * o.v, self.g * o.v[:, None] + self.v[:, None] * o.g)
    return _Dual(self.v * o, self.g * o)

  __rmul__ = __mul__


def rsh_jet(d: torch.Tensor, degree: int):
  """rsh(d, degree) (M, K) and its Jacobian dY_c / dd (M, K, 3), by dual numbers over the recurrence of rsh()."""
  M = d.shape[0]
  unit = torch.eye(3, dtype=d.dtype, device=d.device)
  x, y, z = (_Dual(d[:, k], unit[k].expand(M, 3)) for k in range(3))
  const = lambda c: _Dual(torch.full_like(d[:, 0], float(c)), torch.zeros_like(d))
  out = [None] * ((degree + 1) ** 2)
  Cm, Sm = const(1), const(0)
  for m in range(degree + 1):
    if m > 0:
      Cm, Sm = Cm * x - Sm * y, Sm * x + Cm * y
    qmm = (-1) ** m * math.prod(range(1, 2 * m, 2))
    q2, q1 = None, None
    for l in range(m, degree + 1):
      if l == m:
        q = const(qmm)
      elif l == m + 1:
        q = (2 * m + 1) * (z * q1)
      else:
        q = (1.0 / (l - m)) * ((2 * l - 1) * (z * q1) - (l + m - 1) * q2)
      q2, q1 = q1, q
      k = SH_K[l][m]
      if m == 0:
        out[l * (l + 1)] = k * q
      else:
        out[l * (l + 1) + m] = k * (q * Cm)
        out[l * (l + 1) - m] = k * (q * Sm)
  return torch.stack([o.v for o in out], 1), torch.stack([o.g for o in out], 1)


def dy_scale(dy: torch.Tensor, tile_rows: int = TILE_ROWS) -> torch.Tensor:
  """cm_scale_for per tile of `tile_rows` consecutive rows, over every column of dy: (M, 1) powers of two.  Rows past M
  count as zero; a zero or non-finite maximum gives 1."""
  M = dy.shape[0]
  tiles = (M + tile_rows - 1) // tile_rows
  amax = dy.abs().amax(1) if dy.shape[1] else dy.new_zeros(M)
  amax = torch.cat([amax, amax.new_zeros(tiles * tile_rows - M)]).reshape(tiles, tile_rows).amax(1)
  ok = (amax > 0) & torch.isfinite(amax)
  _, e = torch.frexp(torch.where(ok, amax, torch.ones_like(amax)))      # amax = m 2^e, m in [0.5, 1)
  k = (SCALE_TOP - e).clamp(-SCALE_CLAMP, SCALE_CLAMP)
  scale = torch.where(ok, torch.ldexp(torch.ones_like(amax), k), torch.ones_like(amax))
  return scale.repeat_interleave(tile_rows)[:M, None]


class _Contract:
  """How dy enters the three products of a Linear's backward."""

  def __init__(self, round16: bool, perturb=()):
    unknown = set(perturb) - set(PERTURBATIONS)
    if unknown:
      raise ValueError(f"unknown perturbations {sorted(unknown)}")
    self.round16 = round16
    self.perturb = frozenset(perturb)

  def quantise(self, dy):
    if not self.round16:
      return dy
    s = dy_scale(dy, 64 if "scale64" in self.perturb else TILE_ROWS)
    scaled = dy * s                                   # exact: a power of two
    if "no_dy_rounding" not in self.perturb:
      scaled = _r16(scaled, True)
    return scaled / s                                 # exact

  def bias_sum(self, dyq):
    if "bias_drop_tail" in self.perturb:
      dyq = dyq[:dyq.shape[0] // TILE_ROWS * TILE_ROWS]
    return dyq.sum(0)

  def linear_bwd(self, dy, x_in, w, grads, wkey, bkey, want_dx=True):
    """dW = dyq^T in16 and d_bias = sum dyq into grads; returns dx = dyq W16 (or None)."""
    dyq = self.quantise(dy)
    in16 = _r16(x_in, self.round16)
    grads[wkey] = dyq.t() @ in16
    if "dw_col_leak" in self.perturb and wkey.endswith("layers.0.m.weight"):
      grads[wkey][:, -1] += dyq[:TILE_ROWS].t() @ in16[:TILE_ROWS, 0]
    grads[bkey] = self.bias_sum(dyq)
    return dyq @ _r16(w, self.round16) if want_dx else None


def _linear_fwd(x, w, b, round16):
  return _r16(x, round16) @ _r16(w, round16).t() + b


def _mlp_fwd(x, params, prefix, L, round16):
  """The output and what the backward recomputes: every Linear's input and every GLU's pre-activation."""
  ins, ys = [], []
  for i in range(L):
    ins.append(x)
    y = _linear_fwd(x, params[f"{prefix}.layers.{i}.m.weight"], params[f"{prefix}.layers.{i}.m.bias"], round16)
    ys.append(y)
    a, g = y.chunk(2, dim=1)
    x = a * torch.sigmoid(g)
  ins.append(x)
  return _linear_fwd(x, params[f"{prefix}.layers.{L}.weight"], params[f"{prefix}.layers.{L}.bias"], round16), ins, ys


def _lum_bwd(o, bias, dout):
  e = torch.exp(o[:, 0:1] + bias)
  s = torch.sigmoid(o[:, 1:])
  return torch.cat([(dout * s * e).sum(1, keepdim=True), dout * e * s * (1 - s)], 1)


def _mlp_bwd(ct, params, prefix, L, ins, ys, d_o, grads):
  dh = ct.linear_bwd(d_o, ins[L], params[f"{prefix}.layers.{L}.weight"], grads, f"{prefix}.layers.{L}.weight",
                     f"{prefix}.layers.{L}.bias")
  for i in reversed(range(L)):
    a, g = ys[i].chunk(2, dim=1)
    s = torch.sigmoid(g)
    dy = torch.cat([dh * s, dh * a * s * (1 - s)], 1)
    dh = ct.linear_bwd(dy, ins[i], params[f"{prefix}.layers.{i}.m.weight"], grads, f"{prefix}.layers.{i}.m.weight",
                       f"{prefix}.layers.{i}.m.bias")
  return dh


def backward(params, point_features, positions, cam_pos, glo_feature, L, S, d_diffuse, d_specular, round16=False,
             perturb=()):
  """Gradients of sum(diffuse d_diffuse) + sum(specular d_specular), either upstream may be None: a dict with
  "point_features", "glo", "cam_pos" and every parameter under its state_dict key, in the dtype of the inputs.  A branch
  without an upstream gradient contributes exact zeros.  `perturb` is for the sensitivity test only."""
  ct = _Contract(round16, perturb)
  M, P = point_features.shape
  G = glo_feature.shape[1]
  Fn = P + G
  enc_w, enc_b = "directional_model.encode_dir.mlp.layers.0.weight", "directional_model.encode_dir.mlp.layers.0.bias"
  grads = {k: torch.zeros_like(params[k]) for k in param_keys(L)}
  grads["cam_pos"] = torch.zeros_like(cam_pos)

  # forward, recomputed
  feat = torch.cat([point_features, glo_feature.expand(M, G)], 1)
  dev = feat - feat.mean(1, keepdim=True)
  rstd = 1 / torch.sqrt((dev * dev).mean(1, keepdim=True) + LN_EPS)
  x = dev * rstd
  dx = torch.zeros_like(x)

  if d_diffuse is not None:
    o, ins, ys = _mlp_fwd(x, params, "base_model", L, round16)
    dx = dx + _mlp_bwd(ct, params, "base_model", L, ins, ys, _lum_bwd(o, 0.0, d_diffuse), grads)

  if d_specular is not None:
    v = positions - cam_pos.reshape(1, 3)
    n = v.norm(dim=1, keepdim=True)
    clamped = ~(n > NORM_EPS)
    den = torch.where(clamped, torch.full_like(n, NORM_EPS), n)
    d = v / den
    sh, jac = rsh_jet(d, S)
    e = _linear_fwd(sh, params[enc_w], params[enc_b], round16)
    a, b = e[:, :Fn], e[:, Fn:]
    z = x * a + b
    q, ins, ys = _mlp_fwd(z, params, "directional_model.mlp", L, round16)
    dz = _mlp_bwd(ct, params, "directional_model.mlp", L, ins, ys, _lum_bwd(q, -2.0, d_specular), grads)
    dx = dx + dz * a
    dsh = ct.linear_bwd(torch.cat([dz * x, dz], 1), sh, params[enc_w], grads, enc_w, enc_b)
    dd = (dsh[:, :, None] * jac).sum(1)
    dot = torch.where(clamped, torch.zeros_like(n), (d * dd).sum(1, keepdim=True))
    grads["cam_pos"] = -((dd - d * dot) / den).sum(0).reshape(cam_pos.shape)

  # LayerNorm
  s1 = dx.sum(1, keepdim=True)
  s2 = (dx * x).sum(1, keepdim=True)
  # pad_leak is a proxy: it does not build the padded operand, it lets a slot past F that is not zero join the LayerNorm
  # row sums, with the last real column's content.  dw_col_leak is the weight-gradient side of the same mistake: in
  # _Contract.linear_bwd the last real input column of both first-layer dW also receives the first 16-row tile's product
  # with input column 0, as one dW tile accumulated one slot off would.
  if "pad_leak" in ct.perturb:
    s1 = s1 + dx[:, -1:]
    s2 = s2 + dx[:, -1:] * x[:, -1:]
  du = rstd * (dx - s1 / Fn - x * (s2 / Fn))
  grads["point_features"] = du[:, :P]
  grads["glo"] = du[:, P:].sum(0, keepdim=True)
  return grads
