"""Cases, figures and bounds of the sparse optimizer step's one-step contract, shared by
tests/test_optim_contract_host.py (CPU: the noise table, the oracle's terms, planted deviations of the model) and
tests/test_gpu_optim_contract.py (csrc/optim.hip through ParameterClass.step against oracle/optim_oracle.py in fp64).

A case is ONE step from a given float32 state; the oracle starts from the same bits in float64.  N = 1027 rows (no
multiple of 16 or 256).  Per row: a clock from CLOCKS (clock 0: zero moments and zero vis_avg; otherwise random moments,
exp_avg_sq scaled with the square of the row's scale, Adam's exp_avg with the scale, LaProp's of order one), a scale 2^k
with k uniform in the variant's k_range ([-40, 30]; DESIGN.md derives that this stays inside what float32 carries),
visibility uniform in (0, 1), every 7th row times 1e-6, every 11th row unseen; gradients are randn * scale * visibility.
Every group draws from a generator of its own, so a test that steps a few groups sees the rows the noise table measured.

Hyper-parameters reach the kernel as C floats: the oracle is fed their float32-rounded values as doubles
(Variant.oracle_options), ParameterClass the plain ones (Variant.options).

figures() returns {(group, figure): value}; each value is a maximum over the rows stepped.  A zero denominator has to be
met by a numerator that is exactly zero, a non-finite result counts as infinitely wrong (both give inf):
  exp_avg_sq   max(0, |v - v_oracle| - 2^-150) / v_oracle entrywise (every term is non-negative).  The subtracted term is
               the one rounding of a stored float32 below 2^-126, where the format's spacing is 2^-149 whatever the
               arithmetic: a faint row's first (1 - beta2) g^2 lands there (the safe range of the gradient)
  exp_avg      |m - m_oracle| over the row maximum of b1 |m_old| + (1 - b1) |u or g| (local_vector: sum_r |B_rk| |g_r| in
               place of |g|, divided by the oracle's denominator where u enters)
  param        max(0, |p - p_oracle| - 2^-24 |p_oracle|) over the row maximum of |dec| (local_vector: sum_k |B_rk| |dec_k|);
               the subtracted term is the one rounding of the stored parameter
  step         largest difference of the clock on any row: 0
  vis_avg      distance in float32 ulps of the oracle's value: at most 2 (two roundings of two positive terms); without
               visibility the column is bit-identical to its old value, any difference is inf
  unseen       entries of the rows not stepped (parameters, both moments, step, vis_avg) that differ from the old bits: 0

NOISE is the float32 oracle against the float64 oracle on these cases, per (variant, algorithm, group type), the worst
over all groups of the type and SEEDS, rounded up to two digits (test_noise_table re-measures it;
profiles/r13_optim_contract.txt has the run).  bound = min(MARGIN x NOISE, CAP).  MARGIN = 4, as for the colour model's
contract: the kernel orders and contracts the same float32 operations differently and uses the device's powf, sqrtf and
division.  CAP = 1e-4 is BASELINE.json's criterion; a bound above it would say nothing.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from helpers import oracle_optim as oo

N = 1027
CLOCKS = (0.0, 1.0, 2.0, 3.0, 10.0, 1000.0, 1e5, 4e5)
MARGIN, CAP = 4.0, 1e-4
SEEDS = (0, 1, 2, 3, 4)
FAINT_EVERY, FAINT = 7, 1e-6
FIGURES = ("exp_avg_sq", "exp_avg", "param")
FIXED_BOUNDS = dict(step=0.0, vis_avg=2.0, unseen=0.0)
ALGOS = ("laprop", "adam")


def f32(x: float) -> float:
  """The value a C float argument takes, as a double."""
  return float(torch.tensor(x, dtype=torch.float32))


@dataclass(frozen=True)
class Variant:
  name: str
  betas: Tuple[float, float]
  vis_beta: float
  vis_smooth: float
  grad_clip: Optional[float] = 2.0
  bias_correction: bool = True
  eps: float = 1e-16
  visibility: bool = True                 # False: SparseAdam / SparseLaProp
  k_range: Tuple[int, int] = (-40, 30)
  grad_dtype: torch.dtype = torch.float32
  unseen_every: Optional[int] = 11
  moment_scale: float = 1.0               # sqrt(exp_avg_sq) of a started row over the row's scale, times e^randn
  algos: Tuple[str, ...] = ALGOS

  def options(self) -> dict:
    return dict(betas=self.betas, eps=self.eps, vis_beta=self.vis_beta, vis_smooth=self.vis_smooth,
                bias_correction=self.bias_correction, grad_clip=self.grad_clip)

  def oracle_options(self) -> dict:
    return dict(betas=(f32(self.betas[0]), f32(self.betas[1])), eps=f32(self.eps), vis_beta=f32(self.vis_beta),
                vis_smooth=f32(self.vis_smooth), bias_correction=self.bias_correction,
                grad_clip=None if self.grad_clip is None else f32(self.grad_clip))


_REF = dict(betas=(0.8, 0.9), vis_beta=0.95, vis_smooth=0.001)          # the reference's, mlp_scene.py:45-52
REFERENCE = Variant("reference", **_REF)
STRESS = Variant("stress", betas=(0.9, 0.999), vis_beta=0.999, vis_smooth=0.01)     # 1 - beta^t cancels at small t
NO_BIAS_CORRECTION = Variant("reference/no_bias_correction", bias_correction=False, **_REF)
NO_CLIP = Variant("reference/no_clip", grad_clip=None, algos=("laprop",), **_REF)
# second moments of a quarter the size: with the faint rows (u of order 1e-3) counted, most entries still clip
CLIP_HALF = Variant("reference/clip0.5", grad_clip=0.5, moment_scale=0.25, algos=("laprop",), **_REF)
NO_VISIBILITY = Variant("reference/no_visibility", visibility=False, **_REF)
ALL_VISIBLE = Variant("reference/all_visible", unseen_every=None, **_REF)           # M = N
# float16 carries 2^-24 to 65504: the row scales stay inside it, the faint rows reach its subnormals and zero
F16_GRAD = Variant("reference/f16_grad", grad_dtype=torch.float16, k_range=(-8, 8), **_REF)
VARIANTS = (REFERENCE, STRESS, NO_BIAS_CORRECTION, NO_CLIP, CLIP_HALF, NO_VISIBILITY, ALL_VISIBLE, F16_GRAD)


@dataclass(frozen=True)
class Group:
  name: str
  kind: str
  shape: Tuple[int, ...]
  lr: float

  @property
  def D(self) -> int:
    d = 1
    for s in self.shape:
      d *= s
    return d


WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 32, 33, 48, 64)
_LRS = (0.3, 0.08, 0.01, 0.1, 5.0, 0.002)                               # config/scene/mlp.yaml:8-14 and a small one
_SPECS = ([(f"{kind}{D}", kind, (D,)) for kind in (oo.SCALAR, oo.VECTOR) for D in WIDTHS]
          + [("local3", oo.LOCAL_VECTOR, (3,))]
          + [(f"{kind}{a}x{b}", kind, (a, b)) for kind in (oo.SCALAR, oo.VECTOR) for a, b in ((3, 16), (3, 9))])
GROUPS = tuple(Group(name, kind, shape, _LRS[i % len(_LRS)]) for i, (name, kind, shape) in enumerate(_SPECS))
BY_NAME = {g.name: g for g in GROUPS}


def instantiation(g: Group) -> str:
  """The kernel of csrc/optim.hip a group runs on."""
  if g.kind == oo.LOCAL_VECTOR:
    return "narrow<3,local_vector>"
  return f"narrow<{g.D},{g.kind}>" if g.D <= 4 else f"wide<{g.kind}>"


@dataclass
class Case:
  variant: Variant
  algo: str
  seed: int
  groups: Tuple[Group, ...]
  tensors: dict          # name -> (N, *shape) float32
  grads: dict            # name -> (N, *shape) of variant.grad_dtype
  state: dict            # step, vis_avg, groups[name] = exp_avg (N, D), exp_avg_sq (N, D) or (N,)
  visibility: torch.Tensor   # (N,) float32, zero on the unseen rows
  basis: torch.Tensor        # (N, 3, 3) float32
  scale: torch.Tensor        # (N,) float64

  @property
  def id(self) -> str:
    return f"{self.variant.name}-{self.algo}-seed{self.seed}"

  @property
  def types(self) -> dict:
    return {g.name: g.kind for g in self.groups}


def _basis(gen) -> torch.Tensor:
  """R(q) diag(exp(log_scaling)) (harness.point_basis) evaluated in float64, rounded once."""
  q = torch.nn.functional.normalize(torch.randn(N, 4, generator=gen, dtype=torch.float64), dim=1)
  s = torch.exp(torch.randn(N, 3, generator=gen, dtype=torch.float64) - 3.0)
  x, y, z, w = q.unbind(-1)
  R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                   2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                   2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(N, 3, 3)
  return (R * s.unsqueeze(-2)).float()


def make_case(variant: Variant, algo: str, seed: int, groups=GROUPS) -> Case:
  gen = torch.Generator().manual_seed(seed)
  lo, hi = variant.k_range
  scale = 2.0 ** torch.randint(lo, hi + 1, (N,), generator=gen).double()
  clock = torch.tensor(CLOCKS, dtype=torch.float64)[torch.randint(0, len(CLOCKS), (N,), generator=gen)]
  vis = torch.rand(N, generator=gen, dtype=torch.float64).clamp_min(2.0 ** -20)
  vis[::FAINT_EVERY] *= FAINT
  if variant.unseen_every:
    vis[::variant.unseen_every] = 0.0
  vis = vis.float()
  started = clock > 0
  # a running visibility as the clock would have left it: (1 - vis_beta^t) of a mean visibility
  vis_avg = torch.rand(N, generator=gen, dtype=torch.float64) * (1 - f32(variant.vis_beta) ** clock) * started
  if not variant.visibility:
    vis_avg.zero_()
  basis = _basis(gen)
  tensors, grads, moments = {}, {}, {}
  for g in groups:
    gg = torch.Generator().manual_seed(7919 * seed + 101 * GROUPS.index(BY_NAME[g.name]) + 13)
    shape = (N,) + g.shape
    bc = (N,) + (1,) * len(g.shape)
    tensors[g.name] = torch.randn(shape, generator=gg)
    raw = torch.randn(shape, generator=gg, dtype=torch.float64) * (scale * vis.double()).view(bc)
    grads[g.name] = raw.float().to(variant.grad_dtype)
    sq_shape = (N, g.D) if g.kind == oo.SCALAR else (N,)
    spread = torch.exp(torch.randn(sq_shape, generator=gg, dtype=torch.float64))
    sq = (variant.moment_scale * spread * scale.view((N,) + (1,) * (len(sq_shape) - 1))) ** 2
    avg = torch.randn(N, g.D, generator=gg, dtype=torch.float64) * (0.5 if algo == "laprop" else scale.view(N, 1))
    moments[g.name] = dict(exp_avg=(avg * started.view(N, 1)).float(),
                           exp_avg_sq=(sq * started.view((N,) + (1,) * (len(sq_shape) - 1))).float())
  state = dict(step=clock.float(), vis_avg=vis_avg.float(), groups=moments)
  return Case(variant, algo, seed, tuple(groups), tensors, grads, state, vis, basis, scale)


def indexes(case: Case, order: str = "ascending", M: Optional[int] = None) -> torch.Tensor:
  """The visible rows ascending, or a random permutation of them; the first M of either."""
  idx = case.visibility.nonzero().squeeze(1)
  if order == "permuted":
    idx = idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(1000 + case.seed))]
  else:
    assert order == "ascending", order
  return idx if M is None else idx[:M]


def clone_state(state: dict, dtype=None, device=None) -> dict:
  to = lambda t: t.to(dtype=dtype, device=device, copy=True)
  return dict(step=to(state["step"]), vis_avg=to(state["vis_avg"]),
              groups={k: {n: to(v) for n, v in g.items()} for k, g in state["groups"].items()})


def oracle_step(case: Case, idx: torch.Tensor, dtype=torch.float64, without_grad=(), step_fn=None) -> dict:
  """One step of the oracle (or of `step_fn`, a deviant copy of it) from the case's state in `dtype`:
  dict(tensors, state, terms).  Groups named in `without_grad` have no gradient."""
  tensors = {k: v.to(dtype, copy=True) for k, v in case.tensors.items()}
  state = clone_state(case.state, dtype)
  grads = {k: (None if k in without_grad else v.to(dtype)) for k, v in case.grads.items()}
  lrs = {g.name: f32(g.lr) for g in case.groups}
  terms = (step_fn or oo.step)(tensors, grads, state, lrs, case.types, idx,
                               visibility=case.visibility[idx].to(dtype) if case.variant.visibility else None,
                               basis=case.basis[idx].to(dtype), algo=case.algo, return_terms=True,
                               **case.variant.oracle_options())
  return dict(tensors=tensors, state=state, terms=terms)


def _worst(num: torch.Tensor, den: torch.Tensor) -> float:
  if not num.numel():
    return 0.0
  if not torch.isfinite(num).all():
    return float("inf")
  zero = den == 0
  if (num[zero] != 0).any():
    return float("inf")
  rel = num[~zero] / den[~zero]
  return rel.max().item() if rel.numel() else 0.0


def figures(case: Case, idx: torch.Tensor, got: dict, ref: dict) -> dict:
  """{(group or '', figure): value} of `got` (tensors, state) against the float64 oracle result `ref`."""
  out = {}
  d = lambda t: t.detach().double().cpu()
  b1 = f32(case.variant.betas[0])
  for g in case.groups:
    terms = ref["terms"].get(g.name)
    rows = lambda t: d(t).reshape(N, -1)[idx]
    got_s, ref_s, old_s = got["state"]["groups"][g.name], ref["state"]["groups"][g.name], case.state["groups"][g.name]
    if terms is None:                         # no gradient: the group is untouched
      same = (torch.equal(d(got["tensors"][g.name]), d(case.tensors[g.name]))
              and all(torch.equal(d(got_s[n]), d(old_s[n])) for n in old_s))
      out[(g.name, "untouched")] = 0.0 if same else float("inf")
      continue
    v_ref = rows(ref_s["exp_avg_sq"])
    out[(g.name, "exp_avg_sq")] = _worst(((rows(got_s["exp_avg_sq"]) - v_ref).abs() - 2.0 ** -150).clamp_min(0), v_ref)
    size = terms["momentum_in"].abs()
    if g.kind == oo.LOCAL_VECTOR:
      size = terms["g_abs"] if case.algo == "adam" else terms["g_abs"] / terms["denom"]
    den = (b1 * rows(old_s["exp_avg"]).abs() + (1 - b1) * size).amax(1)
    out[(g.name, "exp_avg")] = _worst((rows(got_s["exp_avg"]) - rows(ref_s["exp_avg"])).abs().amax(1), den)
    p_ref = rows(ref["tensors"][g.name])
    num = ((rows(got["tensors"][g.name]) - p_ref).abs() - 2.0 ** -24 * p_ref.abs()).clamp_min(0).amax(1)
    dec = terms["dec_abs"] if g.kind == oo.LOCAL_VECTOR else terms["dec"].abs()
    out[(g.name, "param")] = _worst(num, dec.amax(1))
  out[("", "step")] = (d(got["state"]["step"]) - ref["state"]["step"]).abs().max().item()
  va, va_ref, va_old = d(got["state"]["vis_avg"]), ref["state"]["vis_avg"], d(case.state["vis_avg"])
  if case.variant.visibility:
    ulp = torch.exp2(torch.frexp(va_ref[idx].float()).exponent.double() - 24)      # frexp: |x| = m 2^e, 0.5 <= m < 1
    out[("", "vis_avg")] = _worst((va[idx] - va_ref[idx]).abs(), ulp)
  else:
    out[("", "vis_avg")] = 0.0 if torch.equal(va, va_old) else float("inf")
  unseen = torch.ones(N, dtype=torch.bool)
  unseen[idx] = False
  differ = int((d(got["state"]["step"])[unseen] != d(case.state["step"])[unseen]).sum()) + int((va[unseen] != va_old[unseen]).sum())
  for g in case.groups:
    differ += int((d(got["tensors"][g.name])[unseen] != d(case.tensors[g.name])[unseen]).sum())
    for n, old in case.state["groups"][g.name].items():
      differ += int((d(got["state"]["groups"][g.name][n])[unseen] != d(old)[unseen]).sum())
  out[("", "unseen")] = float(differ)
  return out


# (variant, algorithm, group type) -> float32 oracle against float64 oracle: (exp_avg_sq, exp_avg, param)
NOISE = {
  ("reference", "laprop", "scalar"): (3.3e-07, 2.4e-07, 1.3e-05),
  ("reference", "laprop", "vector"): (3.3e-07, 2.4e-07, 3.7e-06),
  ("reference", "laprop", "local_vector"): (4.0e-07, 1.5e-07, 5.8e-07),
  ("reference", "adam", "scalar"): (3.3e-07, 1.7e-07, 1.8e-05),
  ("reference", "adam", "vector"): (3.3e-07, 1.6e-07, 1.7e-06),
  ("reference", "adam", "local_vector"): (4.0e-07, 1.6e-07, 5.8e-07),
  ("stress", "laprop", "scalar"): (3.7e-07, 3.0e-06, 1.6e-05),
  ("stress", "laprop", "vector"): (3.4e-07, 3.3e-06, 5.4e-05),
  ("stress", "laprop", "local_vector"): (3.6e-07, 9.1e-07, 6.9e-06),
  ("stress", "adam", "scalar"): (3.7e-07, 1.7e-07, 1.1e-05),
  ("stress", "adam", "vector"): (3.4e-07, 1.6e-07, 1.3e-05),
  ("stress", "adam", "local_vector"): (3.6e-07, 1.5e-07, 1.0e-05),
  ("reference/no_bias_correction", "laprop", "scalar"): (3.3e-07, 1.8e-07, 6.2e-06),
  ("reference/no_bias_correction", "laprop", "vector"): (3.3e-07, 2.2e-07, 2.9e-06),
  ("reference/no_bias_correction", "laprop", "local_vector"): (4.0e-07, 1.2e-07, 1.7e-06),
  ("reference/no_bias_correction", "adam", "scalar"): (3.3e-07, 1.7e-07, 1.8e-05),
  ("reference/no_bias_correction", "adam", "vector"): (3.3e-07, 1.6e-07, 1.6e-05),
  ("reference/no_bias_correction", "adam", "local_vector"): (4.0e-07, 1.6e-07, 8.1e-07),
  ("reference/no_clip", "laprop", "scalar"): (3.3e-07, 2.4e-07, 1.8e-05),
  ("reference/no_clip", "laprop", "vector"): (3.3e-07, 2.4e-07, 4.8e-06),
  ("reference/no_clip", "laprop", "local_vector"): (4.0e-07, 1.5e-07, 5.8e-07),
  ("reference/clip0.5", "laprop", "scalar"): (3.6e-07, 1.5e-07, 6.3e-06),
  ("reference/clip0.5", "laprop", "vector"): (3.4e-07, 2.0e-07, 1.2e-05),
  ("reference/clip0.5", "laprop", "local_vector"): (4.0e-07, 1.3e-07, 1.4e-06),
  ("reference/no_visibility", "laprop", "scalar"): (1.4e-07, 2.1e-07, 8.1e-07),
  ("reference/no_visibility", "laprop", "vector"): (2.3e-07, 2.0e-07, 5.9e-06),
  ("reference/no_visibility", "laprop", "local_vector"): (4.0e-07, 1.4e-07, 8.1e-07),
  ("reference/no_visibility", "adam", "scalar"): (1.4e-07, 1.2e-07, 3.4e-07),
  ("reference/no_visibility", "adam", "vector"): (2.3e-07, 1.2e-07, 3.5e-07),
  ("reference/no_visibility", "adam", "local_vector"): (4.0e-07, 1.2e-07, 8.1e-07),
  ("reference/all_visible", "laprop", "scalar"): (3.4e-07, 2.4e-07, 1.3e-05),
  ("reference/all_visible", "laprop", "vector"): (3.4e-07, 2.4e-07, 3.7e-06),
  ("reference/all_visible", "laprop", "local_vector"): (4.3e-07, 1.5e-07, 5.8e-07),
  ("reference/all_visible", "adam", "scalar"): (3.4e-07, 1.7e-07, 1.8e-05),
  ("reference/all_visible", "adam", "vector"): (3.4e-07, 1.6e-07, 1.7e-06),
  ("reference/all_visible", "adam", "local_vector"): (4.3e-07, 1.6e-07, 5.8e-07),
  ("reference/f16_grad", "laprop", "scalar"): (3.3e-07, 2.0e-07, 2.5e-05),
  ("reference/f16_grad", "laprop", "vector"): (3.7e-07, 1.9e-07, 4.1e-05),
  ("reference/f16_grad", "laprop", "local_vector"): (7.7e-07, 1.5e-07, 2.7e-07),
  ("reference/f16_grad", "adam", "scalar"): (3.3e-07, 1.6e-07, 1.1e-05),
  ("reference/f16_grad", "adam", "vector"): (3.7e-07, 1.7e-07, 1.0e-06),
  ("reference/f16_grad", "adam", "local_vector"): (7.7e-07, 1.7e-07, 4.5e-07),
}


def bound(case: Case, group: str, figure: str) -> float:
  if figure in FIXED_BOUNDS:
    return FIXED_BOUNDS[figure]
  if figure == "untouched":
    return 0.0
  noise = NOISE[(case.variant.name, case.algo, BY_NAME[group].kind)][FIGURES.index(figure)]
  return min(MARGIN * noise, CAP)


def outside(case: Case, figs: dict):
  """[(figure / bound, group, figure)] of the figures above their bound, largest first (a zero bound: inf)."""
  out = []
  for (group, figure), e in figs.items():
    b = bound(case, group, figure)
    if not e <= b:
      out.append((e / b if b > 0 else float("inf"), group, figure))
  return sorted(out, reverse=True)


def measure_noise(variants=VARIANTS, seeds=SEEDS) -> dict:
  """{(variant, algorithm, type): [exp_avg_sq, exp_avg, param]}: the float32 oracle against the float64 oracle, worst
  over GROUPS and seeds.  The fixed figures (step, vis_avg, unseen) have to hold for the float32 oracle as well."""
  worst = {}
  for variant in variants:
    for algo in variant.algos:
      for seed in seeds:
        case = make_case(variant, algo, seed)
        idx = indexes(case)
        figs = figures(case, idx, oracle_step(case, idx, torch.float32), oracle_step(case, idx))
        for (group, figure), e in figs.items():
          if figure in FIXED_BOUNDS:
            assert e <= FIXED_BOUNDS[figure], (case.id, figure, e)
            continue
          row = worst.setdefault((variant.name, algo, BY_NAME[group].kind), [0.0, 0.0, 0.0])
          row[FIGURES.index(figure)] = max(row[FIGURES.index(figure)], e)
  return worst


# ---- point_basis_rows: R(normalize(q)) diag(max(exp(log_scaling), eps)) per row (harness.point_basis)
BASIS_ROWS = 1027


def basis_inputs(seed: int = 0):
  """(log_scaling, rotation) float32: log scales uniform in [-20, 10] (below log(1e-4) the clamp decides), quaternions
  of any length from 1e-3 to 1e3, row 5 a zero quaternion (F.normalize's clamp decides: the identity)."""
  gen = torch.Generator().manual_seed(seed)
  ls = torch.rand(BASIS_ROWS, 3, generator=gen) * 30 - 20
  rot = torch.randn(BASIS_ROWS, 4, generator=gen) * 10 ** (torch.rand(BASIS_ROWS, 1, generator=gen) * 6 - 3)
  rot[5] = 0
  return ls, rot


def basis_figure(got: torch.Tensor, ls: torch.Tensor, rot: torch.Tensor) -> float:
  """Worst row of |got - want| over the row's largest |want|, want = harness.point_basis in float64."""
  from splat_trainer_amd.harness import point_basis
  want = point_basis(ls.double(), rot.double())
  got = got.detach().double().cpu()
  assert got.shape == want.shape
  return _worst((got - want).abs().amax(dim=(1, 2)), want.abs().amax(dim=(1, 2)))


def measure_basis_noise(seeds=SEEDS) -> float:
  from splat_trainer_amd.harness import point_basis
  return max(basis_figure(point_basis(*basis_inputs(s)), *basis_inputs(s)) for s in seeds)


BASIS_NOISE = 5.9e-7         # harness.point_basis in float32 against float64, worst row over SEEDS, rounded up
BASIS_BOUND = MARGIN * BASIS_NOISE
