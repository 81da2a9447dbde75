"""CPU checks of the optimizer step's one-step contract (optim_contract.py): the float32-against-float64 noise table
behind the GPU bounds, the oracle's return_terms, and ten planted deviations of the model.

The deviations live in `deviant_step`, a copy of oracle/optim_oracle.py's step with one switch each, run in fp64 on the
GPU tests' own cases: a kernel that made the same mistake would fail tests/test_gpu_optim_contract.py on the case and
figure named in PLANTED, by the factor stated there at least.  `old_criterion` is what tests/test_gpu_optim.py asks of
the same deviation: four steps from a zero state, rows of one size (randn x U(0, 1) gradients, 40 % of the rows unseen),
betas 0.8 / 0.95, every tensor within 2e-5 of its largest magnitude; it is evaluated on the contract's groups and row
count.  It misses (PLANTED's last column): the rows skipped below a visibility of 1e-5 (its rows hold none), eps inside
the square root (none of its rows has a second moment near eps^2) and the decrement of one tail column 1e-4 too large
(2e-5 of a parameter of size 4 hides it) -- and, whatever the deviation, every instantiation its two feature shapes do
not reach.

`python tests/test_optim_contract_host.py` prints the tables of profiles/r13_optim_contract.txt.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import optim_contract as oc  # noqa: E402
from helpers import oracle_optim as oo  # noqa: E402

DEVIATIONS = ("bias_correction_at_t", "vector_sum_for_mean", "basis_not_transposed", "clip_on_momentum", "rho_from_avg",
              "second_moment_unweighted", "norm_drops_tail", "eps_inside_sqrt", "faint_rows_skipped", "tail_column_dec")


@torch.no_grad()
def deviant_step(dev, tensors, grads, state, lrs, types, indexes, visibility=None, basis=None, algo="laprop",
                 betas=(0.9, 0.999), eps=1e-16, vis_beta=0.9, vis_smooth=0.01, bias_correction=True, grad_clip=None,
                 return_terms=False):
  """oracle/optim_oracle.py's step, restated, with the deviation `dev` (None: none) planted."""
  assert dev is None or dev in DEVIATIONS, dev
  beta1, beta2 = betas
  idx = indexes
  t = state["step"][idx] + 1
  state["step"][idx] = t
  tb = t - 1 if dev == "bias_correction_at_t" else t                               # 1
  if visibility is not None:
    w = visibility.to(t.dtype)
    avg = vis_beta * state["vis_avg"][idx] + (1 - vis_beta) * w
    state["vis_avg"][idx] = avg
    avg_hat = avg / (1 - vis_beta ** tb) if bias_correction else avg
    if dev == "rho_from_avg":                                                      # 5
      avg_hat = avg
    inv_w = 1 / (w + vis_smooth)
    rho = w / (avg_hat + vis_smooth)
  else:
    w = torch.ones_like(t)
    inv_w = torch.ones_like(t)
    rho = torch.ones_like(t)
  bc1 = 1 - beta1 ** tb if bias_correction else torch.ones_like(t)
  bc2 = 1 - beta2 ** tb if bias_correction else torch.ones_like(t)
  live = (w >= 1e-5) if dev == "faint_rows_skipped" else torch.ones_like(t, dtype=torch.bool)       # 9
  for name, p in tensors.items():
    grad = grads.get(name)
    if grad is None:
      continue
    n = p.shape[0]
    flat = p.reshape(n, -1)
    D = flat.shape[1]
    kind = types.get(name, oo.SCALAR)
    raw = grad.reshape(n, -1)[idx]
    g = raw * inv_w[:, None]
    rotate = "mkr,mr->mk" if dev == "basis_not_transposed" else "mrk,mr->mk"       # 3
    if kind == oo.LOCAL_VECTOR:
      g = torch.einsum(rotate, basis.to(g.dtype), g)
      raw = torch.einsum(rotate, basis.to(g.dtype), raw)
    g2 = raw if dev == "second_moment_unweighted" else g                           # 6
    st = state["groups"][name]
    if kind == oo.SCALAR:
      v = beta2 * st["exp_avg_sq"][idx] + (1 - beta2) * g2 * g2
      second = v
    else:
      sq = g2 * g2
      if dev == "norm_drops_tail" and D > 4:                                       # 7 (the wide kernel's reduction)
        sq = sq[:, :16 * (D // 16)]
      s = sq.sum(dim=1) if dev == "vector_sum_for_mean" else sq.sum(dim=1) / D     # 2
      if dev is None:
        s = (g2 * g2).mean(dim=1)
      v = beta2 * st["exp_avg_sq"][idx] + (1 - beta2) * s
      second = v[:, None]
    if dev == "eps_inside_sqrt":                                                   # 8
      denom = torch.sqrt(second / bc2[:, None] + eps)
    else:
      denom = torch.sqrt(second / bc2[:, None]) + eps
    m = st["exp_avg"][idx]
    clip = grad_clip is not None and grad_clip > 0
    if algo == "laprop":
      u = g / denom
      if clip and dev != "clip_on_momentum":
        u = u.clamp(-grad_clip, grad_clip)
      m = beta1 * m + (1 - beta1) * u
      if clip and dev == "clip_on_momentum":                                       # 4
        m = m.clamp(-grad_clip, grad_clip)
      dec = lrs[name] * (rho / bc1)[:, None] * m
    else:
      m = beta1 * m + (1 - beta1) * g
      dec = lrs[name] * (rho / bc1)[:, None] * m / denom
    if dev == "tail_column_dec" and kind == oo.SCALAR and D % 16 == 1 and D > 16:  # 10: one column, 1e-4 of itself
      dec[:, -1] *= 1 + 1e-4
    if kind == oo.LOCAL_VECTOR:
      dec = torch.einsum("mrk,mk->mr", basis.to(g.dtype), dec)
    lv = live[:, None]
    st["exp_avg_sq"][idx] = torch.where(live if v.dim() == 1 else lv, v, st["exp_avg_sq"][idx])
    st["exp_avg"][idx] = torch.where(lv, m, st["exp_avg"][idx])
    flat[idx] = torch.where(lv, flat[idx] - dec, flat[idx])
  return None


def _planted(dev, case):
  """[(figure / bound, group, figure)] above the bound, largest first: the deviant model in fp64 against the oracle."""
  idx = oc.indexes(case)
  ref = oc.oracle_step(case, idx)
  got = oc.oracle_step(case, idx, step_fn=lambda *a, return_terms, **kw: deviant_step(dev, *a, **kw))
  return oc.outside(case, oc.figures(case, idx, got, ref))


OLD_TOL = 2e-5


def old_criterion(dev, algo, steps=4, seed=0):
  """tests/test_gpu_optim.py's comparison of the deviant model with the oracle: the worst of parameters, exp_avg and
  exp_avg_sq over the groups, each relative to its tensor's largest magnitude.  It passes below OLD_TOL."""
  n = oc.N
  options = dict(betas=(0.8, 0.95), vis_beta=0.999, vis_smooth=0.01, bias_correction=True, grad_clip=2.0)
  gen = torch.Generator().manual_seed(seed)
  shapes = {g.name: (n,) + g.shape for g in oc.GROUPS}
  types = {g.name: g.kind for g in oc.GROUPS}
  lrs = {g.name: g.lr for g in oc.GROUPS}
  a = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
  b = {k: v.clone() for k, v in a.items()}
  sa, sb = oo.new_state(a, types), oo.new_state(b, types)
  basis = oc.make_case(oc.REFERENCE, algo, seed, groups=()).basis.double()
  for _ in range(steps):
    visible = torch.rand(n, generator=gen, dtype=torch.float64) * (torch.rand(n, generator=gen) < 0.6)
    grads = {k: torch.randn(s, generator=gen, dtype=torch.float64) * visible.view(-1, *[1] * (len(s) - 1))
             for k, s in shapes.items()}
    idx = visible.nonzero().squeeze(1)
    kw = dict(visibility=visible[idx], basis=basis[idx], algo=algo, **options)
    oo.step(a, grads, sa, lrs, types, idx, **kw)
    deviant_step(dev, b, grads, sb, lrs, types, idx, **kw)
  worst = 0.0
  rel = lambda x, y: ((x - y).abs().max() / y.abs().max().clamp_min(1e-30)).item() if torch.isfinite(x).all() else float("inf")
  for k in shapes:
    worst = max(worst, rel(b[k], a[k]), rel(sb["groups"][k]["exp_avg"], sa["groups"][k]["exp_avg"]),
                rel(sb["groups"][k]["exp_avg_sq"], sa["groups"][k]["exp_avg_sq"]))
  return worst


# deviation -> (variant, algorithm, group, figure that lands outside, by this factor at least, the old criterion sees it)
PLANTED = {
  "bias_correction_at_t": (oc.REFERENCE, "laprop", "vector64", "param", 1e6, True),        # 1 / 0 on the rows at clock 0
  "vector_sum_for_mean": (oc.REFERENCE, "laprop", "vector64", "exp_avg_sq", 1e6, True),
  "basis_not_transposed": (oc.REFERENCE, "adam", "local3", "exp_avg_sq", 1e6, True),
  "clip_on_momentum": (oc.REFERENCE, "laprop", "vector16", "exp_avg", 1e5, True),
  "rho_from_avg": (oc.REFERENCE, "laprop", "local3", "param", 1e6, True),
  "second_moment_unweighted": (oc.STRESS, "laprop", "vector64", "exp_avg_sq", 1e5, True),
  "norm_drops_tail": (oc.REFERENCE, "laprop", "vector17", "exp_avg_sq", 100.0, True),      # one column of 17
  "eps_inside_sqrt": (oc.REFERENCE, "laprop", "vector1", "param", 1e6, False),             # only rows near eps differ
  "faint_rows_skipped": (oc.REFERENCE, "adam", "vector64", "exp_avg", 1e5, False),
  "tail_column_dec": (oc.REFERENCE, "laprop", "scalar17", "param", 1.5, False),
}


@pytest.mark.parametrize("dev", DEVIATIONS)
def test_planted_deviation_lands_outside(dev):
  variant, algo, group, figure, least, old_sees = PLANTED[dev]
  case = oc.make_case(variant, algo, 0)
  found = {(g, f): r for r, g, f in _planted(dev, case)}
  print(dev, case.id, sorted(((r, g, f) for (g, f), r in found.items()), reverse=True)[:3])
  assert found.get((group, figure), 0.0) > least, (dev, case.id, group, figure, found.get((group, figure)))
  old = old_criterion(dev, algo)
  print(dev, f"old criterion: {old:.2e} against {OLD_TOL:.0e}")
  assert (old >= OLD_TOL) == old_sees, (dev, old)


def test_the_old_criterion_misses_what_is_confined_to_faint_rows_or_one_column():
  for dev in ("faint_rows_skipped", "tail_column_dec"):
    assert PLANTED[dev][5] is False
    for algo in PLANTED[dev][0].algos:
      assert old_criterion(dev, algo) < OLD_TOL, (dev, algo)
      assert _planted(dev, oc.make_case(PLANTED[dev][0], algo, 0)), (dev, algo)


@pytest.mark.parametrize("algo", oc.ALGOS)
def test_deviant_copy_without_a_deviation_is_the_oracle(algo):
  for variant in (oc.REFERENCE, oc.NO_VISIBILITY):
    case = oc.make_case(variant, algo, 1)
    idx = oc.indexes(case, "permuted")
    ref = oc.oracle_step(case, idx)
    got = oc.oracle_step(case, idx, step_fn=lambda *a, return_terms, **kw: deviant_step(None, *a, **kw))
    for k in ref["tensors"]:
      assert torch.equal(got["tensors"][k], ref["tensors"][k]), k
      for n in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(got["state"]["groups"][k][n], ref["state"]["groups"][k][n]), (k, n)
    assert torch.equal(got["state"]["step"], ref["state"]["step"])
    assert torch.equal(got["state"]["vis_avg"], ref["state"]["vis_avg"])
    assert not oc.outside(case, oc.figures(case, idx, got, ref))


def test_noise_table():
  """NOISE is the float32 oracle against the float64 oracle on the GPU tests' cases, rounded up to two digits.  A CPU
  whose vector width sums mean() and einsum() in another order moves the worst entry of a figure: the re-measurement may
  differ from the table by 1.5x either way before this fails.  Every bound is MARGIN x NOISE, capped at CAP."""
  measured = oc.measure_noise()
  assert set(measured) == set(oc.NOISE), set(measured) ^ set(oc.NOISE)
  for key, row in sorted(measured.items()):
    case = oc.make_case(next(v for v in oc.VARIANTS if v.name == key[0]), key[1], 0, groups=())
    group = next(g.name for g in oc.GROUPS if g.kind == key[2])
    for figure, e, stored in zip(oc.FIGURES, row, oc.NOISE[key]):
      b = oc.bound(case, group, figure)
      print(f"{key[0]:30s} {key[1]:7s} {key[2]:13s} {figure:11s} measured {e:.2e}  table {stored:.1e}  bound {b:.1e}")
      assert stored / 1.5 <= e <= stored * 1.5, (key, figure, e, stored)
      assert b == min(oc.MARGIN * stored, oc.CAP) and b <= 1e-4 and oc.MARGIN == 4.0, (key, figure, b)


def test_basis_noise():
  e = oc.measure_basis_noise()
  print(f"point_basis float32 against float64, worst row: {e:.2e}  table {oc.BASIS_NOISE:.1e}  bound {oc.BASIS_BOUND:.1e}")
  assert oc.BASIS_NOISE / 1.5 <= e <= oc.BASIS_NOISE * 1.5 and oc.BASIS_BOUND == 4 * oc.BASIS_NOISE <= 1e-4


@pytest.mark.parametrize("algo", oc.ALGOS)
def test_terms_agree_with_the_oracles_outputs(algo):
  case = oc.make_case(oc.REFERENCE, algo, 2)
  idx = oc.indexes(case, "permuted")
  ref = oc.oracle_step(case, idx)
  # the flag changes no result
  tensors = {k: v.double().clone() for k, v in case.tensors.items()}
  state = oc.clone_state(case.state, torch.float64)
  out = oo.step(tensors, {k: v.double() for k, v in case.grads.items()}, state, {g.name: oc.f32(g.lr) for g in case.groups},
                case.types, idx, visibility=case.visibility[idx].double(), basis=case.basis[idx].double(), algo=algo,
                **case.variant.oracle_options())
  assert out is None
  b1 = oc.f32(case.variant.betas[0])
  B = case.basis[idx].double()
  for g in case.groups:
    k, t = g.name, ref["terms"][g.name]
    assert torch.equal(tensors[k], ref["tensors"][k]), k
    for n in ("exp_avg", "exp_avg_sq"):
      assert torch.equal(state["groups"][k][n], ref["state"]["groups"][k][n]), (k, n)
    rows = lambda x: x.double().reshape(oc.N, -1)[idx]
    dec = rows(case.tensors[k]) - rows(ref["tensors"][k])                      # the decrement is the parameter difference
    assert (dec - t["dec"]).abs().max() <= 1e-12 * t["dec"].abs().max().clamp_min(1.0), k
    m = b1 * rows(case.state["groups"][k]["exp_avg"]) + (1 - b1) * t["momentum_in"]
    assert torch.allclose(m, rows(ref["state"]["groups"][k]["exp_avg"]), rtol=1e-13, atol=0), k
    sq = t["g"] * t["g"] if g.kind == oo.SCALAR else (t["g"] * t["g"]).mean(1, keepdim=True)
    b2 = oc.f32(case.variant.betas[1])
    v = b2 * rows(case.state["groups"][k]["exp_avg_sq"]) + (1 - b2) * sq
    assert torch.allclose(v, rows(ref["state"]["groups"][k]["exp_avg_sq"]), rtol=1e-13, atol=0), k
    if g.kind == oo.LOCAL_VECTOR:
      weighted = rows(case.grads[k]) / (case.visibility[idx].double() + oc.f32(case.variant.vis_smooth))[:, None]
      assert torch.allclose(t["g_abs"], torch.einsum("mrk,mr->mk", B.abs(), weighted.abs()), rtol=1e-13, atol=0)
      assert (t["g"].abs() <= t["g_abs"] * (1 + 1e-12)).all() and (t["dec"].abs() <= t["dec_abs"] * (1 + 1e-12)).all()
    else:
      assert set(t) == {"g", "momentum_in", "denom", "dec"}
  assert torch.equal(state["step"], ref["state"]["step"]) and torch.equal(state["vis_avg"], ref["state"]["vis_avg"])


def test_cases_reach_every_instantiation_and_hold_what_they_claim():
  reached = {oc.instantiation(g) for g in oc.GROUPS}
  assert reached == ({f"narrow<{D},{k}>" for D in (1, 2, 3, 4) for k in ("scalar", "vector")}
                     | {"narrow<3,local_vector>", "wide<scalar>", "wide<vector>"}) and len(reached) == 11
  assert {g.D for g in oc.GROUPS if g.D > 4} == {5, 15, 16, 17, 32, 33, 48, 64, 27}
  case = oc.make_case(oc.REFERENCE, "laprop", 0)
  idx = oc.indexes(case)
  unseen = torch.ones(oc.N, dtype=torch.bool)
  unseen[idx] = False
  assert unseen[::11].all() and int(unseen.sum()) == len(range(0, oc.N, 11))
  assert set(case.state["step"].tolist()) == set(oc.CLOCKS)
  fresh = case.state["step"] == 0
  assert not case.state["vis_avg"][fresh].any() and (case.state["vis_avg"][~fresh] > 0).all()
  for g in case.groups:
    st = case.state["groups"][g.name]
    assert not st["exp_avg"][fresh].any() and not st["exp_avg_sq"][fresh].any() and (st["exp_avg_sq"][~fresh] > 0).all()
  faint = case.visibility[idx] < 1e-5
  assert 0.1 < faint.float().mean() < 0.2
  perm = oc.indexes(case, "permuted")
  assert not torch.equal(perm, idx) and torch.equal(perm.sort().values, idx)
  assert oc.indexes(oc.make_case(oc.ALL_VISIBLE, "adam", 0)).numel() == oc.N
  # the clip of CLIP_HALF takes hold of most entries
  half = oc.make_case(oc.CLIP_HALF, "laprop", 0)
  terms = oc.oracle_step(half, oc.indexes(half))["terms"]
  clipped = torch.cat([(t["momentum_in"].abs() == 0.5).flatten() for t in terms.values()])
  assert clipped.double().mean() > 0.5


def _tables():
  print("float32 oracle against float64 oracle, worst over", len(oc.GROUPS), "groups and seeds", oc.SEEDS)
  print(f"{'variant':30s} {'algo':7s} {'type':13s} " + " ".join(f"{f + ' noise':>17s} {'bound':>8s}" for f in oc.FIGURES))
  for key, row in oc.measure_noise().items():
    case = oc.make_case(next(v for v in oc.VARIANTS if v.name == key[0]), key[1], 0, groups=())
    group = next(g.name for g in oc.GROUPS if g.kind == key[2])
    print(f"{key[0]:30s} {key[1]:7s} {key[2]:13s} " + " ".join(f"{e:17.2e} {oc.bound(case, group, f):8.1e}" for f, e in zip(oc.FIGURES, row)))
  print()
  print("planted deviations (fp64 deviant model against the oracle, seed 0): figure / bound, three largest; and the old")
  print(f"criterion of tests/test_gpu_optim.py (passes below {OLD_TOL:.0e})")
  for dev in DEVIATIONS:
    for variant in (oc.REFERENCE, oc.STRESS):
      for algo in oc.ALGOS:
        found = _planted(dev, oc.make_case(variant, algo, 0))
        print(f"{dev:26s} {variant.name:10s} {algo:7s} outside: {len(found):3d}  ",
              ", ".join(f"{g} {f} {r:.3g}x" for r, g, f in found[:3]) or "-")
    for algo in oc.ALGOS:
      old = old_criterion(dev, algo)
      print(f"{dev:26s} old criterion {algo:7s} {old:.2e}  {'sees it' if old >= OLD_TOL else 'MISSES it'}")


if __name__ == "__main__":
  _tables()
  print()
  print(f"point_basis float32 against float64, worst row over seeds {oc.SEEDS}: {oc.measure_basis_noise():.2e}  "
        f"bound {oc.BASIS_BOUND:.1e}")
