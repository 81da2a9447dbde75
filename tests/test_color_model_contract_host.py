"""CPU checks of the colour model's backward contract model (color_model_oracle.backward, cases and bounds in
color_model_contract.py): the exact form against autograd, the rounded form against autograd through the
straight-through forward, the float32-against-float64 noise table that bounds the GPU comparison, the sensitivity of
that comparison to five planted deviations of the model, and the dynamic range of the per-tile dy scale.

`python tests/test_color_model_contract_host.py` prints the measured tables (profiles/r12_color_model_contract.txt).
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import color_model_contract as cc  # noqa: E402
import color_model_oracle as cmo  # noqa: E402


def _autograd(case, params, args, round16):
  dt = torch.float64
  P = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in params.items()}
  pf, pos, cam, glo, dd, ds = (None if t is None else t.to(dt) for t in args)
  for t in (pf, cam, glo):
    t.requires_grad_(True)
  dif, spec = cmo.forward(P, pf, pos, cam, glo, case.L, case.S, round16=round16)
  loss = 0
  if dd is not None:
    loss = loss + (dif * dd).sum()
  if ds is not None:
    loss = loss + (spec * ds).sum()
  loss.backward()
  zero_if_none = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
  out = dict(point_features=zero_if_none(pf), glo=zero_if_none(glo), cam_pos=zero_if_none(cam))
  out.update({k: zero_if_none(p) for k, p in P.items()})
  return out


def _rel(got, ref):
  """per tensor: max |got - ref| over max |ref| (an all-zero reference: over 1)"""
  out = {}
  for k, r in ref.items():
    if r.numel():
      scale = r.abs().max().item()
      out[k] = (got[k] - r).abs().max().item() / (scale if scale > 0 else 1.0)
  return out


# F in {1, 5, 32, 33, 64}, with P = 0 and G = 0 among the splits
EXACT_SPLITS = [(1, 0), (0, 1), (3, 2), (5, 0), (16, 16), (0, 32), (17, 16), (31, 33), (64, 0)]


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("S", [2, 3, 4, 5])
def test_exact_form_matches_autograd(L, S):
  for P, G in EXACT_SPLITS:
    for sides in ("both", "diffuse", "specular"):
      case = cc.Case("exact", L, S, P, G, 70, sides=sides, geometry="edges", seed=P + 2 * G)
      params, args = cc.make_model(case).state_dict(), cc.inputs(case)
      got = cc.contract(case, params, args, torch.float64, round16=False)
      assert all(v.dtype == torch.float64 for v in got.values())
      for k, e in _rel(got, _autograd(case, params, args, False)).items():
        assert e <= 1e-12, (case.id, k, e)


def test_runs_in_the_dtype_of_its_inputs_and_zeroes_an_unused_branch():
  case = cc.Case("dtype", 2, 3, 5, 4, 40, sides="diffuse")
  params, args = cc.make_model(case).state_dict(), cc.inputs(case)
  g = cc.contract(case, params, args, torch.float32)
  assert all(v.dtype == torch.float32 for v in g.values())
  assert set(g) == {"point_features", "glo", "cam_pos", *cmo.param_keys(2)}
  for k, v in g.items():
    if k.startswith("directional_model") or k == "cam_pos":
      assert not v.any(), k
  assert g["point_features"].shape == (40, 5) and g["glo"].shape == (1, 4) and g["cam_pos"].shape == (3,)


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("S", [2, 5])
@pytest.mark.parametrize("P,G", [(1, 0), (16, 16), (31, 33)])
def test_rounded_form_within_f16_noise_of_straight_through_autograd(L, S, P, G):
  """The rounded backward differs from autograd through forward(round16=True) only by the rounding of dy (autograd's dy
  is exact; operands and activations are the same f16 values).  f16 keeps 11 bits, so a quantised dy entry is off by at
  most 2^-11 of itself.  A product contracts K such entries, K <= 128 (the encoder's dy is [dz x, dz], 2 F <= 128 wide);
  independent errors grow as sqrt(K) 2^-11 of a typical term, and a signed sum over rows may cancel down to one typical
  term, which is what the tensor's maximum is made of.  A gradient passes through at most L + 2 quantised products (out,
  L GLU layers, the encoder) and their errors add at worst.  Bound: (L + 2) sqrt(128) 2^-11 of the tensor's maximum,
  1.7e-2 for L = 1 and 2.2e-2 for L = 2."""
  tol = (L + 2) * math.sqrt(128) * 2.0 ** -11
  case = cc.Case("rounded", L, S, P, G, 333, seed=11 + P)
  params, args = cc.make_model(case).state_dict(), cc.inputs(case)
  got = cc.contract(case, params, args, torch.float64, round16=True)
  errs = _rel(got, _autograd(case, params, args, True))
  print(case.id, {k: f"{e:.1e}" for k, e in errs.items()})
  for k, e in errs.items():
    assert e <= tol, (case.id, k, e, tol)
  assert max(errs.values()) > 1e-6          # the rounding of dy is there


def test_dy_scale():
  dy = torch.zeros(40, 3)
  dy[0, 1], dy[3, 2] = 3e-7, -1e-9                    # tile 0
  dy[20, 0] = float("inf")                            # tile 1: not finite
  dy[32, 0], dy[39, 2] = 1e-45, 5.0                   # tile 2, the partial last one
  s = cmo.dy_scale(dy)
  assert s.shape == (40, 1)
  assert (s[:16] == s[0]).all() and 2.0 ** 14 <= 3e-7 * s[0].item() < 2.0 ** 15
  assert (s[16:32] == 1).all()
  assert (s[32:] == 2.0 ** 12).all()                  # 5 = 0.625 x 2^3
  assert cmo.dy_scale(torch.zeros(5, 2)).eq(1).all()
  assert cmo.dy_scale(torch.full((1, 1), 1e-45)).item() == 2.0 ** 120        # exponent clamp
  assert cmo.dy_scale(torch.full((1, 1), 1e38)).item() == 2.0 ** (15 - 127)
  # 64-row scale of the sensitivity test
  assert (cmo.dy_scale(dy, 64)[:16] == 1).all()


def test_noise_table():
  """NOISE is what the contract model's float32 run measures against its float64 run on the GPU tests' inputs.  The
  committed figures are that measurement rounded up; a CPU whose BLAS sums in another order moves single entries, so the
  re-measurement may exceed a figure by up to 2x before this fails, and MARGIN is not spent on that."""
  measured = cc.measure_noise()
  assert set(measured) == set(cc.NOISE), set(measured) ^ set(cc.NOISE)
  for cls, (e, where) in sorted(measured.items()):
    print(f"{cls:30s} measured {e:.2e} ({where})  table {cc.NOISE[cls]:.1e}  bound {cc.bound(cls):.1e}")
    assert e <= 2 * cc.NOISE[cls], (cls, e, where)
    assert cc.bound(cls) <= 3e-3                      # an order of magnitude under 3e-2
    assert 2.5 * cc.NOISE[cls] <= cc.bound(cls) <= 4 * cc.NOISE[cls]


def _outside(case, perturb):
  """[(figure / bound, class)] of the perturbed fp64 contract model against the unperturbed one, largest first."""
  params, args = cc.make_model(case).state_dict(), cc.inputs(case)
  ref = cc.contract(case, params, args, torch.float64)
  try:
    figs = cc.figures(case, cc.contract(case, params, args, torch.float64, perturb=(perturb,)), ref)
  except AssertionError as e:                         # an exact zero was missed
    return [(float("inf"), str(e.args[0][:2]))]
  return sorted(((e / cc.bound(cls), cls) for cls, e in figs), reverse=True)


MIXED_BOTH = [c for c in cc.MIXED if c.sides == "both"]


# scale64 is invisible where the rows of a step are alike: f16 rounding of a normal number does not depend on the power
# of two in front of it, so a 64-row scale only differs once a tile lies 2^-29 or more under its step's maximum.  The
# mixed-magnitude case has such a tile (MIXED_LONE_ROW).  Unrounded dy moves every entry by 2^-12 or so, which the maxima
# hardly see next to single neighbouring-f16 entries (at most 2.6x a bound, 1.4x on the mixed cases): detecting it rests
# on the median of d_point_features alone (390x its bound), on the uniform rows of the class-default case.
# dw_col_leak lands furthest out on the per-column figures (40x to 890x against 8x to 130x entrywise): those are the
# figures that see one column of a first-layer dW go wrong.
@pytest.mark.parametrize("perturb,cases,least", [
    ("scale64", MIXED_BOTH, 50.0),
    ("no_dy_rounding", [cc.CLASS_DEFAULT], 100.0),
    ("pad_leak", [cc.CLASS_DEFAULT] + MIXED_BOTH, 5.0),
    ("dw_col_leak", [cc.CLASS_DEFAULT] + MIXED_BOTH, 30.0),
    ("bias_drop_tail", [cc.CLASS_DEFAULT] + MIXED_BOTH, 5.0)])
def test_sensitivity(perturb, cases, least):
  """Each planted deviation of the model lands outside the GPU tolerance, by the stated factor at least, on the GPU
  tests' own inputs: a kernel that made the same mistake would fail tests/test_gpu_color_model_contract.py."""
  for case in cases:
    worst = _outside(case, perturb)
    print(perturb, case.id, [(f"{r:.1f}x", c) for r, c in worst[:3]])
    assert worst[0][0] > least, (perturb, case.id, worst[:3])


def test_unknown_perturbation_raises():
  case = cc.Case("x", 1, 2, 2, 2, 4)
  with pytest.raises(ValueError):
    cc.contract(case, cc.make_model(case).state_dict(), cc.inputs(case), torch.float64, perturb=("typo",))


def test_dynamic_range_of_the_tile_scale():
  """DESIGN.md "Colour model" quotes this: a row 2^-24 of its tile's largest keeps the accuracy of a full-size row (the
  f16 operand noise, 1e-3 of the row); from 2^-27 on bits are lost and past 2^-40 the row is flushed."""
  rows = cc.dynamic_range()
  full = rows[0][1]
  for j, med, worst in rows:
    if j <= 24:
      assert med < 2 * full and worst < 4e-3, (j, med, worst)
    if j >= 41:
      assert med == 1.0, (j, med)


def test_cases_reach_every_instantiation():
  reached = {(c.L, c.KF, c.S) for c in cc.GRID}
  assert reached == {(L, KF, S) for L in (1, 2) for KF in (1, 2) for S in (2, 3, 4, 5)}
  assert {c.F for c in cc.GRID if c.KF == 1} == {1, 5, 16, 31, 32} and {c.F for c in cc.GRID if c.KF == 2} == {33, 48, 63, 64}
  assert len({c.id for c in cc.CASES}) == len(cc.CASES)


if __name__ == "__main__":
  print("float32 contract model against the float64 contract model, worst over", len(cc.CASES), "cases")
  print(f"{'tensor class':30s} {'measured':>9s}  {'bound':>8s}  worst case")
  for cls, (e, where) in sorted(cc.measure_noise().items()):
    print(f"{cls:30s} {e:9.2e}  {cc.bound(cls):8.1e}  {where}")
  print()
  print("perturbed contract model against the contract model (fp64): figure / bound, three largest")
  for perturb in cmo.PERTURBATIONS:
    for case in [cc.CLASS_DEFAULT] + MIXED_BOTH:
      print(f"{perturb:15s} {case.id:34s}", ", ".join(f"{c} {r:.3g}x" for r, c in _outside(case, perturb)[:3]))
  print()
  print("contract model against plain fp64, d_point_features per row relative to the row's maximum; 15 rows per tile at")
  print("2^-j of the tile's full-size row (class-default shape)")
  print(f"{'j':>3s} {'median':>9s} {'worst':>9s}")
  for j, med, worst in cc.dynamic_range():
    print(f"{j:3d} {med:9.2e} {worst:9.2e}")
