"""csrc/optim.hip through ParameterClass.step against oracle/optim_oracle.py in fp64, ONE step from a given state, every
figure per row (optim_contract.py: cases, figures, bounds = 4 x the float32 oracle's own noise, at most 1e-4;
tests/test_optim_contract_host.py measures the noise and shows that the figures discriminate).

All 11 kernel instantiations run under both algorithms in every test that steps optim_contract.GROUPS: narrow scalar and
vector at D = 1..4, narrow local_vector, wide scalar and wide vector at D in {5, 15, 16, 17, 32, 33, 48, 64} and at the
(3, 16) and (3, 9) feature shapes.  Every figure is printed next to its bound and goes into the run's parity table.
"""
import pytest
import torch

import helpers
import optim_contract as oc
from splat_trainer_amd import optim

pytestmark = pytest.mark.gpu

OPTIMIZERS = {(True, "laprop"): optim.VisibilityAwareLaProp, (True, "adam"): optim.VisibilityAwareAdam,
              (False, "laprop"): optim.SparseLaProp, (False, "adam"): optim.SparseAdam}
# one group per kernel family, odd and even tails
FEW = tuple(oc.BY_NAME[n] for n in ("scalar1", "vector3", "local3", "scalar17", "vector32", "vector3x9"))


def _class(case):
  v = case.variant
  pc = optim.ParameterClass({k: t.cuda() for k, t in case.tensors.items()},
                            {g.name: dict(lr=g.lr, type=g.kind) for g in case.groups},
                            optimizer=OPTIMIZERS[(v.visibility, case.algo)],
                            state=oc.clone_state(case.state, device="cuda"), **v.options())
  return pc


def _native(case, idx, without_grad=(), grad_view=False):
  """One step of the kernels from the case's state: dict(tensors, state) on the CPU."""
  pc = _class(case)
  for g in case.groups:
    if g.name in without_grad:
      continue
    p, grad = pc.tensors[g.name], case.grads[g.name].cuda()
    if grad_view:                                       # every second row of a taller tensor: not contiguous
      tall = torch.zeros((2 * oc.N,) + g.shape, device="cuda", dtype=grad.dtype)
      tall[::2] = grad
      grad = tall[::2]
      assert not grad.is_contiguous()
    if grad.dtype != p.dtype:
      p.grad_dtype = None                               # a gradient of another dtype than its parameter
    p.grad = grad
    assert p.grad.dtype == case.variant.grad_dtype and p.grad.is_contiguous() != grad_view
  if idx.numel():
    kw = dict(visibility=case.visibility[idx].cuda()) if case.variant.visibility else {}
    pc.step(indexes=idx.cuda(), basis=case.basis[idx].cuda(), **kw)
  else:
    pc.step(indexes=idx.cuda(), visibility=torch.zeros(0, device="cuda"), basis=torch.zeros(0, 3, 3, device="cuda"))
  torch.cuda.synchronize()
  return dict(tensors={k: pc.tensors[k].detach().cpu() for k in case.tensors}, state=oc.clone_state(pc._state, device="cpu"))


def _check(label, case, idx, got, without_grad=()):
  ref = oc.oracle_step(case, idx, without_grad=without_grad)
  figs = oc.figures(case, idx, got, ref)
  worst = {}
  for (group, figure), e in figs.items():
    b = oc.bound(case, group, figure)
    share = e / b if b > 0 else (0.0 if e == 0 else float("inf"))
    print(f"CONTRACT {label} {group or '-'} {figure}: {e:.3e} (bound {b:.1e}, {share:.2f} of it)")
    kind = oc.BY_NAME[group].kind if group else "rows"
    if share >= worst.get((kind, figure), (-1.0,))[0]:
      worst[(kind, figure)] = (share, e, b)
  for (kind, figure), (share, e, b) in worst.items():   # the worst of each type into the parity table
    helpers.observe(label, f"{kind}/{figure}", torch.tensor([1.0 + min(e, 1e30)], dtype=torch.float64),
                    torch.ones(1, dtype=torch.float64), max(b, 1e-30))
  bad = oc.outside(case, figs)
  assert not bad, (label, bad[:8])
  return ref


def _bits_equal(a, b):
  for k in a["tensors"]:
    assert torch.equal(a["tensors"][k], b["tensors"][k]), k
    for n in ("exp_avg", "exp_avg_sq"):
      assert torch.equal(a["state"]["groups"][k][n], b["state"]["groups"][k][n]), (k, n)
  assert torch.equal(a["state"]["step"], b["state"]["step"]) and torch.equal(a["state"]["vis_avg"], b["state"]["vis_avg"])


@pytest.mark.parametrize("algo", oc.ALGOS)
@pytest.mark.parametrize("variant", [oc.REFERENCE, oc.STRESS], ids=lambda v: v.name)
def test_every_instantiation(variant, algo):
  """The reference's hyper-parameters and the set where 1 - beta^t cancels; clocks 0 to 4e5, row scales 2^-40 to 2^30,
  visibility down to 1e-6, every 11th row unseen."""
  case = oc.make_case(variant, algo, 0)
  assert {oc.instantiation(g) for g in case.groups} >= {"wide<scalar>", "wide<vector>", "narrow<3,local_vector>"}
  idx = oc.indexes(case)
  _check(case.id, case, idx, _native(case, idx))


@pytest.mark.parametrize("variant,algo", [(v, a) for v in (oc.NO_BIAS_CORRECTION, oc.NO_CLIP, oc.CLIP_HALF, oc.NO_VISIBILITY)
                                          for a in v.algos], ids=lambda x: getattr(x, "name", x))
def test_option_variants(variant, algo):
  """bias_correction=False; LaProp without a clip; a clip of 0.5 that takes hold of most entries; SparseAdam and
  SparseLaProp, which leave vis_avg bit-identical (the vis_avg figure of a variant without visibility)."""
  case = oc.make_case(variant, algo, 0)
  idx = oc.indexes(case)
  ref = _check(case.id, case, idx, _native(case, idx))
  if variant is oc.CLIP_HALF:
    clipped = torch.cat([(t["momentum_in"].abs() == 0.5).flatten() for t in ref["terms"].values()])
    assert clipped.double().mean() > 0.5, clipped.double().mean()


@pytest.mark.parametrize("M", [1, 15, 16, 17, 255, 256, 257])
def test_sizes_of_M(M):
  """One row, and the edges of a 16-row wide block and of a 256-thread narrow block; the rows left out stay bit-identical
  (the unseen figure)."""
  for algo in oc.ALGOS:
    case = oc.make_case(oc.REFERENCE, algo, 1, groups=FEW)
    idx = oc.indexes(case, "permuted", M)
    assert idx.numel() == M
    _check(f"{case.id}-M{M}", case, idx, _native(case, idx))


def test_every_row_and_no_row():
  case = oc.make_case(oc.ALL_VISIBLE, "laprop", 0)
  idx = oc.indexes(case)
  assert idx.numel() == oc.N
  _check(case.id, case, idx, _native(case, idx))
  case = oc.make_case(oc.REFERENCE, "adam", 0, groups=FEW)
  none = torch.zeros(0, dtype=torch.int64)
  got = _native(case, none)                          # M = 0: nothing moves
  _bits_equal(got, dict(tensors=case.tensors, state=case.state))


@pytest.mark.parametrize("algo", oc.ALGOS)
def test_permuted_indexes(algo):
  """Rows are independent: a permutation of the indexes meets the bounds, gives the bits of the ascending call, and a
  second run gives them again."""
  case = oc.make_case(oc.STRESS, algo, 2)
  asc, perm = oc.indexes(case), oc.indexes(case, "permuted")
  a = _native(case, asc)
  b = _native(case, perm)
  _check(f"{case.id}-permuted", case, perm, b)
  _bits_equal(a, b)
  _bits_equal(b, _native(case, perm))


def test_group_without_gradient():
  """.grad None: the group's parameter and moments stay, the clock and vis_avg advance, the other groups are stepped."""
  case = oc.make_case(oc.REFERENCE, "laprop", 3, groups=FEW)
  idx = oc.indexes(case)
  skipped = ("vector3", "scalar17")
  got = _native(case, idx, without_grad=skipped)
  _check(f"{case.id}-nograd", case, idx, got, without_grad=skipped)
  for k in skipped:
    assert torch.equal(got["tensors"][k], case.tensors[k])
    assert torch.equal(got["state"]["groups"][k]["exp_avg_sq"], case.state["groups"][k]["exp_avg_sq"])
  assert torch.equal(got["state"]["step"][idx], case.state["step"][idx] + 1)
  assert (got["state"]["vis_avg"][idx] != case.state["vis_avg"][idx]).any()


@pytest.mark.parametrize("algo", oc.ALGOS)
def test_gradient_call_forms(algo):
  """A gradient held as a non-contiguous view, and one held in float16 (the oracle is fed the float16 values)."""
  case = oc.make_case(oc.REFERENCE, algo, 4, groups=FEW)
  idx = oc.indexes(case)
  _check(f"{case.id}-view", case, idx, _native(case, idx, grad_view=True))
  case = oc.make_case(oc.F16_GRAD, algo, 0)
  idx = oc.indexes(case)
  _check(case.id, case, idx, _native(case, idx))


def test_point_basis_rows_per_row():
  """optim.point_basis_rows against harness.point_basis in fp64, per row relative to the row's largest entry: log scales
  from -20 to 10, quaternions of any length, a zero quaternion; all rows, a permuted subset, and one row."""
  ls, rot = oc.basis_inputs(0)
  gen = torch.Generator().manual_seed(9)
  some = torch.randperm(oc.BASIS_ROWS, generator=gen)[:300]
  for label, rows in (("all", None), ("permuted", some), ("one", torch.tensor([5])), ("last", torch.tensor([oc.BASIS_ROWS - 1]))):
    got = optim.point_basis_rows(ls.cuda(), rot.cuda(), None if rows is None else rows.cuda())
    sel = slice(None) if rows is None else rows
    e = oc.basis_figure(got, ls[sel], rot[sel])
    print(f"CONTRACT point_basis-{label} - basis/row: {e:.3e} (bound {oc.BASIS_BOUND:.1e}, {e / oc.BASIS_BOUND:.2f} of it)")
    helpers.observe(f"point_basis-{label}", "basis/row", torch.tensor([1.0 + e], dtype=torch.float64),
                    torch.ones(1, dtype=torch.float64), oc.BASIS_BOUND)
    assert e <= oc.BASIS_BOUND, (label, e)
  one = optim.point_basis_rows(ls.cuda(), rot.cuda(), torch.tensor([5]).cuda()).cpu()[0]
  assert torch.equal(one, torch.diag(one.diag())) and (one.diag() > 0).all()         # the zero quaternion: R = identity
