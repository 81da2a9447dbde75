"""The colour model's HIP kernels (csrc/color_model.hip) against the contract model in fp64 (color_model_oracle.forward
and .backward with round16=True: the kernels' own rounding decisions restated on the CPU), on every template
instantiation and at the edges of the shapes, row counts, magnitudes and geometry.  Cases, figures and bounds live in
color_model_contract.py; the bounds are the contract model's measured float32 noise times a stated margin
(tests/test_color_model_contract_host.py measures it and shows that the comparison discriminates).

Each case id names its instantiation: L<hidden_layers>KF<feature blocks of 32>S<sh_degree>.  Every figure goes through
helpers.observe into the run's parity table.
"""
import pytest
import torch

import color_model_contract as cc
import color_model_oracle as cmo
import helpers

pytestmark = pytest.mark.gpu


def _native(case, model, args, pf_view=False):
  pf, pos, cam, glo, dd, ds = args
  model.zero_grad(set_to_none=True)
  if pf_view:                                         # every second column of a wider tensor: not contiguous
    wide = torch.zeros(pf.shape[0], 2 * pf.shape[1])
    wide[:, ::2] = pf
    leaf = wide.cuda().requires_grad_(True)
    x = leaf[:, ::2]
    assert not x.is_contiguous()
  else:
    leaf = x = pf.cuda().requires_grad_(True)
  cp = cam.cuda().requires_grad_(case.cam_grad)
  g = glo.cuda().requires_grad_(True)
  col = model(x, pos.cuda(), cp, g)
  loss = 0
  if dd is not None:
    loss = loss + (col.diffuse * dd.cuda()).sum()
  if ds is not None:
    loss = loss + (col.specular * ds.cuda()).sum()
  loss.backward()
  torch.cuda.synchronize()
  d_pf = leaf.grad
  if pf_view:
    assert d_pf.shape == leaf.shape and not d_pf[:, 1::2].any()      # arrives in the caller's tensor, only where it reads
    d_pf = d_pf[:, ::2]
  if d_pf is None and not x.numel():                  # P = 0 or G = 0: autograd may leave an empty leaf without a gradient
    d_pf = torch.zeros_like(x)
  d_glo = g.grad if g.grad is not None or g.numel() else torch.zeros_like(g)
  out = dict(point_features=d_pf, glo=d_glo, cam_pos=cp.grad if case.cam_grad else None)
  for k, p in model.named_parameters():
    assert p.grad is not None and p.grad.shape == p.shape, k
    out[k] = p.grad
  return (col.diffuse.detach(), col.specular.detach()), out


def _logged(label, cls, figure):
  """A derived figure (per column, per row, median) into the parity table, as an error of `figure` on a unit value."""
  helpers.observe(label, cls, torch.tensor([1.0 + figure], dtype=torch.float64), torch.ones(1, dtype=torch.float64),
                  cc.bound(cls))


def _compare(case, model, args, native):
  colours, got = native
  params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
  pf, pos, cam, glo, dd, ds = (None if t is None else t.double() for t in args)
  # forward: the bounds of tests/test_gpu_color_model.py::test_forward_matches_rounded_oracle
  with torch.no_grad():
    ref_colours = cmo.forward({k: v.double() for k, v in params.items()}, pf, pos, cam, glo, case.L, case.S, round16=True)
  for name, a, b in zip(("diffuse", "specular"), colours, ref_colours):
    worst, _ = helpers.observe(case.id, name, a, b, 8e-3)
    med = (a.cpu().double() - b).abs().median().item() / b.abs().max().item()
    helpers.observe(case.id, f"{name}/median", torch.tensor([1.0 + med], dtype=torch.float64),
                    torch.ones(1, dtype=torch.float64), 2e-6)
    assert med < 2e-6 and worst < 8e-3, (case.id, name, med, worst)
  ref = cc.contract(case, params, args, torch.float64)
  for key, r in ref.items():
    if r is not None and got[key] is not None and r.numel():        # P = 0 or G = 0: nothing to log
      helpers.observe(case.id, key, got[key], r, cc.bound(cc.tensor_class(key)))
  figs = cc.figures(case, got, ref)                   # asserts the exact zeros
  bad = []
  for cls, e in figs:
    if "/" in cls:
      _logged(case.id, cls, e)
    print(f"{case.id} {cls}: {e:.2e} (bound {cc.bound(cls):.1e})")
    if not e <= cc.bound(cls):
      bad.append((cls, e, cc.bound(cls)))
  assert not bad, (case.id, bad)


def _run(case, **kw):
  model = cc.make_model(case).cuda()
  args = cc.inputs(case)
  _compare(case, model, args, _native(case, model, args, **kw))


@pytest.mark.parametrize("case", cc.GRID, ids=lambda c: c.id)
def test_shape_grid(case):
  """All 16 (L, KF, S) instantiations; F in {1, 5, 16, 31, 32} and {33, 48, 63, 64}; P = 0, G = 0, P odd, (17, 16)."""
  _run(case)


def test_class_default():
  """ColorModel() as it is constructed without arguments: L = 2, S = 5, P = G = 16."""
  assert (cc.CLASS_DEFAULT.L, cc.CLASS_DEFAULT.S, cc.CLASS_DEFAULT.P, cc.CLASS_DEFAULT.G) == (2, 5, 16, 16)
  _run(cc.CLASS_DEFAULT)


@pytest.mark.parametrize("case", cc.ROWS, ids=lambda c: c.id)
def test_row_counts(case):
  _run(case)


@pytest.mark.parametrize("case", cc.MIXED, ids=lambda c: c.id)
def test_mixed_magnitudes_inside_a_wave(case):
  """Upstream rows times 10^U(-6, 0), one tile all zero, one tile with a single row 1e-12 of its neighbours: every row
  of d_point_features is right relative to its own size, the zero rows are exact zeros."""
  _run(case)


@pytest.mark.parametrize("case", cc.EXTREME, ids=lambda c: c.id)
def test_extreme_scales(case):
  """Upstream gradients times 1e-30 and 1e+30: nothing underflows on the way in or overflows on the way back.  The
  scale's exponent stays inside its +-120 clamp here (k is about 115 on the outer layers of the 1e-30 case); the clamp
  itself is pinned on the model only (test_dy_scale in tests/test_color_model_contract_host.py)."""
  _run(case)


@pytest.mark.parametrize("case", cc.EDGES, ids=lambda c: c.id)
def test_geometry_edges(case):
  """A point at the camera (the normalize clamp), rows along +-z and +-x, +-y; with and without a camera gradient."""
  _run(case)


@pytest.mark.parametrize("shape", [cc.DEFAULT, cc.WIDE], ids=["KF1", "KF2"])
def test_call_forms(shape):
  """A non-contiguous point_features view and parameters held as non-contiguous views: forward() makes contiguous
  copies, the gradients arrive in the caller's tensors with the caller's shapes."""
  case = cc.Case("call_forms", M=517, seed=6, **shape)
  model = cc.make_model(case).cuda()
  for lin in (model.base_model.layers[0].m, model.directional_model.encode_dir.mlp.layers[0]):
    w = lin.weight.detach()
    lin.weight = torch.nn.Parameter(w.t().contiguous().t())
    assert not lin.weight.is_contiguous() and torch.equal(lin.weight, w)
  args = cc.inputs(case)
  _compare(case, model, args, _native(case, model, args, pf_view=True))


@pytest.mark.parametrize("shape", [cc.DEFAULT, cc.WIDE], ids=["KF1", "KF2"])
def test_bit_reproducible(shape):
  case = cc.Case("repro", M=40_001, seed=8, **shape)       # 626 steps on 256 workgroups
  model = cc.make_model(case).cuda()
  args = cc.inputs(case)
  (d1, s1), a = _native(case, model, args)
  (d2, s2), b = _native(case, model, args)
  assert torch.equal(d1, d2) and torch.equal(s1, s2)
  for k in a:
    assert torch.equal(a[k], b[k]), k
