"""The edges the shared host rules touch on the device.  Empty rows in the modules whose pointer rule became
``_lib.ptr`` (reg, color_model, optim, neighbours -- the last refuses an empty cloud in Python): an empty tensor now
arrives as NULL whether it is a fresh ``torch.empty(0)`` or a view ``x[:0]`` of a tensor with rows, and the native
wrappers return for M = 0 before they look at a pointer (csrc/reg.hip: reg_args_ok; csrc/color_model.hip:
gsr_color_forward / _backward test the row pointers under ``M > 0`` only; ``ParameterClass.step`` returns in Python).  And
the one alignment rule (``f32(align16=True)``) of the 3-D smoothing filter, on rows that start 4 bytes off."""
import pytest
import torch

import splat_trainer_amd as sta
from splat_trainer_amd import _lib, optim

pytestmark = pytest.mark.gpu

EMPTY = ["fresh", "view"]


def empty(kind, *row, dtype=torch.float32):
  """No rows of shape ``row``: a fresh tensor, or the first no rows of a tensor that has some."""
  if kind == "fresh":
    return torch.empty(0, *row, dtype=dtype, device="cuda")
  full = torch.ones(4, *row, dtype=dtype, device="cuda")
  view = full[:0]
  assert view.numel() == 0 and view.untyped_storage().data_ptr() == full.data_ptr() != 0
  return view


@pytest.mark.parametrize("kind", EMPTY)
def test_reg_loss_of_no_rows(kind):
  points = sta.RenderedPoints(idx=empty(kind, dtype=torch.int64), depths=empty(kind, 1),
                              opacity=empty(kind).requires_grad_(True), screen_scale=empty(kind, 2),
                              visibility=empty(kind), prune_cost=empty(kind), split_score=empty(kind),
                              attributes=sta.Colors(empty(kind, 3), empty(kind, 3)))
  log_scaling = torch.randn(8, 3, device="cuda", requires_grad=True)
  weights = dict(scale=1.0, opacity=1.0, aspect=1.0, specular=1.0)
  loss, terms = sta.reg_loss(points, log_scaling, weights, return_terms=True)
  assert loss.shape == () and float(loss.detach()) == 0.0 and terms.shape == (5,) and float(terms[4]) == 0.0     # no visible row
  loss.backward()
  assert log_scaling.grad.shape == (8, 3) and not log_scaling.grad.any()
  assert points.opacity.grad is None or points.opacity.grad.shape == (0,)


@pytest.mark.parametrize("kind", EMPTY)
def test_color_model_of_no_points(kind):
  torch.manual_seed(0)
  model = sta.ColorModel(sta.ColorModelConfig(hidden_layers=1, sh_degree=2), glo_features=4, point_features=4).cuda()
  features = empty(kind, 4).requires_grad_(True)
  glo = torch.randn(1, 4, device="cuda", requires_grad=True)
  colors = model(features, empty(kind, 3), torch.tensor([0.0, 0.0, 2.0], device="cuda"), glo)
  assert colors.diffuse.shape == (0, 3) and colors.specular.shape == (0, 3)
  assert colors.diffuse.dtype is torch.float32 and colors.diffuse.device.type == "cuda"
  (colors.diffuse.sum() + colors.specular.sum()).backward()
  grads = [p.grad for p in model.parameters() if p.requires_grad]
  assert grads and all(g is not None and g.shape == p.shape for g, p in zip(grads, model.parameters()))
  assert not any(bool(g.any()) for g in grads) and not glo.grad.any()
  assert features.grad is None or features.grad.shape == (0, 4)


@pytest.mark.parametrize("kind", EMPTY)
@pytest.mark.parametrize("optimizer", [optim.SparseAdam, optim.VisibilityAwareLaProp])
def test_optimizer_step_on_no_rows(kind, optimizer):
  torch.manual_seed(1)
  tensors = dict(position=torch.randn(8, 3, device="cuda"), alpha_logit=torch.randn(8, 1, device="cuda"))
  points = optim.ParameterClass(tensors, dict(position=dict(lr=0.1, type=optim.LOCAL_VECTOR), alpha_logit=dict(lr=0.1)),
                                optimizer=optimizer)
  for name in tensors:
    points.tensors[name].grad = torch.ones_like(points.tensors[name])
  snapshot = lambda: ([t.detach().clone() for t in points.tensors.values()] +
                      [points._state["step"].clone(), points._state["vis_avg"].clone()] +
                      [v.clone() for g in points._state["groups"].values() for v in g.values()])
  before = snapshot()
  points.step(empty(kind, dtype=torch.int64), visibility=empty(kind), basis=empty(kind, 3, 3))
  torch.cuda.synchronize()
  after = snapshot()
  assert len(before) == len(after) == 8 and all(torch.equal(a, b) for a, b in zip(before, after))
  assert optim.point_basis_rows(tensors["position"], torch.randn(8, 4, device="cuda"),
                                empty(kind, dtype=torch.int64)).shape == (0, 3, 3)


def test_filter_on_rows_that_start_off_alignment():
  """N = 5 rows sliced to start 4 bytes into their buffers against the same rows in aligned tensors: the kernels move
  four floats at a time, the rule copies what does not start on 16 bytes, and nothing but the address differs."""
  torch.manual_seed(2)
  N = 5

  def off(*shape):
    n = 1
    for d in shape:
      n *= d
    buffer = torch.randn(n + 4, device="cuda")
    view = buffer[1:n + 1].view(*shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view

  def run(ls, a, rate, g_ls, g_a):
    ls, a = ls.detach().requires_grad_(True), a.detach().requires_grad_(True)
    g = sta.Gaussians3D(position=torch.zeros(N, 3, device="cuda"), rotation=torch.zeros(N, 4, device="cuda"),
                        log_scaling=ls, alpha_logit=a, feature=torch.zeros(N, 3, device="cuda"))
    out = sta.smooth_gaussians(g, rate, 0.2)
    torch.autograd.backward([out.log_scaling, out.alpha_logit], [g_ls, g_a])
    return out.log_scaling.detach(), out.alpha_logit.detach(), ls.grad, a.grad

  views = off(N, 3), off(N, 1), off(N).abs() + 0.5, off(N, 3), off(N, 1)
  views = views[:2] + (off(N).copy_(views[2]),) + views[3:]            # (abs() made an aligned tensor: move it back off)
  assert all(v.data_ptr() % 16 == 4 for v in views)
  copies = tuple(v.clone() for v in views)
  assert all(c.data_ptr() % 16 == 0 for c in copies)
  for got, want in zip(run(*views), run(*copies)):
    assert got.shape == want.shape and torch.equal(got, want)
    assert bool(got.isfinite().all()) and bool(got.any())


def test_on_device_hands_out_the_current_stream():
  device = torch.device("cuda", torch.cuda.current_device())
  with _lib.on_device(device) as stream:
    assert stream == _lib.current_stream_ptr() == torch.cuda.current_stream().cuda_stream
  side = torch.cuda.Stream()
  with torch.cuda.stream(side), _lib.on_device(device) as stream:
    assert stream == side.cuda_stream != 0
  assert torch.cuda.current_device() == device.index
