"""Host-side checks of the scene class and the regulariser (no GPU): the fp64 restatement against the golden ``saturate``
values and against finite differences, the config defaults against the reference's (mlp_scene.py:40-52), and the error
cases of ``reg_loss`` (there is no CPU fallback)."""
import json
import os

import pytest
import torch

import mlp_scene_oracle as mso
import splat_trainer_amd as sta
from splat_trainer_amd.reg import scene_post_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_reproduces_the_golden_saturate():
  d = json.load(open(os.path.join(ROOT, "tests", "golden", "misc_vectors.json")))
  t = torch.tensor(d["t"], dtype=torch.float32)
  got = mso.saturate(t, gain=4.0, k=2.0)
  assert torch.allclose(got, torch.tensor(d["saturate_gain4_k2"]), rtol=1e-6, atol=1e-7)


def _rows(M=7, N=11, seed=0):
  gen = torch.Generator().manual_seed(seed)
  idx = torch.randperm(N, generator=gen)[:M]
  opacity = torch.rand(M, generator=gen, dtype=torch.float64)
  depths = 1 + 4 * torch.rand(M, 1, generator=gen, dtype=torch.float64)
  specular = torch.randn(M, 3, generator=gen, dtype=torch.float64)
  visibility = torch.rand(M, generator=gen, dtype=torch.float64)
  visibility[::3] = 0
  log_scaling = torch.randn(N, 3, generator=gen, dtype=torch.float64) * 0.5
  return idx, opacity, depths, specular, visibility, log_scaling


@pytest.mark.parametrize("weighted", [True, False])
def test_restatement_gradcheck(weighted):
  idx, opacity, depths, specular, visibility, log_scaling = _rows()
  weights = dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5)

  def f(o, d, s, ls):
    return mso.reg_loss(idx, o, d, s, visibility, ls, weights, weighted)[0]

  args = [t.clone().requires_grad_(True) for t in (opacity, depths, specular, log_scaling)]
  assert torch.autograd.gradcheck(f, args)


def test_restatement_masks_and_drops():
  idx, opacity, depths, specular, visibility, log_scaling = _rows()
  loss, terms, count = mso.reg_loss(idx, opacity, depths, specular, visibility, log_scaling, dict(scale=1.0))
  assert count == int((visibility > 0).sum()) and torch.allclose(loss, terms["scale"])
  loss0, _, count0 = mso.reg_loss(idx, opacity, depths, specular, torch.zeros_like(visibility), log_scaling,
                                  dict(scale=1.0))
  assert count0 == 0 and loss0.item() == 0.0


def test_config_defaults_are_the_references():
  c = sta.MLPSceneConfig(parameters={}, reg_weight={})
  assert (c.lr_glo_feature, c.image_features, c.point_features) == (0.001, 8, 8)
  assert (c.beta1, c.beta2, c.vis_beta, c.vis_smooth, c.per_image, c.grad_clip) == (0.8, 0.9, 0.95, 0.001, True, 2.0)
  assert c.color_model == sta.ColorModelConfig()
  o = c.optim_options()
  assert o["betas"] == (0.8, 0.9) and o["bias_correction"] is True and o["grad_clip"] == 2.0
  assert o["optimizer"] is sta.optim.VisibilityAwareLaProp and o["vis_beta"] == 0.95 and o["vis_smooth"] == 0.001


def _points(M=5, N=9, **over):
  f = dict(idx=torch.arange(M), depths=torch.ones(M, 1), opacity=torch.rand(M), screen_scale=torch.ones(M, 2),
           visibility=torch.ones(M), prune_cost=torch.zeros(M), split_score=torch.zeros(M),
           attributes=sta.Colors(torch.zeros(M, 3), torch.zeros(M, 3)))
  f.update(over)
  return sta.RenderedPoints(**f), torch.zeros(N, 3)


def test_reg_loss_refuses_cpu_tensors():
  points, ls = _points()
  with pytest.raises(sta.GsplatHipError, match="no CPU fallback"):
    sta.reg_loss(points, ls, dict(scale=1.0))
  with pytest.raises(sta.GsplatHipError, match="no CPU fallback"):
    scene_post_step(torch.zeros(4, 4), torch.zeros(4, 3))


def test_reg_loss_argument_errors():
  points, ls = _points()
  with pytest.raises(ValueError, match="unknown regulariser term"):
    sta.reg_loss(points, ls, dict(scales=1.0))
  with pytest.raises(ValueError, match="log_scaling must be an"):
    sta.reg_loss(points, torch.zeros(9), dict(scale=1.0))
  with pytest.raises(ValueError, match=r"log_scaling must be \(9, 3\)"):
    sta.reg_loss(points, torch.zeros(9, 4), dict(scale=1.0))
  with pytest.raises(ValueError, match="points.idx must be"):
    sta.reg_loss(_points(idx=torch.zeros(5, 1, dtype=torch.int64))[0], ls, dict(scale=1.0))
  with pytest.raises(ValueError, match="points.idx must be torch.int64"):
    sta.reg_loss(_points(idx=torch.arange(5, dtype=torch.int32))[0], ls, dict(scale=1.0))
  with pytest.raises(ValueError, match="must be a torch.Tensor"):
    sta.reg_loss(_points(opacity=[0.0] * 5)[0], ls, dict(scale=1.0))
  with pytest.raises(ValueError, match="points.opacity must be torch.float32"):
    sta.reg_loss(_points(opacity=torch.rand(5, dtype=torch.float64))[0], ls, dict(scale=1.0))
  with pytest.raises(ValueError, match=r"points.depths must be \(5, 1\) or \(5,\)"):
    sta.reg_loss(_points(depths=torch.ones(5, 2))[0], ls, dict(scale=1.0))
  with pytest.raises(ValueError, match=r"points.visibility must be \(5,\)"):
    sta.reg_loss(_points(visibility=torch.ones(4))[0], ls, dict(scale=1.0))
  with pytest.raises(ValueError, match=r"points.attributes.specular must be \(5, 3\)"):
    sta.reg_loss(_points(attributes=sta.Colors(torch.zeros(5, 2), torch.zeros(5, 2)))[0], ls, dict(scale=1.0))
  with pytest.raises(ValueError, match=r"rotation must be \(4, 4\)"):
    scene_post_step(torch.zeros(4, 3), torch.zeros(4, 3))
