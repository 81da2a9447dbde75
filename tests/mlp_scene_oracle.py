"""fp64 torch restatement of the scene regulariser: ``MLPScene.compute_reg`` and the masking of ``reg_loss``
(splat_trainer/scene/mlp_scene.py:246-288), written from the formulas.  Test infrastructure only."""
import torch

TERMS = ("scale", "opacity", "aspect", "specular")


def saturate(t, gain=4.0, k=2.0):                      # util/misc.py:68-69; pinned by tests/golden/misc_vectors.json
  return (1 - 1 / torch.exp(gain * t)).pow(k)


def compute_reg(opacity, log_scale, depths, specular, weight):
  """The four unweighted terms over the rows handed in (already the visible ones)."""
  scale = torch.exp(log_scale)
  norm_scale = scale.pow(2).sum(1) / depths.pow(2).squeeze(-1)
  aspect_term = scale.max(1).values / scale.min(1).values
  opacity_term = saturate(opacity, gain=4.0, k=2.0) * norm_scale
  spec_term = specular.abs().sum(1) if specular is not None else torch.zeros_like(norm_scale)
  return dict(scale=(norm_scale * weight).mean(), opacity=(opacity_term * weight).mean(),
              aspect=(aspect_term * weight).mean(), specular=(spec_term * weight).mean())


def reg_loss(idx, opacity, depths, specular, visibility, log_scaling, weights, visibility_weighted=True):
  """-> (loss, terms dict, count): rows with visibility > 0 only; no such row gives zeros (the native convention; the
  reference's mean over nothing is NaN).  ``visibility`` is a constant.  A term with a missing or zero weight is dropped."""
  rows = (visibility > 0).nonzero().squeeze(1)
  count = int(rows.shape[0])
  zero = (opacity.sum() + depths.sum() + log_scaling.sum()) * 0
  if count == 0:
    return zero, {k: zero for k in TERMS}, 0
  vis = visibility.detach()[rows]
  w = vis if visibility_weighted else torch.ones_like(vis)
  terms = compute_reg(opacity[rows], log_scaling[idx[rows]], depths[rows], None if specular is None else specular[rows], w)
  loss = zero
  for k in TERMS:
    if weights.get(k, 0.0) != 0.0:
      loss = loss + weights[k] * terms[k]
  return loss, terms, count
