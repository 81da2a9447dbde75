"""The reference's scene class (``splat_trainer.scene.mlp_scene``: ``MLPSceneConfig``, ``MLPScene``) over this package's
native pieces: ``project_to_image`` / ``render_projected``, ``ColorModel``, ``ParameterClass`` with the visibility-aware
LaProp step, the native regulariser and post-step projection (reg.py), ``split_gaussians_uniform`` and
``keep_and_append``, ``evaluate_sh_at``.

What differs from the reference's surface, because the packages behind it are not here: no tensordict, hydra, beartype or
logger; a scene is told the number of images instead of being handed a camera table; ``parameters``, ``reg_weight`` and
the learning rates are plain floats -- the caller evaluates its schedules and passes the values to
``update_learning_rate``; ``to_sh_gaussians`` takes the cameras to fit against.  There is no autocast in ``render``: the
native colour model is fp32 outside and f16 MFMA inside.

Beyond the reference: ``MLPSceneConfig.filter_3d`` > 0 switches on Mip-Splatting's 3-D smoothing filter (filter3d.py).
``update_filter(cameras)`` stores every point's sampling rate as the unoptimised column ``filter_rate`` of ``points``
(as ``visible`` rides along), and ``render``, ``query_visibility`` and ``to_sh_gaussians`` then work on the smoothed
scales and opacities; ``gaussians`` and ``reg_loss`` stay on the raw parameters.  At 0, the default, none of it runs.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Dict, Iterable, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import reg
from .color_model import ColorModel, ColorModelConfig, Colors
from .filter3d import sampling_rate, smooth_gaussians
from .data_types import CameraParams, Gaussians3D, RasterConfig, Rendering, pop_raster_config
from .harness import split_gaussians_uniform
from .histogram import tensor_histogram
from .normals import geometry_features
from .optim import ParameterClass, VisibilityAwareLaProp, VisibilityOptimizer, point_basis_rows
from .renderer import project_to_image, render_projected
from .sh import evaluate_sh_at
from .sh_fit import DEFAULT_RIDGE, fit_sh

SH_C0 = 0.282094791773878


class GLOTable(nn.Module):
  """scene/color_model.py:11-45: one embedding per image, initialised to zero."""

  def __init__(self, n: int, glo_features: int):
    super().__init__()
    self.embeddings = nn.Embedding(n, glo_features)
    nn.init.zeros_(self.embeddings.weight)

  @property
  def weight(self) -> torch.Tensor:
    return self.embeddings.weight

  def forward(self, idx):
    if isinstance(idx, int):
      return self.embeddings.weight[idx]
    return self.embeddings(idx)

  def optimizer(self, lr_glo: float) -> torch.optim.Optimizer:
    return torch.optim.Adam([dict(params=list(self.embeddings.parameters()), lr=float(lr_glo), name="glo")],
                            betas=(0.8, 0.95))


def _clone_tree(obj):
  if isinstance(obj, torch.Tensor):
    return obj.detach().clone()
  if isinstance(obj, dict):
    return {k: _clone_tree(v) for k, v in obj.items()}
  if isinstance(obj, (list, tuple)):
    return type(obj)(_clone_tree(v) for v in obj)
  return obj


@dataclass(frozen=True)
class MLPSceneConfig:
  """mlp_scene.py:34-93; defaults :40-52.  ``parameters``: {name: dict(lr=, type=)} for position, log_scaling, rotation,
  alpha_logit and feature (config/scene/mlp.yaml:6-14); ``reg_weight``: {scale, opacity, aspect, specular} (:16-20).
  ``filter_3d``: strength of the 3-D smoothing filter (Mip-Splatting uses 0.2); 0 = off."""
  parameters: Dict[str, dict]
  reg_weight: Dict[str, float]
  color_model: ColorModelConfig = field(default_factory=ColorModelConfig)
  lr_glo_feature: float = 0.001
  image_features: int = 8
  point_features: int = 8
  beta1: float = 0.8
  beta2: float = 0.9
  vis_beta: float = 0.95
  vis_smooth: float = 0.001
  per_image: bool = True
  grad_clip: Optional[float] = 2.0
  filter_3d: float = 0.0

  def optim_options(self) -> dict:
    """mlp_scene.py:58-60."""
    return dict(optimizer=VisibilityAwareLaProp, betas=(self.beta1, self.beta2), vis_beta=self.vis_beta,
                bias_correction=True, vis_smooth=self.vis_smooth, grad_clip=self.grad_clip)

  def from_color_gaussians(self, gaussians: Gaussians3D, num_images: int, device, seed: Optional[int] = None
                           ) -> "MLPScene":
    """mlp_scene.py:64-80: point features N(0, 5^2) replace the colours; ``visible`` rides along unoptimised."""
    n = int(gaussians.batch_size[0])
    gen = None if seed is None else torch.Generator().manual_seed(seed)
    feature = torch.empty(n, self.point_features).normal_(std=5.0, generator=gen)
    tensors = {k: v.detach().to(device=device, dtype=torch.float32) for k, v in gaussians.to_dict().items()}
    tensors["feature"] = feature.to(device)
    tensors["visible"] = torch.zeros(n, device=device)
    points = ParameterClass(tensors, parameter_groups=self.parameters, **self.optim_options())
    return MLPScene(points, self, num_images)

  def from_state_dict(self, state: dict, num_images: int) -> "MLPScene":
    """mlp_scene.py:83-93.  The tensors are copied: the new scene shares nothing with the one that made ``state``."""
    state = _clone_tree(state)
    points = ParameterClass.from_state_dict(state["points"], **self.optim_options())
    scene = MLPScene(points, self, num_images)
    scene.color_model.load_state_dict(state["color_model"])
    scene.color_table.load_state_dict(state["color_table"])
    scene.color_opt.load_state_dict(state["color_opt"])
    scene.glo_opt.load_state_dict(state["glo_opt"])
    return scene


class MLPScene:
  """mlp_scene.py:97-427."""

  def __init__(self, points: ParameterClass, config: MLPSceneConfig, num_images: int):
    self.config = config
    self.points = points
    self.num_images = int(num_images)
    # ColorModel checks its own limits (hidden_features = 32, 1 or 2 hidden layers, SH degree 2..5, <= 64 features)
    self.color_model = ColorModel(config=config.color_model, glo_features=config.image_features,
                                  point_features=config.point_features).to(self.device)
    self._color_model = self.color_model                   # (the reference keeps the uncompiled module under this name)
    self.color_opt = self.color_model.optimizer()
    self.color_table = GLOTable(self.num_images, config.image_features).to(self.device)
    self.glo_opt = self.color_table.optimizer(config.lr_glo_feature)
    self._training = [True] * self.num_images
    self.update_learning_rate(None, lr_color=dict(spec=config.color_model.lr_specular, base=config.color_model.lr_diffuse),
                              lr_glo=config.lr_glo_feature)

  @property
  def device(self):
    return self.points.position.device

  @property
  def num_points(self) -> int:
    return self.points.position.shape[0]

  def __repr__(self):
    return f"MLPScene({self.num_points} points)"

  def set_training_images(self, image_indexes: Iterable[int]):
    """The images whose GLO vector ``render`` looks up (the reference's ``Label.Training``, mlp_scene.py:355-357);
    every other index renders with a zero GLO vector.  Default: all."""
    chosen = set(int(i) for i in image_indexes)
    self._training = [i in chosen for i in range(self.num_images)]

  def update_learning_rate(self, groups: Optional[Dict[str, float]] = None, lr_color=None, lr_glo: Optional[float] = None
                           ) -> Dict[str, float]:
    """mlp_scene.py:142-153 with the schedules evaluated by the caller: ``groups`` = {point parameter: lr (or dict(lr=))},
    ``lr_color`` = one float for both colour groups or dict(spec=, base=), ``lr_glo`` = the GLO table's.  Returns every
    learning rate by name."""
    rates = dict(self.points.update_groups(**(groups or {})))
    if lr_color is not None:
      by_name = lr_color if isinstance(lr_color, dict) else dict(spec=lr_color, base=lr_color)
      for g in self.color_opt.param_groups:
        if g["name"] in by_name:
          g["lr"] = float(by_name[g["name"]])
    if lr_glo is not None:
      for g in self.glo_opt.param_groups:
        g["lr"] = float(lr_glo)
    rates.update({g["name"]: g["lr"] for g in self.color_opt.param_groups})
    rates.update({g["name"]: g["lr"] for g in self.glo_opt.param_groups})
    return rates

  @torch.no_grad()
  def zero_grad(self):
    """mlp_scene.py:155-161."""
    self.points.visible.zero_()
    self.points.zero_grad()
    self.color_opt.zero_grad()
    self.glo_opt.zero_grad()

  @torch.no_grad()
  def step(self):
    """mlp_scene.py:214-239: the sparse step on the rows the batch has seen, the colour and GLO steps, the projection
    (unit quaternions, log-scales in [-8, 8]: one native sweep) and ``zero_grad``, which also clears ``visible``."""
    pts = self.points
    vis_idx = pts.visible.nonzero().squeeze(1)             # (the step's one host wait: the row count sizes the step)
    basis = point_basis_rows(pts.log_scaling, pts.rotation, vis_idx)
    if isinstance(pts.optimizer, VisibilityOptimizer):
      pts.step(visibility=pts.visible[vis_idx], indexes=vis_idx, basis=basis)
    else:
      pts.step(indexes=vis_idx, basis=basis)
    self.color_opt.step()
    self.glo_opt.step()
    reg.scene_post_step(pts.rotation.data, pts.log_scaling.data)
    self.zero_grad()

  # ---- detailed logs (mlp_scene.py:163-211).  The scene holds no logger: each method is handed one.  Every histogram is
  # a Histogram built by tensor_histogram -- gather, weight and log10 fused into the native sweep, no boolean-mask
  # indexing, no host wait per histogram -- and none of them writes a parameter, a gradient or optimizer state.
  @torch.no_grad()
  def detail_histograms(self, what: str, min_vis: float = 0.1) -> Dict[str, "Histogram"]:
    """{name: Histogram} of one family of the detailed logs: ``"gradients"`` (log10 of the positive gradient entries of
    the rows whose accumulated visibility exceeds ``min_vis``, raw and divided by ``vis_smooth + visibility``),
    ``"optimizer"`` (log10 of the positive entries of the optimizer state) or ``"params"``."""
    pts, out = self.points, {}
    if what == "gradients":
      visible = pts.visible
      vis_idx = torch.nonzero(visible > min_vis).squeeze(1)          # (the one wait of a detailed log)
      for key in pts.parameter_groups:
        grad = pts.tensors[key].grad
        if grad is not None:
          out[f"log10_grad/{key}"] = tensor_histogram(grad, rows=vis_idx, log10="drop", min_value=1e-16)
          out[f"log10_norm_grad/{key}"] = tensor_histogram(grad, rows=vis_idx, weight=visible, eps=self.config.vis_smooth,
                                                           log10="drop", min_value=1e-16)
    elif what == "optimizer":
      for key, state in pts.tensor_state.items():
        for k, v in state.items():
          out[f"{key}/{k}"] = tensor_histogram(v, log10="drop", min_value=1e-16)
    elif what == "params":
      out["params/opacity"] = tensor_histogram(torch.sigmoid(pts.alpha_logit.detach()))
      out["params/log_scale"] = tensor_histogram(pts.log_scaling)
      out["params/feature"] = tensor_histogram(pts.feature)
      out["params/glo_feature"] = tensor_histogram(self.color_table.weight)
      scale = torch.exp(pts.log_scaling.detach())
      largest = scale.max(1).values
      out["params/stable_rank"] = tensor_histogram(scale.sum(1) / largest)
      out["params/aspect"] = tensor_histogram(largest / (scale.min(1).values + 1e-4))
    else:
      raise ValueError(f"what must be 'gradients', 'optimizer' or 'params', got {what!r}")
    return out

  def log_gradients(self, logger, min_vis: float = 0.1):
    """mlp_scene.py:167-178; call it before ``step``, which clears the gradients and ``visible``."""
    for name, hist in self.detail_histograms("gradients", min_vis).items():
      logger.log_histogram(name, hist)

  def log_optimizer_state(self, logger, name: str = "optimizer"):
    """mlp_scene.py:180-187."""
    for key, hist in self.detail_histograms("optimizer").items():
      logger.log_histogram(f"{name}/{key}", hist)

  def log_params(self, logger):
    """mlp_scene.py:190-206."""
    for name, hist in self.detail_histograms("params").items():
      logger.log_histogram(name, hist)

  def log_checkpoint(self, logger, progress=None):
    """mlp_scene.py:210-211."""
    self.log_params(logger)

  @torch.no_grad()
  def add_rendering(self, image_idx: Optional[int], rendering: Rendering):
    """mlp_scene.py:241-244."""
    points = rendering.points
    self.points.visible.index_add_(0, points.idx, points.visibility)

  def reg_loss(self, rendering: Rendering, weights: Optional[Dict[str, float]] = None, return_terms: bool = False):
    """mlp_scene.py:268-288 through the native regulariser (reg.reg_loss): no ``points.visible``, no host wait.
    ``weights``: this step's values of the schedules; default ``config.reg_weight``."""
    return reg.reg_loss(rendering.points, self.points.log_scaling,
                        self.config.reg_weight if weights is None else weights,
                        visibility_weighted=isinstance(self.points.optimizer, VisibilityOptimizer),
                        return_terms=return_terms)

  @torch.no_grad()
  def split_and_prune(self, keep_mask: torch.Tensor, split_idx: Optional[torch.Tensor] = None,
                      generator: Optional[torch.Generator] = None):
    """mlp_scene.py:301-310: two children per row of ``split_idx`` appended behind the rows ``keep_mask`` keeps."""
    if split_idx is None:
      self.points = self.points[keep_mask]
      return
    splits = split_gaussians_uniform(self.points[split_idx].detach(), k=2, random_axis=True, generator=generator)
    self.points = self.points.keep_and_append(keep_mask, splits)

  def state_dict(self) -> dict:
    """mlp_scene.py:316-322."""
    return dict(points=self.points.state_dict(), color_model=self.color_model.state_dict(),
                color_opt=self.color_opt.state_dict(), color_table=self.color_table.state_dict(),
                glo_opt=self.glo_opt.state_dict())

  def clone(self) -> "MLPScene":
    scene = self.config.from_state_dict(self.state_dict(), self.num_images)
    scene._training = list(self._training)
    return scene

  def lookup_glo_feature(self, image_idx) -> torch.Tensor:
    """mlp_scene.py:331-336."""
    return self.color_table(image_idx)

  def eval_colors(self, point_indexes: torch.Tensor, camera_params: CameraParams, image_idx: Optional[int]) -> Colors:
    """mlp_scene.py:352-368: an image that is not a training image (or None) gets a zero GLO vector."""
    if image_idx is not None and self._training[image_idx]:
      glo_feature = self.color_table.weight[image_idx:image_idx + 1]
    else:
      glo_feature = torch.zeros((1, self.config.image_features), device=self.device)
    return self.color_model(self.points.feature[point_indexes], self.points.position[point_indexes],
                            camera_params.camera_position, glo_feature)

  @property
  def gaussians(self) -> Gaussians3D:
    """mlp_scene.py:401-407."""
    p = self.points
    return Gaussians3D(position=p.position, rotation=p.rotation, log_scaling=p.log_scaling, alpha_logit=p.alpha_logit,
                       feature=p.feature)

  @torch.no_grad()
  def update_filter(self, cameras, margin: float = 0.15):
    """Recomputes every point's sampling rate over ``cameras`` (anything ``CameraBatch.of`` accepts; the training views)
    and stores it as the column ``filter_rate`` of ``points``.  Call it when the cameras or the points have changed,
    e.g. after a densify round: until then ``split_and_prune`` keeps the rate of the rows it keeps and gives children
    their parent's.  Points that no camera samples get the smallest rate among the others (the strongest filter)."""
    if not self.config.filter_3d > 0:
      raise ValueError("update_filter needs MLPSceneConfig.filter_3d > 0 (the filter's strength; 0 = off)")
    self.points.tensors["filter_rate"] = sampling_rate(cameras, self.points.position.detach(), margin=margin)

  def _filtered_gaussians(self) -> Gaussians3D:
    """What ``render`` projects: ``gaussians``, through the 3-D smoothing filter when ``config.filter_3d`` > 0."""
    if not self.config.filter_3d > 0:
      return self.gaussians
    if "filter_rate" not in self.points.tensors:
      raise RuntimeError("MLPSceneConfig.filter_3d > 0 but the scene has no sampling rates yet: call "
                         "update_filter(cameras) with the training cameras first")
    return smooth_gaussians(self.gaussians, self.points.tensors["filter_rate"], self.config.filter_3d)

  def render(self, camera_params: CameraParams, image_idx: Optional[int] = None, specular_weight: float = 1.0,
             render_geometry: bool = False, **options) -> Rendering:
    """mlp_scene.py:410-427: project, colour the culled points, rasterise ``colors.total(specular_weight)``; the
    rendering's ``points.attributes`` are the ``Colors`` and its image has gone through ``post_activation``.  With
    ``config.filter_3d`` > 0 the smoothed Gaussians are projected (one autograd node in front of the projection).

    ``render_geometry`` rasterises the rows of ``geometry_features`` behind the colour, 8 channels on the wide path, and
    returns them as ``geometry_image`` (H, W, 5), with their graph: the input of ``normal_consistency_loss``."""
    config = pop_raster_config(options)
    prefetch = {}
    gaussians = self._filtered_gaussians()
    gaussians2d, depth, indexes = project_to_image(gaussians, camera_params, config, prefetch=prefetch)
    colors = self.eval_colors(indexes, camera_params, image_idx)
    features = colors.total(specular_weight)
    if render_geometry:
      if features.shape[1] != 3:
        raise ValueError(f"render_geometry needs a 3-channel colour, got {features.shape[1]} channels")
      features = torch.cat([features, geometry_features(gaussians, indexes, depth, camera_params)], 1)
    rendering = render_projected(indexes, gaussians2d, features, depth, camera_params, config,
                                 _depth_order=prefetch.get("depth_order"), **options)
    image = rendering.image[..., :3] if render_geometry else rendering.image
    return replace(rendering, points=rendering.points.replace(attributes=colors),
                   image=self.color_model.post_activation(image),
                   geometry_image=rendering.image[..., 3:8] if render_geometry else None)

  @torch.no_grad()
  def query_visibility(self, camera_params: CameraParams) -> Tuple[torch.Tensor, torch.Tensor]:
    """mlp_scene.py:372-381: indexes and visibility of the points that reach a pixel (one zero feature channel)."""
    config = RasterConfig(compute_visibility=True)
    gaussians2d, depth, indexes = project_to_image(self._filtered_gaussians(), camera_params, config)
    feature = torch.zeros((indexes.shape[0], 1), device=self.device)
    rendering = render_projected(indexes, gaussians2d, feature, depth, camera_params, config)
    visible = rendering.points.visible
    return visible.idx, visible.visibility

  def evaluate_sh_features(self, cameras: Sequence[CameraParams], image_indexes: Sequence[Optional[int]], epochs: int = 1,
                           sh_degree: int = 2, generator: Optional[torch.Generator] = None, method: str = "adam",
                           ridge: float = DEFAULT_RIDGE) -> torch.Tensor:
    """mlp_scene.py:384-391 + scene/transfer_sh.py:54-113: per-point SH coefficients (N, 3, (sh_degree + 1)^2) fitted to
    the scene's view-dependent colours.  Cameras at half resolution in a random order per epoch; Adam, base band lr 0.1,
    higher bands lr 0.01 with weight decay 1e-4; visibility-weighted MSE + 0.1 L1 of the base colour.  ``generator``: a
    CPU generator for the initial coefficients and the camera order.

    ``method="lstsq"`` solves the weighted fit over the same half-resolution cameras directly instead (sh_fit.fit_sh:
    one pass in the given order, ``ridge`` on the higher bands; no ``epochs``, no ``generator``; a point no camera sees
    gets zero coefficients, not random ones)."""
    if method not in ("adam", "lstsq"):
      raise ValueError(f"method must be 'adam' or 'lstsq', got {method!r}")

    def eval_colors(idx, cam, image_idx):
      with torch.no_grad():
        return self.color_model.post_activation(self.eval_colors(idx, cam, image_idx).total())

    half = [resized_camera(c, 0.5) for c in cameras]
    if method == "lstsq":
      return fit_sh(eval_colors, self.query_visibility, half, list(image_indexes), self.points.position.detach(),
                    sh_degree=sh_degree, ridge=ridge)[0]
    return transfer_sh(eval_colors, self.query_visibility, half, list(image_indexes), self.points.position.detach(),
                       epochs=epochs, sh_degree=sh_degree, generator=generator)

  def to_sh_gaussians(self, cameras: Sequence[CameraParams], image_indexes: Sequence[Optional[int]], epochs: int = 1,
                      sh_degree: int = 2, generator: Optional[torch.Generator] = None, method: str = "adam",
                      ridge: float = DEFAULT_RIDGE) -> Gaussians3D:
    """mlp_scene.py:394-398: the scene's geometry with fitted SH colours, as ``ply_io.write_gaussians`` takes it.  With
    ``config.filter_3d`` > 0 the scales and opacities are the smoothed ones: the export bakes the filter in, so a
    standard 3DGS viewer shows what was trained.  ``method`` and ``ridge`` as for ``evaluate_sh_features``."""
    feature = self.evaluate_sh_features(cameras, image_indexes, epochs, sh_degree, generator, method=method, ridge=ridge)
    with torch.no_grad():
      g = self._filtered_gaussians()
    return Gaussians3D(position=g.position.detach(), rotation=g.rotation.detach(), log_scaling=g.log_scaling.detach(),
                       alpha_logit=g.alpha_logit.detach(), feature=feature)


def resized_camera(camera: CameraParams, scale: float) -> CameraParams:
  """The camera of the same view at ``scale`` times the resolution (transfer_sh.py:74)."""
  W, H = camera.image_size
  return replace(camera, projection=camera.projection * scale,
                 image_size=(max(1, int(round(W * scale))), max(1, int(round(H * scale)))))


def transfer_sh(eval_colors, query_visibility, cameras: Sequence[CameraParams], image_indexes: Sequence[Optional[int]],
                positions: torch.Tensor, epochs: int = 2, sh_degree: int = 3,
                generator: Optional[torch.Generator] = None) -> torch.Tensor:
  """scene/transfer_sh.py:54-113 over ``evaluate_sh_at`` and ``torch.optim.Adam``."""
  n, dev = positions.shape[0], positions.device
  base_sh = nn.Parameter(torch.randn(n, 3, 1, generator=generator).to(dev))
  higher_sh = nn.Parameter(torch.zeros(n, 3, (sh_degree + 1) ** 2 - 1, device=dev))
  optimizer = torch.optim.Adam([dict(params=[base_sh], lr=0.1, name="base_sh"),
                                dict(params=[higher_sh], lr=0.01, name="higher_sh", weight_decay=1e-4)],
                               betas=(0.9, 0.999))
  for _ in range(epochs):
    for i in torch.randperm(len(cameras), generator=generator).tolist():
      camera = cameras[i]
      optimizer.zero_grad()
      point_indexes, visibility = query_visibility(camera)
      if point_indexes.shape[0] == 0:
        continue
      colors = eval_colors(point_indexes, camera, image_indexes[i])
      with torch.enable_grad():
        pred = evaluate_sh_at(torch.cat([base_sh, higher_sh], dim=2), positions, point_indexes,
                              camera.camera_position).clamp(0, 1)
        mse = torch.nn.functional.mse_loss(pred, colors, reduction="none")
        rgb = torch.nn.functional.l1_loss((base_sh.squeeze(2) * SH_C0 + 0.5)[point_indexes], colors)
        vis = visibility.unsqueeze(1)
        loss = (mse * vis).sum() / vis.sum() + rgb * 0.1
        loss.backward()
      optimizer.step()
  return torch.cat([base_sh, higher_sh], dim=2).detach()
