"""The reference's training loop (``splat_trainer.trainer``: ``Trainer``, ``TrainConfig``, the checkpoint helpers and the
training exceptions) over this package's native pieces: ``MLPScene.render``, ``reference_loss`` (one fused call per
direction), ``MLPScene.reg_loss``, the sparse step, the controllers, ``Evaluation`` and ``PointClusters.view_features``.
Detailed logs (``log_details``) go through ``tensor_histogram`` (histogram.py).

What differs from the reference, because the packages behind it are not here or because it does not work there:
no hydra, beartype, pydispatch, termcolor: ``on_update`` is a plain list of callbacks (``bind(on_update=fn)``); the
progress bar is tqdm's when that imports (and ``TQDM_DISABLE`` is not set) and nothing otherwise; ``TrainConfig.output_path`` says where outputs go (the
reference writes into the working directory, the default here too); the scene holds no logger, so the trainer hands
its own to the scene's ``log_*`` methods; the point-cloud export fits SH coefficients with the direct least-squares fit
over the training cameras.  ``state_dict`` stores ``None`` for a view clustering that does not exist yet (the reference
fails there) and the ``evaluation_log`` (which it reads back but never writes), and the batches already selected but
not yet trained on, so that a restored trainer continues with exactly the batches the live one would have used.
Logged loss scalars are read from ``reference_loss``'s metrics tensor on logging steps only: a step that does not log
waits for the host no more than the render and ``MLPScene.step`` do.  The prefetch thread calls ``dataset.loader`` and
nothing else -- host memory only; batches are selected and uploaded (uint8 -> float / 255) on the training thread.
"""
from __future__ import annotations

import heapq
import json
import math
import os
import queue
import threading
import time
from collections import deque
from dataclasses import dataclass, replace
from enum import Enum
from pathlib import Path
from types import SimpleNamespace
from typing import Any, Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ply_io
from .camera_table import Label, camera_json
from .cloud_init import CloudInitConfig, get_initial_gaussians, to_pointcloud
from .compat import count_nonfinite
from .controller import ControllerConfig, Progress, eval_schedule
from .data_types import CameraParams, Gaussians3D, Rendering
from .dataset import Dataset, ImageView, PointCloud
from .evaluation import Evaluation
from .fusion import FusionConfig, fuse_scene
from .mesh import TriangleMesh, TsdfConfig, mesh_scene
from .histogram import tensor_histogram
from .logger import Logger, LoggerWithState
from .loss import reference_loss
from .normals import normal_consistency_loss
from .visibility import PointClusters, ViewClustering

try:
  from tqdm import tqdm as _tqdm
except ImportError:                                      # the progress bar is optional
  _tqdm = None


class TrainingException(Exception):
  """Base of the exceptions that abort a training run for a stated reason."""


class NaNParameterException(TrainingException):
  """Non-finite entries were found in the scene's state."""


class NoProgressException(TrainingException):
  """The evaluation metrics stopped improving: the run is not worth finishing."""


class TrainingTimeoutException(TrainingException):
  """Training steps are slower than ``TrainConfig.min_step_rate``."""


class TrainerState(Enum):
  Stopped = 0
  Training = 1
  Paused = 2


@dataclass(kw_only=True, frozen=True)
class TrainConfig:
  """trainer/config.py TrainConfig: the reference's fields and defaults; ``output_path``, ``prefetch`` and ``seed`` are
  this package's."""
  scene: Any                        # MLPSceneConfig (from_color_gaussians / from_state_dict)
  controller: ControllerConfig
  view_selection: Any               # a sampler config: create(train_idx) / from_state_dict(state, train_idx)
  cloud_init: CloudInitConfig

  total_steps: int
  eval_steps: int
  log_interval: int = 10

  target_points: int
  densify_interval: Any = 100

  min_step_rate: Optional[float] = None      # steps per second over 10 log intervals below which training aborts
  max_ssim_regression: float = 0.04

  num_logged_images: int = 8
  log_worst_images: int = 2
  log_details: bool = False

  ssim_weight: float = 0.0
  mse_weight: float = 0.0
  l1_weight: float = 0.0
  ssim_levels: int = 4

  normal_weight: float = 0.0                 # depth-normal consistency (normals.py); 0 = off: the step is unchanged
  normal_from: float = 0.3                   # fraction of the training progress from which the term is added
  normal_alpha_min: float = 0.5              # pixels below this accumulated alpha have no depth for the term

  vis_clusters: int = 1024

  antialias: bool = False
  blur_cov: float = 0.3

  device: str

  save_checkpoints: bool = False
  save_output: bool = True
  log_images: bool = True

  output_path: Optional[str] = None          # None: the working directory
  prefetch: int = 4                          # batches selected and loaded ahead of the step that trains on them
  seed: Optional[int] = None                 # of the initial cloud's draws and the scene's point features


def find_checkpoint(path: Path, checkpoint: Optional[int] = None) -> Path:
  """``path / "checkpoint" / "checkpoint_<n>.pt"`` with the largest n, or with n = ``checkpoint``."""
  checkpoint_path = Path(path) / "checkpoint"
  found = {}
  for file in checkpoint_path.glob("checkpoint_*.pt"):
    number = file.stem.split("_")[1]
    if number.isdigit():
      found[int(number)] = file
  if not found:
    raise FileNotFoundError(f"No checkpoints found in {checkpoint_path}")
  n = max(found) if checkpoint is None else checkpoint
  if n not in found:
    raise FileNotFoundError(f"Checkpoint {n} not found, options are {sorted(found)}")
  return found[n]


def load_checkpoint(splat_path: Path, step: Optional[int] = None) -> Tuple[dict, Path]:
  """(state_dict, workspace path) of a workspace directory (its newest checkpoint, or ``step``) or a checkpoint file."""
  splat_path = Path(splat_path)
  if splat_path.is_dir():
    workspace_path, checkpoint = splat_path, find_checkpoint(splat_path, step)
  elif splat_path.is_file():
    workspace_path, checkpoint = splat_path.parent.parent, splat_path
  else:
    raise FileNotFoundError(f"Checkpoint {splat_path} not found")
  return torch.load(checkpoint, weights_only=True), workspace_path


class _Prefetcher:
  """A thread that turns submitted batch indices into ``dataset.loader(idx)`` results, in order.  Host work only."""

  def __init__(self, load: Callable[[torch.Tensor], Sequence[ImageView]]):
    self._load = load
    self._requests, self._results = queue.Queue(), queue.Queue()
    self._thread = threading.Thread(target=self._run, daemon=True)
    self._thread.start()

  def _run(self):
    while True:
      idx = self._requests.get()
      if idx is None:
        return
      try:
        self._results.put(self._load(idx))
      except BaseException as e:              # handed to the training thread, which raises it
        self._results.put(e)

  def submit(self, idx: torch.Tensor):
    self._requests.put(idx)

  def next(self) -> Sequence[ImageView]:
    result = self._results.get()
    if isinstance(result, BaseException):
      raise result
    return result

  def stop(self):
    self._requests.put(None)
    self._thread.join()


class Trainer:
  """trainer/trainer.py Trainer."""

  def __init__(self, config: TrainConfig, scene, controller, dataset: Dataset, logger: LoggerWithState, view_selection,
               step: int = 0, evaluation_log: Optional[List[dict]] = None,
               view_clustering: Optional[ViewClustering] = None, pending_batches: Optional[List[torch.Tensor]] = None):
    if not isinstance(logger, LoggerWithState):
      raise TypeError("Trainer takes a LoggerWithState (Trainer.initialize wraps any Logger)")
    self.device = torch.device(config.device)
    self.config = config
    self.scene = scene
    self.controller = controller
    self.dataset = dataset
    self.camera_table = dataset.camera_table.to(self.device)
    self.logger = logger
    self.view_selection = view_selection
    self.view_clustering = view_clustering
    self.evaluation_log = list(evaluation_log or [])
    self.step = step
    self.last_checkpoint = step
    self.state = TrainerState.Stopped
    self.pbar = None
    self.running_time = deque(maxlen=10)
    self.last_time = None
    self._on_update: List[Callable[[], None]] = []
    self._pending = deque(pending_batches or [])
    self._prefetcher: Optional[_Prefetcher] = None
    self._camera_params: Dict[int, CameraParams] = {}

  # ---------------------------------------------------------------------------------------------------- construction
  @staticmethod
  def _train_idx(camera_table) -> torch.Tensor:
    return camera_table.cameras.has_label(Label.Training)

  @staticmethod
  def initialize(config: TrainConfig, dataset: Dataset, logger: Logger) -> "Trainer":
    device = torch.device(config.device)
    camera_table = dataset.camera_table.to(device)
    generator = None if config.seed is None else torch.Generator().manual_seed(config.seed)
    initial_gaussians = get_initial_gaussians(config.cloud_init, dataset, device, generator=generator)
    if not isinstance(logger, LoggerWithState):
      logger = LoggerWithState(logger)
    scene = config.scene.from_color_gaussians(initial_gaussians, camera_table.num_images, device, seed=config.seed)
    progress = Progress(step=0, total_steps=config.total_steps, logging_step=False)
    controller = config.controller.make_controller(scene, config.target_points, progress, logger)
    view_selection = config.view_selection.create(Trainer._train_idx(camera_table))
    trainer = Trainer(config, scene, controller, dataset, logger, view_selection)
    if config.save_output:                                # in the original coordinates: the normalisation undone
      paths = trainer.paths()
      trainer.write_cameras(paths.cameras)
      to_pointcloud(dataset.to_original.transform_gaussians(initial_gaussians)).save_ply(paths.point_cloud)
    return trainer

  @staticmethod
  def from_state_dict(config: TrainConfig, dataset: Dataset, logger: Logger, state_dict: dict) -> "Trainer":
    device = torch.device(config.device)
    camera_table = dataset.camera_table.to(device)
    if not isinstance(logger, LoggerWithState):
      logger = LoggerWithState(logger)
    step = state_dict["step"]
    scene = config.scene.from_state_dict(state_dict["scene"], camera_table.num_images)
    progress = Progress(step=step, total_steps=config.total_steps)
    controller = config.controller.from_state_dict(state_dict["controller"], scene, target_points=config.target_points,
                                                   progress=progress, logger=logger)
    view_selection = config.view_selection.from_state_dict(
        {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in state_dict["view_selection"].items()},
        Trainer._train_idx(camera_table))
    clustering = state_dict.get("view_clustering")
    view_clustering = None if clustering is None else ViewClustering.from_state_dict(clustering)
    return Trainer(config, scene, controller, dataset, logger, view_selection, step=step,
                   evaluation_log=[dict(e) for e in state_dict.get("evaluation_log") or []],
                   view_clustering=view_clustering,
                   pending_batches=[b.clone() for b in state_dict.get("pending_batches") or []])

  def state_dict(self) -> dict:
    return dict(step=self.step, scene=self.scene.state_dict(), controller=self.controller.state_dict(),
                view_selection=self.view_selection.state_dict(),
                view_clustering=None if self.view_clustering is None else self.view_clustering.state_dict(),
                evaluation_log=[dict(e) for e in self.evaluation_log], pending_batches=list(self._pending))

  def clone(self) -> "Trainer":
    return self.from_state_dict(self.config, self.dataset, self.logger, self.state_dict())

  def replace(self, logger: Optional[Logger] = None, **kwargs) -> "Trainer":
    """A clone with a changed config."""
    return self.from_state_dict(replace(self.config, **kwargs), self.dataset, logger or self.logger, self.state_dict())

  def update_config(self, **kwargs):
    self.config = replace(self.config, **kwargs)

  def bind(self, on_update: Optional[Callable[[], None]] = None):
    """``on_update`` is called after every logging step of ``train``."""
    if on_update is not None:
      self._on_update.append(on_update)

  def emit(self, event: str):
    if event != "on_update":
      raise ValueError(f"unknown event {event!r}")
    for fn in list(self._on_update):
      fn()

  def __repr__(self):
    return f"Trainer(step={self.step}, scene={self.scene} controller={self.controller})"

  # ----------------------------------------------------------------------------------------------------------- output
  @property
  def unnormalize(self):
    return self.dataset.to_original

  @property
  def output_path(self) -> Path:
    return Path.cwd() if self.config.output_path is None else Path(self.config.output_path)

  def paths(self, step: Optional[int] = None) -> SimpleNamespace:
    step = self.step if step is None else step
    root = self.output_path
    paths = dict(checkpoint=root / "checkpoint" / f"checkpoint_{step}.pt",
                 point_cloud=root / "point_cloud" / f"iteration_{step}" / "point_cloud.ply",
                 cameras=root / "cameras.json", workspace=root)
    for name, path in paths.items():
      (path if name == "workspace" else path.parent).mkdir(parents=True, exist_ok=True)
    return SimpleNamespace(**paths)

  def print(self, text: str):
    if self.pbar is not None:
      self.pbar.write(text)
    else:
      print(text)

  def write_cameras(self, filename):
    with open(filename, "w") as f:
      cameras = self.unnormalize.transform_cameras(self.camera_table.cameras)
      json.dump(camera_json(cameras), f, indent=2, sort_keys=True)

  def write_checkpoint(self):
    paths = self.paths()
    torch.save(self.state_dict(), paths.checkpoint)
    ply_io.write_gaussians(paths.point_cloud, self.sh_gaussians(), with_sh=True)
    self.print(f"Checkpoint saved to {paths.checkpoint}")

  def sh_gaussians(self) -> Gaussians3D:
    """The scene with SH colours fitted over the training cameras, in the original coordinates."""
    train_idx = self._train_idx(self.camera_table).tolist()
    cameras = [self.camera_params(i) for i in train_idx]
    return self.unnormalize.transform_gaussians(self.scene.to_sh_gaussians(cameras, train_idx, method="lstsq"))

  def fused_cloud(self, config: Optional[FusionConfig] = None, which: str = "train") -> PointCloud:
    """The dense cloud fused from the median depth maps of the ``which`` = "train" or "val" views (fusion.fuse_scene),
    in the original coordinates."""
    if which not in ("train", "val"):
      raise ValueError(f"which must be 'train' or 'val', got {which!r}")
    views = self.dataset.train(shuffle=False) if which == "train" else self.dataset.val()
    indexes = [int(v.image_idx) for v in views]
    if not indexes:
      raise ValueError(f"the dataset has no {which} views")
    render = lambda camera, idx: self.render(camera, idx, render_median_depth=True)      # noqa: E731
    cloud, _ = fuse_scene(render, [self.camera_params(i) for i in indexes], config or FusionConfig(), indexes)
    return self.unnormalize.transform_cloud(cloud)

  def write_fused_cloud(self, path, config: Optional[FusionConfig] = None, which: str = "train") -> PointCloud:
    cloud = self.fused_cloud(config, which)
    cloud.save_ply(path)
    return cloud

  def mesh(self, config: Optional[TsdfConfig] = None, which: str = "train") -> TriangleMesh:
    """The triangle mesh of the TSDF volume integrated from the median depth maps of the ``which`` = "train" or "val"
    views (mesh.mesh_scene), in the original coordinates."""
    if which not in ("train", "val"):
      raise ValueError(f"which must be 'train' or 'val', got {which!r}")
    views = self.dataset.train(shuffle=False) if which == "train" else self.dataset.val()
    indexes = [int(v.image_idx) for v in views]
    if not indexes:
      raise ValueError(f"the dataset has no {which} views")
    render = lambda camera, idx: self.render(camera, idx, render_median_depth=True)      # noqa: E731
    mesh = mesh_scene(render, [self.camera_params(i) for i in indexes], config or TsdfConfig(), indexes)
    return mesh.transformed(self.unnormalize)

  def write_mesh(self, path, config: Optional[TsdfConfig] = None, which: str = "train") -> TriangleMesh:
    mesh = self.mesh(config, which)
    mesh.save_ply(path)
    return mesh

  def load_cloud(self) -> Gaussians3D:
    paths = self.paths()
    if paths.point_cloud.exists():
      return ply_io.read_gaussians(paths.point_cloud, with_sh=True).to(self.device)
    return self.sh_gaussians().to(self.device)

  # ---------------------------------------------------------------------------------------------------------- render
  @property
  def progress(self) -> Progress:
    return Progress(step=self.step, total_steps=self.config.total_steps, logging_step=self.is_logging_step)

  @property
  def is_logging_step(self) -> bool:
    return self.step % self.config.log_interval == 0

  @property
  def normal_term_active(self) -> bool:
    """Whether this step renders the geometry image and adds the depth-normal consistency term."""
    return self.config.normal_weight > 0 and self.progress.t >= self.config.normal_from

  def camera_params(self, cam_idx: int) -> CameraParams:
    """The camera of image ``cam_idx`` on the device.  The table is not trained by this loop, so each is read once."""
    cam_idx = int(cam_idx)
    if cam_idx not in self._camera_params:
      camera = self.camera_table[cam_idx].item()
      self._camera_params[cam_idx] = camera.to_camera_params().to(self.device, dtype=torch.float32)
    return self._camera_params[cam_idx]

  def render(self, camera_params: CameraParams, image_idx: Optional[int] = None, **options) -> Rendering:
    return self.scene.render(camera_params, image_idx, **options, antialias=self.config.antialias,
                             compute_visibility=True, compute_point_heuristic=True,
                             blur_cov=0.0 if self.config.antialias else self.config.blur_cov)

  # ------------------------------------------------------------------------------------------------------ evaluation
  def evaluate_image(self, image_view: ImageView) -> Evaluation:
    image_view = self.load_data(image_view)
    with torch.no_grad():
      rendering = self.render(self.camera_params(image_view.image_idx), image_view.image_idx, render_median_depth=True)
    return Evaluation(image_view.filename, rendering.detach(), image_view.image)

  def iter_evaluations(self, image_views: Sequence[ImageView]) -> Iterator[Evaluation]:
    for image_view in image_views:
      yield self.evaluate_image(image_view)

  def _logged_indices(self, n: int, random_seed: int) -> set:
    rng = np.random.RandomState(random_seed)
    return set(rng.choice(n, min(self.config.num_logged_images, n), replace=False).tolist()) if n else set()

  def evaluate_training(self, name: str, image_views: Sequence[ImageView], random_seed: int = 0):
    """Evaluates the training views, logs a selection of them and the worst by PSNR, and rebuilds the view clustering
    from every view's cluster visibilities."""
    worst: List[Tuple[float, int, Evaluation]] = []          # the config.log_worst_images lowest PSNRs
    view_features, metrics = [], {}
    point_clusters = PointClusters.cluster(self.scene.points.position.detach(), self.config.vis_clusters)
    point_visible = torch.zeros(self.scene.num_points, dtype=torch.int32, device=self.device)
    log_indices = self._logged_indices(len(image_views), random_seed)
    for i, image_view in enumerate(image_views):
      evaluation = self.evaluate_image(image_view)
      if i in log_indices:
        self.log_evaluation_images(f"{name}_images/{evaluation.image_id}", evaluation, log_source=self.step == 0)
      if self.config.log_worst_images > 0:
        entry = (-evaluation.psnr, i, evaluation)            # a max-heap on -psnr keeps the lowest PSNRs
        if len(worst) < self.config.log_worst_images:
          heapq.heappush(worst, entry)
        elif entry > worst[0]:
          heapq.heapreplace(worst, entry)
      metrics[evaluation.filename] = evaluation.metrics
      points = evaluation.rendering.points.visible
      view_features.append(point_clusters.view_features(points.idx, points.visibility))
      point_visible.index_add_(0, points.idx, torch.ones_like(points.idx, dtype=torch.int32))
    for i, (_, _, evaluation) in enumerate(sorted(worst, reverse=True)):
      self.log_evaluation_images(f"{name}_images/worst_{i}", evaluation, log_source=True)
    self.logger.log_histogram(f"eval_{name}/points_visible", tensor_histogram(point_visible))
    self.log_evaluation_table(name, metrics)
    if view_features:
      self.view_clustering = ViewClustering(point_clusters, torch.stack(view_features))

  def evaluate_dataset(self, name: str, image_views: Sequence[ImageView], random_seed: int = 0):
    """Evaluates a set of views and logs their metrics, raw and colour-corrected."""
    metrics, metrics_cc = {}, {}
    log_indices = self._logged_indices(len(image_views), random_seed)
    for i, image_view in enumerate(image_views):
      evaluation = self.evaluate_image(image_view)
      corrected = evaluation.color_corrected()
      metrics[evaluation.filename] = evaluation.metrics
      metrics_cc[corrected.filename] = corrected.metrics
      if i in log_indices:
        self.log_evaluation_images(f"{name}_images/{corrected.image_id}", corrected, log_source=self.step == 0)
    self.log_evaluation_table(name, metrics)
    self.log_evaluation_table(f"{name}_cc", metrics_cc)

  def log_evaluation_images(self, name: str, evaluation: Evaluation, log_source: bool = True):
    if not self.config.log_images:
      return
    self.logger.log_image(f"{name}/render", evaluation.rendering.image,
                          caption=f"{evaluation.filename} PSNR={evaluation.psnr:.3f} L1={evaluation.l1:.2f} "
                                  f"ssim={evaluation.ssim:.2f}")
    depth = evaluation.rendering.median_ndc_image
    if depth is not None:
      self.logger.log_image(f"{name}/depth", depth, caption=evaluation.filename)
    if log_source:
      self.logger.log_image(f"{name}/image", evaluation.source_image, caption=evaluation.filename)

  def log_evaluation_table(self, name: str, metrics: Dict[str, Dict[str, float]]):
    self.logger.log_evaluations(f"eval_{name}/evals", metrics)
    rows = list(metrics.values())
    for k in (rows[0] if rows else {}):
      values = [row[k] for row in rows]
      self.logger.log_value(f"eval_{name}/{k}", float(np.mean(values)))
      self.logger.log_histogram(f"eval_{name}/{k}_hist", torch.tensor(values, dtype=torch.float32))

  def evaluate(self) -> Dict[str, float]:
    self.print(f"Performing evaluation at step {self.step}")
    self.evaluate_training("train", self.dataset.train(shuffle=False))
    val = self.dataset.val()
    if len(val) > 0:
      self.evaluate_dataset("val", val)
    means = self.eval_metrics()
    self.print(f"step={self.step:<6d} n={self.scene.num_points:<7} " +
               " ".join(f"{k}:{v:.4f}" for k, v in means.items()))
    self.update_progress()
    return means

  def eval_metrics(self, metrics: Tuple[str, ...] = ("ssim", "psnr")) -> Dict[str, float]:
    result = {}
    for category in ("train", "val", "val_cc"):
      name = f"eval_{category}"
      if name in self.logger:
        result.update({f"{category}_{k}": v.value for k, v in self.logger[name].items()
                       if k in metrics and hasattr(v, "value")})
    return result

  # -------------------------------------------------------------------------------------------------------- training
  def reg_weights(self) -> Dict[str, float]:
    """This step's values of the scene's regulariser weights (numbers, or schedules of the progress)."""
    progress = self.progress
    return {k: float(eval_schedule(v, progress)) for k, v in self.scene.config.reg_weight.items()}

  def compute_losses(self, rendering: Rendering, image: torch.Tensor) -> torch.Tensor:
    """One fused loss call plus the scene's regulariser and, on a rendering with a geometry image while
    ``normal_term_active``, ``normal_weight`` times the depth-normal consistency loss.  The logged scalars come from the
    metrics tensor [loss, l1, mse, ssim_0, ...] and are read on logging steps only, in one read."""
    config = self.config
    loss, metrics = reference_loss(rendering.image, image, l1_weight=config.l1_weight, mse_weight=config.mse_weight,
                                   ssim_weight=config.ssim_weight, ssim_levels=config.ssim_levels, return_metrics=True)
    reg_loss = self.scene.reg_loss(rendering, self.reg_weights())
    total = loss + reg_loss
    normal_loss = None
    if rendering.geometry_image is not None and self.normal_term_active:
      normal_loss = config.normal_weight * normal_consistency_loss(rendering.geometry_image, rendering.camera.projection,
                                                                   alpha_min=config.normal_alpha_min)
      total = total + normal_loss
    if self.is_logging_step:
      extra = [reg_loss.detach().reshape(1)] + ([] if normal_loss is None else [normal_loss.detach().reshape(1)])
      values = torch.cat([metrics.detach().reshape(-1)] + extra).tolist()                            # one read
      terms = {}
      if normal_loss is not None:
        terms["normal"] = values.pop()
      image_loss, l1, mse, ssim, reg = values[0], values[1], values[2], values[3], values[-1]
      ssim_loss = sum(1.0 - s for s in values[3:-1]) / config.ssim_levels
      self.logger.log_values("train/loss", dict(l1=l1 * config.l1_weight, mse=mse * config.mse_weight,
                                                ssim=ssim_loss * config.ssim_weight, reg=reg, **terms,
                                                total=image_loss + reg + terms.get("normal", 0.0)))
      psnr = 10 * math.log10(1 / mse) if mse > 0 else math.inf
      self.logger.log_values("train/metrics", dict(l1=l1, mse=mse, ssim=ssim, psnr=psnr))
    return total

  def evaluate_backward_with(self, batch: List[ImageView], f: Callable[[int, Rendering], None]):
    for image_view in batch:
      camera_params = self.camera_params(image_view.image_idx)
      with torch.enable_grad():
        geometry = dict(render_geometry=True) if self.normal_term_active else {}
        rendering = self.render(camera_params, image_view.image_idx, **geometry)
        if rendering.points.idx.shape[0] == 0:
          raise TrainingException(f"No visible points: {image_view.filename} - check training parameters or dataset "
                                  "camera poses")
        loss = self.compute_losses(rendering, image_view.image)
        loss.backward()
      f(image_view.image_idx, rendering)

  def log_rendering_histograms(self, rendering: Rendering):
    """log10 histograms of the per-point outputs of one rendering, over the points that reached a pixel."""
    points = rendering.points
    rows = torch.nonzero(points.visible_mask).squeeze(1)
    for name, values, min_value in (("prune_cost", points.prune_cost, 1e-20), ("split_score", points.split_score, 1e-10),
                                    ("max_scale_px", points.screen_scale, 1e-6), ("visibility", points.visibility, 1e-10)):
      self.logger.log_histogram(f"rendering/log10_{name}",
                                tensor_histogram(values, rows=rows, log10="drop", min_value=min_value))

  def training_step(self, batch: List[ImageView]):
    """render -> loss -> backward -> scene.add_rendering -> controller.add_rendering -> (details) -> scene.step ->
    logger.step, as the reference orders them."""
    self.step += len(batch)
    details = self.config.log_details and self.is_logging_step

    @torch.no_grad()
    def f(image_idx: int, rendering: Rendering):
      self.scene.add_rendering(image_idx, rendering)
      self.controller.add_rendering(image_idx, rendering, self.progress)
      if details:
        self.log_rendering_histograms(rendering)

    self.evaluate_backward_with(batch, f)
    if details:                                              # (the reference's scene.step(log_details=True))
      self.scene.log_gradients(self.logger)
      self.scene.log_optimizer_state(self.logger)
      self.scene.log_params(self.logger)
    self.scene.step()
    self.logger.step(self.progress)

  # ------------------------------------------------------------------------------------------------------------ data
  def load_data(self, image_view: ImageView) -> ImageView:
    """The view with its image on the device as float in [0, 1] (a view that already is one passes through)."""
    image = image_view.image
    if image.dtype is torch.uint8:
      image = image.to(self.device, non_blocking=True) / 255.0           # (true division: float32 in one launch)
    else:
      image = image.to(self.device, dtype=torch.float32)
    return replace(image_view, image=image.contiguous())

  def load_batch(self, batch_idx: torch.Tensor) -> List[ImageView]:
    return [self.load_data(view) for view in self.dataset.loader(batch_idx)]

  def _refill(self):
    """Selects batches until ``config.prefetch`` (at least one) wait to be trained on, and hands the new ones to the
    prefetch thread when there is one."""
    while len(self._pending) < max(1, self.config.prefetch):
      batch_idx = self.view_selection.select_images(self.view_clustering, self.progress).detach().cpu().clone()
      self._pending.append(batch_idx)
      if self._prefetcher is not None:
        self._prefetcher.submit(batch_idx)

  def iter_batches(self) -> Iterator[List[ImageView]]:
    """Batches without end, each uploaded on this thread.  Selection runs ``config.prefetch`` batches ahead; the
    selected indices are part of ``state_dict``."""
    while True:
      self._refill()
      views = self._prefetcher.next() if self._prefetcher is not None else self.dataset.loader(self._pending[0])
      self._pending.popleft()
      yield [self.load_data(view) for view in views]

  # ------------------------------------------------------------------------------------------------------- main loop
  def is_training(self) -> bool:
    return self.state in (TrainerState.Training, TrainerState.Paused)

  def set_paused(self, paused: bool):
    if not self.is_training():
      raise RuntimeError("set_paused outside train()")
    self.state = TrainerState.Paused if paused else TrainerState.Training
    if self.pbar is not None:
      self.pbar.set_description_str(self.state.name)

  def checkpoint(self, save: bool = True):
    """Checks the scene for non-finite entries, evaluates, applies the abort rules and (``save`` and
    ``config.save_output``) writes a checkpoint."""
    bad = count_nonfinite(self.scene.state_dict(), "scene")
    if len(bad) > 0:
      raise NaNParameterException(f"Non-finite entries detected: {bad}")
    self.scene.log_checkpoint(self.logger, self.progress)
    metrics = self.evaluate()
    if len(self.evaluation_log) > 0:
      ssim = metrics["train_ssim"]
      prev_ssim = self.evaluation_log[-1]["train_ssim"]
      initial_ssim = self.evaluation_log[0]["train_ssim"]
      if ssim < initial_ssim:
        raise NoProgressException("Training aborted - ssim is worse than untrained ssim")
      if prev_ssim > ssim + self.config.max_ssim_regression:
        raise NoProgressException(f"Training aborted - ssim regression exceeded {prev_ssim:4f} - {ssim:4f} > "
                                  f"{self.config.max_ssim_regression:4f}")
    self.evaluation_log.append(dict(step=self.step, **metrics))
    if save and self.config.save_output:
      self.write_checkpoint()
    self.last_checkpoint = self.step
    if self.device.type == "cuda":
      torch.cuda.empty_cache()

  def pbar_metrics(self) -> List[str]:
    desc = []
    if "densify" in self.logger:
      pruned, split, n = [self.logger.get_value(f"densify/{k}", 0) for k in ("prune", "split", "n")]
      desc.append(f"points(+{split} -{pruned} = {n})")
    if "train/metrics" in self.logger:
      ssim, psnr = [self.logger.get_value(f"train/metrics/{k}", math.nan) for k in ("ssim", "psnr")]
      desc.append(f"ssim:{ssim:.3f} psnr:{psnr:.3f}")
    if "train/loss" in self.logger:
      desc.append("losses(" + ", ".join(f"{k}:{v.value:.3f}" for k, v in self.logger["train/loss"].items()) + ")")
    return desc

  def update_progress(self):
    if self.pbar is not None:
      self.pbar.update(self.progress.step - self.pbar.n)
      self.pbar.set_postfix_str(" ".join(self.pbar_metrics()))
    if not self.is_training():
      return
    current_time = time.time()
    if self.last_time is not None:                           # (timing starts after the first interval or evaluation)
      self.running_time.append(current_time - self.last_time)
      step_rate = self.config.log_interval / float(np.mean(self.running_time))
      self.logger.log_value("train/step_rate", step_rate)
      if (self.config.min_step_rate is not None and len(self.running_time) == self.running_time.maxlen
              and step_rate < self.config.min_step_rate):
        raise TrainingTimeoutException(f"Step rate lower than config.min_step_rate: {step_rate:.3f} < "
                                       f"{self.config.min_step_rate:.3f}")
    self.last_time = current_time

  def train(self, state: TrainerState = TrainerState.Training) -> Dict[str, float]:
    self.state = state
    self.dataset.load_images()
    self.checkpoint(self.config.save_checkpoints)
    self.print(f"Beginning training for {self.config.total_steps - self.step} steps, eval_steps={self.config.eval_steps}")
    self._prefetcher = _Prefetcher(self.dataset.loader)
    for batch_idx in self._pending:                          # (restored from a state dict, or left by an earlier run)
      self._prefetcher.submit(batch_idx)
    if _tqdm is not None and not os.environ.get("TQDM_DISABLE"):
      self.pbar = _tqdm(initial=self.step, total=self.config.total_steps, desc=self.state.name)
    try:
      batches = self.iter_batches()
      while self.step < self.config.total_steps:
        if self.state == TrainerState.Paused:
          self.emit("on_update")
          time.sleep(0.1)
          continue
        self.training_step(next(batches))
        if self.last_checkpoint + self.config.eval_steps <= self.step:
          self.checkpoint(self.config.save_checkpoints or self.step >= self.config.total_steps)
          self.last_time = None
        self.controller.step(self.progress)
        if self.is_logging_step:
          self.emit("on_update")
          self.update_progress()
    finally:
      self.state = TrainerState.Stopped
      self._prefetcher.stop()
      self._prefetcher = None
      if self.pbar is not None:
        self.pbar.close()
        self.pbar = None
    return self.eval_metrics()

  def close(self):
    self.logger.close()
    if self._prefetcher is not None:
      self._prefetcher.stop()
      self._prefetcher = None
