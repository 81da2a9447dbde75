"""The reference's ``controller/`` package (``controller.py``, ``disabled.py``, ``target_controller.py``,
``mcmc_controller.py`` and ``densify_and_prune`` / ``log_histograms`` of ``point_state.py:59-110``) over this package's
pieces: ``controller_math.PointState`` / ``take_n`` / ``find_split_prune_indexes``, the scene's ``split_and_prune`` and one
native kernel for the MCMC controller's per-step position noise (csrc/controller.hip, maths in csrc/gsr_controller.h).
Beyond the reference: ``MCMCConfig.relocate`` switches the MCMC controller's prune step to the relocation move of the
MCMC paper -- ``relocate_points`` / ``grow_points`` over ``weighted_draws``, native too (csrc/relocate.hip).

What differs from the reference's surface, because the packages behind it are not here: no hydra, beartype or tensordict.
A schedule-valued field (``TargetConfig.densify_prune_interval``, ``MCMCConfig.noise_level``) is a number or a callable of
``t``.  ``scene`` is duck-typed -- ``num_points``, ``device``, ``points`` (a ``ParameterClass``) and
``split_and_prune(keep_mask, split_idx)`` -- and ``logger`` is None or anything with ``log_values`` / ``log_histogram``.
``TargetController.step`` does not empty the allocator's cache: that is the trainer's choice.

Two deliberate deviations from ``mcmc_controller.py``:

* its noise branch perturbs ``self.scene.points.tensors[enough_views]``, which with a bool mask is a COPY: ``position +=``
  never reaches the scene and the reference's noise is a no-op.  Here the noise is applied to ``scene.points.position``
  in place, on the rows with ``points_in_view > min_views`` -- the evident intent;
* its prune branch takes the ``n`` top-scored rows with an unstable ``argsort`` over scores of which the pruned rows
  are zeroed, so pruned rows may be picked among the zeros.  Here a pruned row is never split
  (``split_mask &= ~prune_mask``); the point count then falls by the overlap.

The noise is drawn by a counter-based generator (Philox4x32-10) keyed on (``MCMCConfig.seed``, step, point index), not by
``torch.randn``: data-parallel replicas that hold full parameter copies add the SAME noise with no communication, and a
run restarted from a checkpoint repeats itself.  ``max_prune_rate`` of the reference's dataclass is read nowhere and is
left out.
"""
from __future__ import annotations

import math
from abc import ABCMeta, abstractmethod
from dataclasses import dataclass, fields
from fractions import Fraction
from typing import Callable, Optional, Tuple, Union

import torch

from . import _lib
from ._args import on_one_device, require
from ._lib import ptr as _ptr
from .controller_math import PointState, find_split_prune_indexes, take_n

Schedule = Union[float, int, Callable[[float], float]]
GATE_MARGIN = 16.0                # soft_lt(opacity, threshold / 2, margin=16.0), mcmc_controller.py:95
SCALE_EPS = 1e-4                  # point_basis(eps=1e-4), gaussians/split.py:17


def _clamp(x: float, lo: float, hi: float) -> float:
  return max(lo, min(x, hi))


@dataclass(frozen=True)
class Progress:
  """config/__init__.py:25-34."""
  step: int
  total_steps: int
  logging_step: bool = False

  @property
  def t(self) -> float:
    return _clamp(self.step / self.total_steps, 0.0, 1.0)

  def __float__(self) -> float:
    return float(self.t)


def eval_schedule(value: Schedule, t: Union[float, Progress]):
  """A number as it is, a callable at ``t`` (config/__init__.py:181-188 without the ``Varying`` class)."""
  return value(float(t)) if callable(value) else value


def smoothstep(t: float, a: float, b: float) -> float:
  """config/__init__.py:127-131 on the interval (0, 1)."""
  t = _clamp(t, 0.0, 1.0)
  return a + (b - a) * (3 * t ** 2 - 2 * t ** 3)


# ---------------------------------------------------------------------------------------------------------- point state
def _columns(state: PointState):
  return [(f.name, getattr(state, f.name)) for f in fields(PointState)]


def point_state_dict(state: PointState) -> dict:
  return {k: v.detach().clone() for k, v in _columns(state)}


def load_point_state(state: PointState, state_dict: dict) -> PointState:
  """Copies ``state_dict`` into the columns of ``state`` (same lengths, the columns' own dtypes and device)."""
  for k, v in _columns(state):
    src = state_dict[k]
    if tuple(src.shape) != tuple(v.shape):
      raise ValueError(f"point state column {k}: {tuple(src.shape)} in the state dict, {tuple(v.shape)} in the controller")
    v.copy_(src)
  return state


def log_histograms(points: PointState, logger, name: str = "densify"):
  """point_state.py:61-72."""
  def log_scale(k, t, min_val=1e-12):
    logger.log_histogram(f"{name}/{k}", torch.log10(torch.clamp_min(t, min_val)))
  log_scale("prune_cost", points.prune_cost)
  log_scale("split_score", points.split_score)
  log_scale("max_scale_px", points.max_scale_px, min_val=1e-6)
  logger.log_histogram(f"{name}/points_in_view", points.points_in_view)
  logger.log_histogram(f"{name}/visibility", points.visibility)


@torch.no_grad()
def densify_and_prune(state: PointState, scene, split_mask: torch.Tensor, prune_mask: torch.Tensor, logger=None,
                      generator: Optional[torch.Generator] = None) -> PointState:
  """point_state.py:76-110: logs the round's metrics, calls ``scene.split_and_prune(~(split | prune), split_idx)``
  (``generator`` is passed on only when one is given) and returns the carried state: the kept rows of all five columns,
  then zeros for the 2 n_split children."""
  split_idx = split_mask.nonzero().squeeze(1)
  n_prune, n_split = int(prune_mask.sum().item()), int(split_idx.shape[0])
  n = int(state.prune_cost.shape[0])
  if logger is not None:
    metrics = dict(n=n, prune=n_prune, split=n_split,
                   max_prune_score=state.prune_cost[prune_mask].max().item() if n_prune > 0 else 0.,
                   min_split_score=state.split_score[split_idx].min().item() if n_split > 0 else 0.,
                   unseen=n - int(torch.count_nonzero(state.prune_cost).item()))
    logger.log_values("densify", metrics)
    log_histograms(state, logger, "densify")
  keep_mask = ~(split_mask | prune_mask)
  if generator is None:
    scene.split_and_prune(keep_mask, split_idx)
  else:
    scene.split_and_prune(keep_mask, split_idx, generator=generator)
  return PointState(**{k: torch.cat([v[keep_mask], v.new_zeros(2 * n_split)]) for k, v in _columns(state)})


# ------------------------------------------------------------------------------------------------------------ interface
class ControllerConfig(metaclass=ABCMeta):
  """controller/controller.py:9-17."""

  @abstractmethod
  def make_controller(self, scene, target_points: int, progress: Progress, logger=None) -> "Controller":
    raise NotImplementedError

  @abstractmethod
  def from_state_dict(self, state_dict: dict, scene, target_points: int, progress: Progress, logger=None) -> "Controller":
    raise NotImplementedError


class Controller(metaclass=ABCMeta):
  """controller/controller.py:20-37."""

  @abstractmethod
  def step(self, progress: Progress, log_details: bool = False):
    """Perform densification and pruning."""
    raise NotImplementedError

  @abstractmethod
  def add_rendering(self, image_idx: int, rendering, progress: Progress):
    """Add a rendering to the controller."""
    raise NotImplementedError

  @abstractmethod
  def state_dict(self) -> dict:
    """Return controller state for checkpointing."""
    raise NotImplementedError


# ------------------------------------------------------------------------------------------------------------- disabled
class DisabledConfig(ControllerConfig):
  """controller/disabled.py:11-16."""

  def make_controller(self, scene, target_points: int, progress: Progress, logger=None) -> "DisabledController":
    return DisabledController(scene, logger)

  def from_state_dict(self, state_dict: dict, scene, target_points: int, progress: Progress, logger=None
                      ) -> "DisabledController":
    return self.make_controller(scene, target_points, progress, logger)


class DisabledController(Controller):
  """controller/disabled.py:20-38: gathers the statistics (for the histograms), never touches the scene."""

  def __init__(self, scene, logger=None):
    self.scene = scene
    self.logger = logger
    self.points = PointState.new_zeros(scene.num_points, device=scene.device)

  def __repr__(self):
    return f"DisabledController(points={self.points.prune_cost.shape[0]})"

  def step(self, progress: Progress, log_details: bool = False):
    if log_details and self.logger is not None:
      log_histograms(self.points, self.logger, "step")
    self.points = PointState.new_zeros(self.points.prune_cost.shape[0], device=self.points.prune_cost.device)

  def add_rendering(self, image_idx: int, rendering, progress: Progress):
    self.points.add_rendering(rendering)

  def state_dict(self) -> dict:
    return {}


# --------------------------------------------------------------------------------------------------------------- target
@dataclass
class TargetConfig(ControllerConfig):
  """target_controller.py:17-46 (the dataclass's defaults; config/controller/target.yaml's prune_rate 0.025 is the
  caller's to pass)."""
  prune_rate: float = 0.04                    # base rate (relative to count) to prune points
  target_count_t: float = 0.8                 # proportion of training when we hit the target count
  min_views: int = 5                          # times a point is in view before it may be pruned
  max_scale_px: float = 200                   # maximum screen-space size for a floater point (otherwise pruned)
  min_split_px: float = 0.0                   # minimum max-screen-space size for a point to be split
  densify_prune_interval: Schedule = 100

  def make_controller(self, scene, target_points: int, progress: Progress, logger=None) -> "TargetController":
    return TargetController(self, scene, target_points, progress, logger)

  def from_state_dict(self, state_dict: dict, scene, target_points: int, progress: Progress, logger=None
                      ) -> "TargetController":
    controller = TargetController(self, scene, target_points, progress, logger, start_points=state_dict["start_points"])
    load_point_state(controller.points, state_dict["points"])
    return controller


class TargetController(Controller):
  """target_controller.py:50-148: every ``densify_prune_interval`` steps, prune the cheapest points and the oversized
  ones and split the top-scored ones so that the count follows a smoothstep from ``start_points`` to ``target_points``."""

  def __init__(self, config: TargetConfig, scene, target_points: int, progress: Progress, logger=None,
               start_points: Optional[int] = None):
    self.config = config
    self.scene = scene
    self.logger = logger
    self.points = PointState.new_zeros(scene.num_points, device=scene.device)
    self.start_points = start_points or scene.num_points
    self.next_densify = self.find_next_densify(progress)
    self.max_points = target_points

  def __repr__(self):
    return f"TargetController(points={self.points.prune_cost.shape[0]})"

  def state_dict(self) -> dict:
    return dict(points=point_state_dict(self.points), start_points=self.start_points)

  def find_split_prune_indexes(self, t: float, target_points: int) -> Tuple[torch.Tensor, torch.Tensor]:
    c = self.config
    return find_split_prune_indexes(self.points, t, target_points, prune_rate=c.prune_rate, min_views=c.min_views,
                                    max_scale_px=c.max_scale_px, min_split_px=c.min_split_px)

  def find_next_densify(self, progress: Progress) -> Optional[int]:
    """target_controller.py:99-103."""
    interval = eval_schedule(self.config.densify_prune_interval, progress.t)
    next_densify = progress.step + interval
    return next_densify if next_densify + interval < progress.total_steps else None

  def target_points(self, progress: Progress) -> int:
    """target_controller.py:106-109."""
    target_step = self.config.target_count_t * progress.total_steps
    t = _clamp(progress.step / target_step, 0.0, 1.0)
    return int(smoothstep(t, self.start_points, self.max_points))

  @torch.no_grad()
  def step(self, progress: Progress, log_details: bool = False, generator: Optional[torch.Generator] = None):
    """target_controller.py:111-126.  ``generator`` (beyond the reference): passed on to ``scene.split_and_prune``."""
    if log_details and self.logger is not None:
      log_histograms(self.points, self.logger, "step")
    next_densify = self.next_densify
    if next_densify is not None and progress.step >= next_densify:
      split_mask, prune_mask = self.find_split_prune_indexes(progress.t, self.target_points(progress))
      densify_and_prune(self.points, self.scene, split_mask, prune_mask, self.logger, generator=generator)
      self.points = PointState.new_zeros(self.scene.num_points, device=self.scene.device)
      self.next_densify = self.find_next_densify(progress)

  def add_rendering(self, image_idx: int, rendering, progress: Progress):
    self.points.add_rendering(rendering)


# ----------------------------------------------------------------------------------------------------------------- mcmc
def _u64(name: str, v) -> int:
  v = int(v)
  if not 0 <= v < 2 ** 64:
    raise ValueError(f"{name} must be in [0, 2^64), got {v}")
  return v


@torch.no_grad()
def mcmc_noise(position: torch.Tensor, log_scaling: torch.Tensor, rotation: torch.Tensor, alpha_logit: torch.Tensor,
               points_in_view: torch.Tensor, *, min_views: int, opacity_threshold: float, noise_level: float, seed: int,
               step: int, margin: float = GATE_MARGIN, scale_eps: float = SCALE_EPS) -> torch.Tensor:
  """One noise step of the MCMC controller, IN PLACE on ``position`` (N, 3), which is returned: for every row with
  ``points_in_view > min_views``

      position += R(rotation / |rotation|) (max(exp(log_scaling), scale_eps) * (xi level))
      level = soft_lt(sigmoid(alpha_logit), opacity_threshold / 2, margin) noise_level

  with ``xi`` three standard normals drawn by Philox4x32-10 at key ``seed``, counter (row, ``step``): a row's noise
  depends on its own values, the seed, the step and its index alone.  Rows with too few views or with a level that
  underflows (opaque points) are not written.  One launch on the current stream, no host wait.  ``log_scaling`` (N, 3),
  ``rotation`` (N, 4) xyzw, ``alpha_logit`` (N, 1) or (N,) float32, ``points_in_view`` (N,) int16; contiguous device
  tensors, there is no CPU fallback."""
  n = int(require("position", position, shape=("N", 3)).shape[0])
  f32 = torch.float32
  for name, t, shape, dtype in (("position", position, (n, 3), f32), ("log_scaling", log_scaling, (n, 3), f32),
                                ("rotation", rotation, (n, 4), f32), ("alpha_logit", alpha_logit, [(n, 1), (n,)], f32),
                                ("points_in_view", points_in_view, (n,), torch.int16)):
    require(name, t, shape=shape, dtype=dtype, what="the MCMC noise step")
    on_one_device({"position": position, name: t})
  dev = position.device
  opacity_threshold, margin, noise_level, scale_eps = (float(opacity_threshold), float(margin), float(noise_level),
                                                       float(scale_eps))
  if not (opacity_threshold > 0 and margin >= 0 and noise_level >= 0 and scale_eps >= 0):
    raise ValueError(f"need opacity_threshold > 0 and margin, noise_level, scale_eps >= 0, got {opacity_threshold}, "
                     f"{margin}, {noise_level}, {scale_eps}")
  seed, step = _u64("seed", seed), _u64("step", step)
  if not position.is_contiguous():
    raise ValueError("position must be contiguous: it is updated in place")
  if n == 0:
    return position
  ls, rot, a, views = (t.detach().contiguous() for t in (log_scaling, rotation, alpha_logit, points_in_view))
  with _lib.on_device(dev) as stream:
    _lib.call("gsr_mcmc_noise", _ptr(position.detach()), _ptr(ls), _ptr(rot), _ptr(a), _ptr(views), n, int(min_views),
              opacity_threshold, margin, noise_level, scale_eps, seed, step, stream)
  return position


def mcmc_draws(num_points: int, seed: int, step: int, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
  """What ``mcmc_noise`` draws for the rows 0..num_points-1 at (seed, step), from the same device functions: the raw
  Philox words (N, 4), uint32 bit patterns held as int32, and the normals ``xi`` (N, 3) float32."""
  n = int(num_points)
  dev = torch.device(device)
  if dev.type != "cuda":
    raise _lib.GsplatHipError(f"mcmc_draws runs on the HIP device only, got {dev} (there is no CPU fallback)")
  with _lib.on_device(dev) as stream:
    dev = torch.device("cuda", torch.cuda.current_device())
    words = torch.empty(n, 4, dtype=torch.int32, device=dev)
    normals = torch.empty(n, 3, dtype=torch.float32, device=dev)
    _lib.call("gsr_mcmc_draws", n, _u64("seed", seed), _u64("step", step), _ptr(words), _ptr(normals), stream)
  return words, normals


# ----------------------------------------------------------------------------------------------------------- relocation
# The relocation move of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al., 2024), which the
# reference's mcmc_controller.py does not have: csrc/relocate.hip, arithmetic in csrc/gsr_relocate.h, contracts in
# include/gsplat_hip.h.  Every function enqueues on the current stream and waits for nothing, except where it says so.
RELOCATE_DOMAIN, GROW_DOMAIN = 1, 2           # the noise step is domain 0 of the same (seed, step)
_WHAT = "the MCMC relocation"


@torch.no_grad()
def relocate_weights(alpha_logit: torch.Tensor, alive: Optional[torch.Tensor] = None) -> torch.Tensor:
  """(N,) int32 draw weights: 0 where ``alive`` (bool, optional) is False, else ``max(1, floor(2^24 sigmoid(a)))`` with
  the sigmoid in fp64."""
  a = require("alpha_logit", alpha_logit, shape=[("N", 1), ("N",)], dtype=torch.float32, what=_WHAT)
  n = int(a.shape[0])
  if alive is not None:
    require("alive", alive, shape=(n,), dtype=torch.bool, what=_WHAT)
    on_one_device({"alpha_logit": a, "alive": alive})
    alive = alive.contiguous()
  with _lib.on_device(a.device) as stream:
    weights = torch.empty(n, dtype=torch.int32, device=a.device)
    _lib.call("gsr_relocate_weights", _ptr(a.detach().contiguous()), _ptr(alive), n, _ptr(weights), stream)
  return weights


@torch.no_grad()
def weighted_draws(weights: torch.Tensor, n: int, seed: int, step: int, domain: int
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
  """``n`` draws over the rows of ``weights`` (N,) -- uint32 values, held as int32 or uint32 bit patterns; 0 cannot be
  drawn -- with probability proportional to the weight: ``(sources (n,) int32, counts (N,) int32, total (1,) int64)``.
  Draw ``k`` is a function of (weights, seed, step, domain, k) alone: Philox4x32-10 at the counter
  (k, step, domain), ``t = floor(r S / 2^64)`` and the smallest row whose inclusive prefix sum exceeds ``t``; all
  integers, no generator state.  A total of 0 gives sources of -1 and counts of 0."""
  w = require("weights", weights, shape=("N",), what=_WHAT)
  if w.dtype not in (torch.int32, torch.uint32):
    raise ValueError(f"weights must be torch.int32 or torch.uint32, got {w.dtype}")
  N, n, domain = int(w.shape[0]), int(n), int(domain)
  if n < 0 or not 0 <= domain < 256:
    raise ValueError(f"need n >= 0 and a domain in [0, 256), got {n} and {domain}")
  seed, step = _u64("seed", seed), _u64("step", step)
  with _lib.on_device(w.device) as stream:
    sources = torch.empty(n, dtype=torch.int32, device=w.device)
    counts = torch.empty(N, dtype=torch.int32, device=w.device)
    total = torch.empty(1, dtype=torch.int64, device=w.device)
    ws = _lib.workspace(_lib.load().gsr_weighted_draws_workspace_bytes(N), w.device)
    _lib.call("gsr_weighted_draws", _ptr(w.contiguous()), N, n, seed, step, domain, _ptr(sources), _ptr(counts),
              _ptr(total), _ptr(ws), ws.numel(), stream)
  return sources, counts, total


@torch.no_grad()
def relocate_rescale(alpha_logit: torch.Tensor, log_scaling: torch.Tensor, counts: torch.Tensor, o_floor: float):
  """The correction of Eq. 9, IN PLACE on ``alpha_logit`` (N, 1) or (N,) and ``log_scaling`` (N, 3), for every row with
  ``counts`` (N,) int32 >= 1: the row and its ``counts`` copies, ``n = min(counts + 1, 51)`` Gaussians in all, get the
  opacity ``1 - (1 - o)^(1/n)`` (clamped to [o_floor, 1 - 2^-24]) and their scales the factor ``o / D``; fp64 inside."""
  a = require("alpha_logit", alpha_logit, shape=[("N", 1), ("N",)], dtype=torch.float32, what=_WHAT)
  n = int(a.shape[0])
  ls = require("log_scaling", log_scaling, shape=(n, 3), dtype=torch.float32, what=_WHAT)
  c = require("counts", counts, shape=(n,), dtype=torch.int32, what=_WHAT)
  on_one_device({"alpha_logit": a, "log_scaling": ls, "counts": c})
  if not (a.is_contiguous() and ls.is_contiguous()):
    raise ValueError("alpha_logit and log_scaling must be contiguous: they are updated in place")
  if not 0.0 < float(o_floor) < 1.0:
    raise ValueError(f"need 0 < o_floor < 1, got {o_floor}")
  with _lib.on_device(a.device) as stream:
    _lib.call("gsr_relocate_rescale", _ptr(a.detach()), _ptr(ls.detach()), _ptr(c.contiguous()), n, float(o_floor), stream)


@torch.no_grad()
def relocate_rows(columns, dst_rows: torch.Tensor, src_rows: torch.Tensor):
  """One launch over ``columns`` = [(tensor (N, ...), zero)]: for every k, row ``dst_rows[k]`` of a column with
  ``zero`` False takes row ``src_rows[k]``, and both rows of a column with ``zero`` True are zero-filled; IN PLACE.
  The dst rows must be unique and disjoint from the src rows.  A k with an index outside [0, N) is skipped."""
  dst = require("dst_rows", dst_rows, shape=("n",), dtype=torch.int32, what=_WHAT)
  src = require("src_rows", src_rows, shape=(int(dst.shape[0]),), dtype=torch.int32, what=_WHAT)
  if len(columns) > _lib.MAX_COLUMNS:
    raise ValueError(f"at most {_lib.MAX_COLUMNS} columns per call")
  if not columns:
    return
  N = int(columns[0][0].shape[0])
  arr = (_lib.GsrRowColumnC * len(columns))()
  for i, (t, zero) in enumerate(columns):
    if not (t.is_cuda and t.element_size() == 4 and t.is_contiguous() and t.shape[0] == N and t.device == dst.device):
      raise ValueError("columns must be contiguous CUDA tensors of 4-byte elements with the same number of rows, on the "
                       "device of the row lists")
    arr[i] = _lib.GsrRowColumnC(data=_ptr(t.detach()), width_dwords=max(t[0].numel(), 1) if N else 1, zero=int(bool(zero)))
  with _lib.on_device(dst.device) as stream:
    _lib.call("gsr_relocate_rows", _ptr(dst.contiguous()), _ptr(src.contiguous()), int(dst.shape[0]), N, arr, len(columns),
              stream)


def _optimizer_columns(points):
  """The optimizer-state columns of a ``ParameterClass``."""
  st = points._state
  return [st["step"], st["vis_avg"]] + [v for g in st["groups"].values() for v in g.values()]


@torch.no_grad()
def relocate_points(points, state: PointState, dead_mask: torch.Tensor, o_floor: float, seed: int, step: int) -> int:
  """Teleports the rows of ``dead_mask`` (N,) bool onto live rows drawn with probability proportional to opacity, IN
  PLACE on the tensors and the optimizer state of ``points`` (a ``ParameterClass``) and on ``state``; returns the
  number of dead rows.  The row count does not change.

  weights (0 for a dead row) -> one draw per dead row at (seed, step, domain 1) -> the opacity / scale correction of
  every drawn source for itself and its copies -> one launch that gives every dead row its source's NEW row in every
  column and zero-fills the optimizer state of both.  The dead rows of ``state`` are zeroed, as children start from zero
  in ``densify_and_prune``; the sources keep theirs.  One host wait: the dead count."""
  from .densify import compact_rows
  n = points.num_points
  dead = require("dead_mask", dead_mask, shape=(n,), dtype=torch.bool, what=_WHAT)
  dev = points.device
  rows = torch.arange(n, dtype=torch.int32, device=dev)
  dead_rows, = compact_rows(dead, [(rows, None)], n_tail=0)              # (the wait: the count sizes the list)
  n_dead = int(dead_rows.shape[0])
  if n_dead == 0:
    return 0
  weights = relocate_weights(points.alpha_logit, alive=~dead)
  sources, counts, _ = weighted_draws(weights, n_dead, seed, step, RELOCATE_DOMAIN)
  relocate_rescale(points.alpha_logit, points.log_scaling, counts, o_floor)
  columns = [(t, False) for t in points.tensors.values()] + [(t, True) for t in _optimizer_columns(points)]
  relocate_rows(columns, dead_rows, sources)
  for _, v in _columns(state):
    v.masked_fill_(dead, 0)
  return n_dead


@torch.no_grad()
def grow_points(points, state: PointState, n_new: int, o_floor: float, seed: int, step: int):
  """``n_new`` copies of rows drawn over ALL rows at (seed, step, domain 2), appended: ``(points, state)``, new objects
  with N + n_new rows.  The sources are corrected in place first, so a copy equals its source's new row; the appended
  rows get fresh optimizer state and zero ``PointState`` rows."""
  n, n_new = points.num_points, int(n_new)
  if n_new <= 0 or n == 0:
    return points, state
  sources, counts, _ = weighted_draws(relocate_weights(points.alpha_logit), n_new, seed, step, GROW_DOMAIN)
  relocate_rescale(points.alpha_logit, points.log_scaling, counts, o_floor)
  idx = sources.to(torch.int64)              # (every row is alive and weighs 1 or more: no source is -1)
  keep = torch.ones(n, dtype=torch.bool, device=points.device)
  grown = points.keep_and_append(keep, {k: t.detach()[idx] for k, t in points.tensors.items()})
  return grown, PointState(**{k: torch.cat([v, v.new_zeros(n_new)]) for k, v in _columns(state)})


def growth_target(num_points: int, target_points: int, grow_rate: float) -> int:
  """``min(target_points, ceil((1 + grow_rate) N))``, never below N; the rate is read as the nearest fraction with a
  denominator up to 10^6, so that 0.05 of 300 is 15 and not 15.000000000000002."""
  n = int(num_points)
  return max(n, min(int(target_points), n + math.ceil(Fraction(float(grow_rate)).limit_denominator(10 ** 6) * n)))


@dataclass
class MCMCConfig(ControllerConfig):
  """mcmc_controller.py:24-50 without ``max_prune_rate`` (read nowhere there) and with ``seed``, the key of the noise.
  ``relocate`` (beyond the reference) replaces the prune-and-split round by the paper's relocation move and a growth
  of ``grow_rate`` per round towards ``target_points``."""
  opacity_threshold: float = 0.1
  prune_interval: int = 50
  min_views: int = 5
  max_scale_px: float = 200
  min_split_px: float = 0.0
  noise_level: Schedule = 100.0
  seed: int = 0
  relocate: bool = False
  grow_rate: float = 0.05

  def make_controller(self, scene, target_points: int, progress: Progress, logger=None) -> "MCMCController":
    return MCMCController(self, scene, target_points, progress, logger)

  def from_state_dict(self, state_dict: dict, scene, target_points: int, progress: Progress, logger=None
                      ) -> "MCMCController":
    controller = MCMCController(self, scene, target_points, progress, logger)
    load_point_state(controller.points, state_dict["points"])
    return controller


class MCMCController(Controller):
  """mcmc_controller.py:54-112.  Every ``prune_interval`` steps: prune the oversized and the nearly transparent points
  and split as many top-scored ones (never a pruned one: the count falls by the overlap the reference's unstable sort
  may produce); the statistics are carried across the round, the children start from zero.  With ``config.relocate``
  that step is ``relocate_round`` instead: nothing is deleted, the dead rows move onto live ones.  Every other step: the
  native noise step on ``scene.points.position`` in place -- the reference's own code perturbs a copy (a bool-mask
  index), so its noise never reaches the scene; see the module docstring."""

  def __init__(self, config: MCMCConfig, scene, target_points: int, progress: Progress, logger=None):
    self.config = config
    self.scene = scene
    self.logger = logger
    self.target_points = target_points
    self.points = PointState.new_zeros(scene.num_points, device=scene.device)
    self.num_points = scene.num_points

  def __repr__(self):
    return f"MCMCController(points={self.points.prune_cost.shape[0]})"

  def state_dict(self) -> dict:
    return {"points": point_state_dict(self.points)}

  def find_split_prune_masks(self) -> Tuple[torch.Tensor, torch.Tensor]:
    """mcmc_controller.py:77-87 with ties to the lowest index (``take_n``) and no pruned row split."""
    c, state = self.config, self.points
    opacity = torch.sigmoid(self.scene.points.alpha_logit.detach()).reshape(-1)
    prune_mask = (state.max_scale_px > c.max_scale_px) | (opacity < c.opacity_threshold)
    n = int(prune_mask.sum().item())
    too_small = state.max_scale_px < c.min_split_px
    split_score = torch.where(prune_mask | too_small, torch.zeros_like(state.split_score), state.split_score)
    split_mask = take_n(split_score, n, descending=True) & ~prune_mask
    return split_mask, prune_mask

  @torch.no_grad()
  def relocate_round(self, progress: Progress):
    """``MCMCConfig.relocate``: the dead rows -- oversized or below ``opacity_threshold`` -- are relocated onto live
    ones, then the count grows to ``growth_target``.  Both moves draw at (``config.seed``, ``progress.step``), in their
    own domains, so replicas with equal parameters make equal moves.  ``scene.points`` must be a ``ParameterClass``."""
    c, scene = self.config, self.scene
    opacity = torch.sigmoid(scene.points.alpha_logit.detach()).reshape(-1)
    dead = (self.points.max_scale_px > c.max_scale_px) | (opacity < c.opacity_threshold)
    n = scene.num_points
    n_dead = relocate_points(scene.points, self.points, dead, c.opacity_threshold, c.seed, progress.step)
    n_new = growth_target(n, self.target_points, c.grow_rate) - n
    if n_new > 0:
      scene.points, self.points = grow_points(scene.points, self.points, n_new, c.opacity_threshold, c.seed, progress.step)
    self.num_points = scene.num_points
    if self.logger is not None:
      self.logger.log_values("relocate", dict(n=n, dead=n_dead, grown=max(n_new, 0)))

  @torch.no_grad()
  def step(self, progress: Progress, log_details: bool = False, generator: Optional[torch.Generator] = None):
    """``generator`` (beyond the reference): passed on to ``scene.split_and_prune`` on a prune step."""
    c = self.config
    if log_details and self.logger is not None:
      log_histograms(self.points, self.logger, "step")
    if progress.step % c.prune_interval == 0 and c.relocate:
      self.relocate_round(progress)
    elif progress.step % c.prune_interval == 0:
      split_mask, prune_mask = self.find_split_prune_masks()
      self.points = densify_and_prune(self.points, self.scene, split_mask, prune_mask, logger=self.logger,
                                      generator=generator)
      self.num_points = self.scene.num_points
    else:
      p = self.scene.points
      mcmc_noise(p.position, p.log_scaling, p.rotation, p.alpha_logit, self.points.points_in_view,
                 min_views=c.min_views, opacity_threshold=c.opacity_threshold,
                 noise_level=eval_schedule(c.noise_level, progress.t), seed=c.seed, step=progress.step)

  def add_rendering(self, image_idx: int, rendering, progress: Progress):
    self.points.add_rendering(rendering)
