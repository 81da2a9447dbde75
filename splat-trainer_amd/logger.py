"""The reference's logging layer (``splat_trainer.logger.logger``): the abstract ``Logger``, ``NullLogger``,
``CompositeLogger``, the two in-memory loggers ``StateLogger`` (last value per path, with the step it was logged at) and
``HistoryLogger`` (every value per path), and ``LoggerWithState``, which the trainer reads its progress line and its
evaluation metrics back from.  Paths are ``"a/b/c"`` strings into a ``StateTree``.

``log_histogram`` takes a tensor or a ``Histogram`` (histogram.py).  The tensorboard and wandb writers are not here:
their packages are no dependency of this one.  ``LoggerWithState.get_value`` works (the reference's calls a method that
``StateLogger`` does not have).
"""
from __future__ import annotations

from abc import ABCMeta, abstractmethod
from typing import Any, Dict, Optional, Union

import torch

from .histogram import Histogram


class Logger(metaclass=ABCMeta):
  """What the trainer, the scene and the controllers log through."""

  @abstractmethod
  def step(self, progress):
    ...

  @abstractmethod
  def log_evaluations(self, name: str, data: Dict[str, Dict]):
    ...

  @abstractmethod
  def log_config(self, config: dict):
    ...

  @abstractmethod
  def log_image(self, name: str, image: torch.Tensor, compressed: bool = True, caption: Optional[str] = None):
    ...

  @abstractmethod
  def log_cloud(self, name: str, points):
    ...

  @abstractmethod
  def log_values(self, name: str, data: dict):
    ...

  @abstractmethod
  def log_value(self, name: str, value: float):
    ...

  @abstractmethod
  def log_histogram(self, name: str, values: Union[torch.Tensor, Histogram], num_bins: Optional[int] = None):
    ...

  @abstractmethod
  def log_json(self, name: str, data: dict):
    ...

  @abstractmethod
  def close(self):
    ...


class NullLogger(Logger):
  """Every method does nothing; the base of the loggers that care about a few."""

  def step(self, progress):
    pass

  def log_evaluations(self, name, data):
    pass

  def log_config(self, config):
    pass

  def log_image(self, name, image, compressed=True, caption=None):
    pass

  def log_cloud(self, name, points):
    pass

  def log_values(self, name, data):
    pass

  def log_value(self, name, value):
    pass

  def log_histogram(self, name, values, num_bins=None):
    pass

  def log_json(self, name, data):
    pass

  def close(self):
    pass


class CompositeLogger(Logger):
  """Forwards every call to each of its loggers, in order."""

  def __init__(self, *loggers: Logger):
    for logger in loggers:
      if not isinstance(logger, Logger):
        raise TypeError(f"CompositeLogger takes Logger instances, got {type(logger).__name__}")
    self.loggers = list(loggers)

  def add_logger(self, logger: Logger) -> "CompositeLogger":
    self.loggers.append(logger)
    return self

  def _forward(self, method, *args, **kwargs):
    for logger in self.loggers:
      getattr(logger, method)(*args, **kwargs)

  def step(self, progress):
    self._forward("step", progress)

  def log_evaluations(self, name, data):
    self._forward("log_evaluations", name, data)

  def log_config(self, config):
    self._forward("log_config", config)

  def log_image(self, name, image, compressed=True, caption=None):
    self._forward("log_image", name, image, compressed=compressed, caption=caption)

  def log_cloud(self, name, points):
    self._forward("log_cloud", name, points)

  def log_values(self, name, data):
    self._forward("log_values", name, data)

  def log_value(self, name, value):
    self._forward("log_value", name, value)

  def log_histogram(self, name, values, num_bins=None):
    self._forward("log_histogram", name, values, num_bins=num_bins)

  def log_json(self, name, data):
    self._forward("log_json", name, data)

  def close(self):
    self._forward("close")


class StepValue:
  """A logged value and the step it was logged at."""

  def __init__(self, step: int, value: Any):
    self.step = step
    self.value = value

  def __repr__(self):
    return f"StepValue(step={self.step}, value={self.value!r})"


def _parts(path: str) -> list:
  return path.split("/")


class StateTree:
  """A tree of dictionaries addressed by ``"a/b/c"`` paths; the leaves are whatever is stored."""

  def __init__(self):
    self.data: Dict[str, Any] = {}

  def __getitem__(self, key: str):
    return self.data[key]

  def __setitem__(self, key: str, value):
    self.data[key] = value

  def __contains__(self, key: str) -> bool:
    return key in self.data

  def items(self):
    return self.data.items()

  def keys(self):
    return self.data.keys()

  def values(self):
    return self.data.values()

  def __repr__(self):
    return f"StateTree({', '.join(self.data)})"

  def get_path(self, path: str):
    """The node or leaf at ``path``; ValueError when a part is missing or a leaf is in the way."""
    node = self
    for part in _parts(path):
      if not isinstance(node, StateTree):
        raise ValueError(f"path {path}: {part} lies below a leaf")
      if part not in node:
        raise ValueError(f"path {path}: {part} not in {node}")
      node = node[part]
    return node

  def has_path(self, path: str) -> bool:
    try:
      self.get_path(path)
      return True
    except ValueError:
      return False

  def get_leaf(self, path: str):
    leaf = self.get_path(path)
    if isinstance(leaf, StateTree):
      raise ValueError(f"path {path}: not a leaf")
    return leaf

  def get_or_insert_path(self, path: str) -> "StateTree":
    """The node at ``path``, with every missing node on the way made."""
    node = self
    for part in _parts(path):
      if part not in node:
        node[part] = StateTree()
      node = node[part]
      if not isinstance(node, StateTree):
        raise ValueError(f"path {path}: {part} is a leaf")
    return node

  def update_leaf(self, path: str, default, update_fn):
    """leaf = update_fn(leaf, or ``default`` when there is none yet); returns the new leaf."""
    *parents, last = _parts(path)
    node = self.get_or_insert_path("/".join(parents)) if parents else self
    node[last] = update_fn(node[last] if last in node else default)
    return node[last]

  def set_leaf(self, path: str, value):
    return self.update_leaf(path, value, lambda _: value)

  def flatten(self) -> Dict[str, Any]:
    """{path: leaf} over the whole tree."""
    flat = {}

    def walk(prefix, node):
      for key, value in node.items():
        path = f"{prefix}/{key}" if prefix else key
        if isinstance(value, StateTree):
          walk(path, value)
        else:
          flat[path] = value
    walk("", self)
    return flat


class _TreeLogger(NullLogger):
  def __init__(self):
    self.tree = StateTree()

  def __getitem__(self, path: str):
    return self.tree.get_path(path)

  def __contains__(self, path: str) -> bool:
    return self.tree.has_path(path)

  def flatten(self) -> dict:
    return self.tree.flatten()


class StateLogger(_TreeLogger):
  """Keeps the last value logged under each path as a ``StepValue``."""

  def __init__(self):
    super().__init__()
    self.current_step = 0

  def step(self, progress):
    self.current_step = progress.step

  def log_config(self, config: dict):
    self.tree["config"] = config

  def log_values(self, name: str, data: dict):
    node = self.tree.get_or_insert_path(name)
    for key, value in data.items():
      node[key] = StepValue(self.current_step, value)

  def log_value(self, name: str, value):
    self.tree.set_leaf(name, StepValue(self.current_step, value))

  def get_value(self, path: str, default: Any = None) -> Any:
    """The value last logged at ``path``, or ``default`` when there is none (or ``path`` is not a leaf)."""
    if path not in self:
      return default
    leaf = self[path]
    return leaf.value if isinstance(leaf, StepValue) else default


class HistoryLogger(_TreeLogger):
  """Keeps every value logged under each path, in order."""

  def log_values(self, name: str, data: dict):
    node = self.tree.get_or_insert_path(name)
    for key, value in data.items():
      node[key] = (node[key] if key in node else []) + [value]

  def log_value(self, name: str, value):
    self.tree.update_leaf(name, [], lambda values: values + [value])


class LoggerWithState(CompositeLogger):
  """``logger`` with a ``StateLogger`` in front of it, so what was logged can be read back."""

  def __init__(self, logger: Logger):
    self.state = StateLogger()
    self.logger = logger
    super().__init__(self.state, logger)

  def get_value(self, path: str, default: Any = None) -> Any:
    return self.state.get_value(path, default)

  def __getitem__(self, path: str):
    return self.state[path]

  def __contains__(self, path: str) -> bool:
    return path in self.state
