"""The host side of the trainer layer: the logger trees, the dataset helpers and ``TensorDataset``, ``PointCloud``,
``TargetOverlap`` on a stub clustering, checkpoint discovery on a temporary directory, and the abort rules of
``Trainer.checkpoint`` with a stubbed ``evaluate``.  Nothing here needs a GPU."""
import math

import numpy as np
import pytest
import torch

import splat_trainer_amd as sta
from splat_trainer_amd import ply_io
from splat_trainer_amd.trainer import _Prefetcher


# --------------------------------------------------------------------------------------------------------------- loggers
def test_state_tree_paths():
  tree = sta.StateTree()
  tree.set_leaf("a/b/c", 1)
  tree.set_leaf("a/d", 2)
  assert tree.update_leaf("a/b/c", 0, lambda v: v + 10) == 11 and tree.update_leaf("e", 5, lambda v: v * 2) == 10
  assert tree.get_path("a/b/c") == 11 and tree.get_leaf("a/d") == 2 and isinstance(tree.get_path("a/b"), sta.StateTree)
  assert tree.has_path("a/b") and not tree.has_path("a/x") and not tree.has_path("a/d/deeper")
  assert "a" in tree and "b" not in tree and "b" in tree["a"]
  assert tree.flatten() == {"a/b/c": 11, "a/d": 2, "e": 10}
  assert tree.get_or_insert_path("f/g").data == {} and tree.has_path("f/g")
  with pytest.raises(ValueError):
    tree.get_leaf("a/b")
  with pytest.raises(ValueError):
    tree.get_path("a/d/deeper")
  with pytest.raises(ValueError):
    tree.get_or_insert_path("a/d/deeper")


def test_state_and_history_loggers():
  state, history = sta.StateLogger(), sta.HistoryLogger()
  both = sta.CompositeLogger(state, history)
  both.log_values("train/loss", dict(l1=0.5, total=1.5))
  both.step(sta.Progress(step=7, total_steps=10))
  both.log_value("train/loss/l1", 0.25)
  both.log_value("eval_train/psnr", 20.0)
  both.log_config(dict(a=1))
  both.log_histogram("h", torch.zeros(3))
  both.log_histogram("h", sta.Histogram(torch.zeros(3)), num_bins=4)
  both.log_image("i", torch.zeros(2, 2, 3))
  both.log_json("j", {})
  both.log_evaluations("e", {})
  both.log_cloud("c", None)
  both.close()
  assert "train/loss" in state and "train/loss/l1" in state and "train" in state and "nothing/here" not in state
  assert state["train/loss/l1"].value == 0.25 and state["train/loss/l1"].step == 7 and state["train/loss/total"].step == 0
  assert sorted(state["train/loss"].keys()) == ["l1", "total"]
  assert history["train/loss/l1"] == [0.5, 0.25] and history["train/loss/total"] == [1.5] and "eval_train/psnr" in history
  assert {k: v.value for k, v in state.flatten().items() if k != "config"} == {"train/loss/l1": 0.25, "train/loss/total": 1.5,
                                                                               "eval_train/psnr": 20.0}
  assert state.tree["config"] == dict(a=1)
  assert history.flatten() == {"train/loss/l1": [0.5, 0.25], "train/loss/total": [1.5], "eval_train/psnr": [20.0]}


def test_logger_with_state_reads_back():
  history = sta.HistoryLogger()
  logger = sta.LoggerWithState(history)
  logger.step(sta.Progress(step=3, total_steps=10))
  logger.log_values("densify", dict(n=100, split=4))
  logger.log_value("train/step_rate", 12.5)
  assert logger.get_value("densify/n") == 100 and logger.get_value("train/step_rate") == 12.5
  assert logger.get_value("densify/missing", -1) == -1 and logger.get_value("densify", "node") == "node"
  assert "densify" in logger and "densify/split" in logger and "other" not in logger
  assert logger["densify/split"].value == 4 and logger["densify/split"].step == 3
  assert history["densify/n"] == [100]
  assert isinstance(logger, sta.Logger) and isinstance(sta.NullLogger(), sta.Logger)
  with pytest.raises(TypeError):
    sta.Logger()
  with pytest.raises(TypeError):
    sta.CompositeLogger(object())


# -------------------------------------------------------------------------------------------------------------- datasets
def test_split_every_and_expand_index():
  train, val = sta.split_every(10, test_every=4)
  assert train.tolist() == [1, 2, 3, 5, 6, 7, 9] and val.tolist() == [0, 4, 8]
  train, val = sta.split_every(10, test_every=3, padding=2)
  assert val.tolist() == [2, 5] and train.tolist() == [2, 4, 5, 7]                   # (by value: the reference's rule)
  train, val = sta.split_every(5, test_every=0)
  assert train.tolist() == [0, 1, 2, 3, 4] and val.tolist() == [] and val.dtype is torch.int64
  train, val = sta.partition_stride(torch.arange(6), 2)
  assert train.tolist() == [1, 3, 5] and val.tolist() == [0, 2, 4]
  with pytest.raises(ValueError):
    sta.partition_stride(torch.arange(6), 0)
  assert sta.expand_index(torch.tensor([0, 2, 5]), 3).tolist() == [0, 1, 2, 6, 7, 8, 15, 16, 17]
  assert sta.expand_index(torch.tensor([4]), 1).tolist() == [4] and sta.expand_index(torch.zeros(0, dtype=torch.long), 2).tolist() == []


def _table(n=5, labels=(2, 2, 1, 2, 3)):
  eye = torch.eye(4).repeat(n, 1, 1)
  eye[:, 2, 3] = torch.arange(n, dtype=torch.float32) + 3.0
  projection = sta.Projections(intrinsics=torch.tensor([[60.0, 60.0, 16.0, 12.0]]), image_size=torch.tensor([[32, 24]]),
                               depth_range=torch.tensor([[0.1, 100.0]]))
  return sta.MultiCameraTable(camera_t_world=eye, camera_idx=torch.zeros(n, dtype=torch.int64), projection=projection,
                              image_names=[f"im{i}.png" for i in range(n)], labels=torch.tensor(labels))


def test_tensor_dataset():
  images = [torch.full((24, 32, 3), i, dtype=torch.uint8) for i in range(5)]
  cloud = sta.PointCloud(torch.randn(7, 3), torch.rand(7, 3))
  norm = sta.Normalization(config=sta.NormalizationConfig(), translation=torch.tensor([1.0, 2.0, 3.0]), scaling=0.5)
  data = sta.TensorDataset(_table(), images, cloud=cloud, normalization=norm)
  assert isinstance(data, sta.Dataset) and data.train_idx.tolist() == [0, 1, 3, 4] and data.val_idx.tolist() == [2, 4]
  views = data.train(shuffle=False)
  assert [v.image_idx for v in views] == [0, 1, 3, 4] and views[2].filename == "im3.png" and views[2].image is images[3]
  assert sorted(v.image_idx for v in data.train()) == [0, 1, 3, 4] and [v.image_idx for v in data.val()] == [2, 4]
  assert [v.image_idx for v in data.loader(torch.tensor([4, 0]))] == [4, 0]
  assert data.pointcloud() is cloud and data.camera_table.num_images == 5 and data.load_images() is None
  back = data.to_original
  assert back.scaling == 2.0 and torch.allclose(back.transform_points(norm.transform_points(cloud.points)), cloud.points, atol=1e-6)
  assert sta.TensorDataset(_table(), images, train_idx=torch.tensor([1, 2])).train_idx.tolist() == [1, 2]
  with pytest.raises(ValueError):
    sta.TensorDataset(_table(), images[:4])
  with pytest.raises(ValueError):
    sta.TensorDataset(_table(), [im.float() for im in images])


def test_point_cloud(tmp_path):
  cloud = sta.PointCloud(torch.arange(12, dtype=torch.float32).reshape(4, 3), torch.tensor([[0.0, 0.5, 1.0]] * 4), batch_size=(4,))
  assert cloud.num_points == 4 and cloud.batch_size == (4,) and len(cloud) == 4 and cloud.device.type == "cpu"
  assert cloud[torch.tensor([True, False, True, False])].points[:, 0].tolist() == [0.0, 6.0]
  assert cloud[torch.tensor([3, 0])].points[:, 0].tolist() == [9.0, 0.0] and cloud[1].num_points == 1 and cloud[1:3].num_points == 2
  assert cloud.to("cpu").num_points == 4 and cloud.append(cloud).num_points == 8
  assert cloud.translated(torch.ones(3)).scaled(2.0).points[0].tolist() == [2.0, 4.0, 6.0]
  cloud.save_ply(tmp_path / "cloud.ply")
  vertex = ply_io.read_ply(tmp_path / "cloud.ply")
  assert vertex.dtype.names == ("x", "y", "z", "red", "green", "blue") and vertex["z"].tolist() == [2.0, 5.0, 8.0, 11.0]
  assert vertex["green"].tolist() == [127.0] * 4 and vertex["blue"].tolist() == [255.0] * 4
  again = sta.PointCloud.load_ply(tmp_path / "cloud.ply")
  assert torch.equal(again.points, cloud.points) and torch.allclose(again.colors, cloud.colors, atol=1 / 255)
  from_np = sta.PointCloud.from_numpy(np.zeros((2, 3)), np.full((2, 3), 255, np.uint8))
  assert from_np.colors.tolist() == [[1.0] * 3] * 2 and from_np.points.dtype is torch.float32
  with pytest.raises(ValueError):
    sta.PointCloud(torch.zeros(3, 3), torch.zeros(2, 3))


def test_scaled_pointcloud_to_gaussians_and_back():
  cloud = sta.PointCloud(torch.randn(6, 3), torch.rand(6, 3))
  make = lambda seed: sta.from_scaled_pointcloud(cloud, torch.full((6,), 0.5), initial_alpha=0.5,
                                                 generator=torch.Generator().manual_seed(seed))
  g = make(1)
  assert torch.equal(g.position, cloud.points) and torch.equal(g.feature, cloud.colors) and g.batch_size == (6,)
  assert torch.allclose(g.log_scaling, torch.full((6, 3), math.log(0.5))) and torch.allclose(g.rotation.norm(dim=1), torch.ones(6))
  assert torch.allclose(torch.sigmoid(g.alpha_logit), torch.full((6, 1), 0.5 - 1e-4), atol=1e-6)
  assert torch.equal(make(1).rotation, g.rotation) and not torch.equal(make(2).rotation, g.rotation)
  back = sta.to_pointcloud(g)
  assert torch.equal(back.points, cloud.points) and torch.equal(back.colors, cloud.colors)
  config = sta.CloudInitConfig(num_neighbors=3, initial_point_scale=0.5, initial_alpha=0.5)
  assert config.limit_points is None and config.initial_points is None and config.min_view_overlap == 4 and config.clamp_near == 0.0


# --------------------------------------------------------------------------------------------------------- TargetOverlap
class _StubClustering:
  """Eight views on a line: the overlap of two views falls with their distance."""

  def __init__(self, n=8):
    feature = torch.stack([torch.exp(-0.5 * ((torch.arange(16.0) - 2.0 * i) / 3.0) ** 2) for i in range(n)])
    self.normalized_visibility = torch.nn.functional.normalize(feature, dim=1)

  def overlaps_with(self, vec):
    return vec @ self.normalized_visibility.T


def test_target_overlap_uses_every_view_before_any_twice():
  torch.manual_seed(4)
  config = sta.TargetOverlapConfig(batch_size=3, history_size=4)
  assert (config.overlap_temperature, config.target_overlap) == (0.5, 0.5) and sta.TargetOverlapConfig().batch_size == 1
  train_idx = torch.arange(8)
  sampler = config.create(train_idx)
  assert sampler.history_idx.shape == (4,) and sampler.available_mask.all()
  clustering = _StubClustering()
  first, second = sampler.select_images(clustering), sampler.select_images(clustering)
  assert len(set(first.tolist()) | set(second.tolist())) == 6 and int(sampler.available_mask.sum()) == 2
  assert sampler.history_idx.tolist() == (second.tolist() + first.tolist())[:4]      # the newest batch first, length held
  third = sampler.select_images(clustering)                                          # two views left for a batch of three: refill
  assert len(set(third.tolist())) == 3 and int(sampler.available_mask.sum()) == 5
  assert sampler.history_idx.tolist() == (third.tolist() + second.tolist())[:4]
  for _ in range(20):
    batch = sampler.select_images(clustering, sta.Progress(1, 10))
    assert len(set(batch.tolist())) == 3 and sampler.history_idx.shape == (4,) and not sampler.available_mask[batch].any()


def test_target_overlap_maps_through_train_idx_and_round_trips():
  torch.manual_seed(5)
  config = sta.TargetOverlapConfig(batch_size=2, history_size=2, overlap_temperature=0.0)
  train_idx = torch.tensor([1, 3, 4, 6, 7])
  sampler, clustering = config.create(train_idx), _StubClustering(5)      # one row per training view
  seen = []
  for _ in range(2):
    seen += sampler.select_images(clustering).tolist()
  assert len(set(seen)) == 4 and set(seen) <= set(train_idx.tolist())
  state = sampler.state_dict()
  assert sorted(state) == ["available_mask", "history_idx"]
  copy = config.from_state_dict({k: v.clone() for k, v in state.items()}, train_idx)
  assert torch.equal(copy.history_idx, sampler.history_idx) and torch.equal(copy.available_mask, sampler.available_mask)
  assert sampler.select_images(clustering).tolist() == copy.select_images(clustering).tolist()        # temperature 0: top-k
  assert torch.equal(copy.history_idx, sampler.history_idx) and torch.equal(copy.available_mask, sampler.available_mask)


# ----------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_discovery(tmp_path):
  with pytest.raises(FileNotFoundError):
    sta.find_checkpoint(tmp_path)
  folder = tmp_path / "checkpoint"
  folder.mkdir()
  for step in (5, 100, 20):
    torch.save(dict(step=step, scene=dict(w=torch.full((2,), float(step)))), folder / f"checkpoint_{step}.pt")
  (folder / "notes.txt").write_text("not a checkpoint")
  (folder / "checkpoint_final.pt").write_text("no number")
  assert sta.find_checkpoint(tmp_path).name == "checkpoint_100.pt" and sta.find_checkpoint(tmp_path, 20).name == "checkpoint_20.pt"
  with pytest.raises(FileNotFoundError, match=r"\[5, 20, 100\]"):
    sta.find_checkpoint(tmp_path, 7)
  state, workspace = sta.load_checkpoint(tmp_path)
  assert state["step"] == 100 and workspace == tmp_path and state["scene"]["w"].tolist() == [100.0, 100.0]
  state, workspace = sta.load_checkpoint(tmp_path, 5)
  assert state["step"] == 5
  state, workspace = sta.load_checkpoint(folder / "checkpoint_20.pt")
  assert state["step"] == 20 and workspace == tmp_path
  with pytest.raises(FileNotFoundError):
    sta.load_checkpoint(tmp_path / "missing.pt")


# ----------------------------------------------------------------------------------------------------------- abort rules
class _StubScene:
  num_points = 3

  def __init__(self):
    self.weights = torch.zeros(3)
    self.checkpoints_logged = 0

  def state_dict(self):
    return dict(points=dict(position=self.weights))

  def log_checkpoint(self, logger, progress=None):
    self.checkpoints_logged += 1


class _StubController:
  def state_dict(self):
    return {}


def _stub_trainer(tmp_path, ssims, **config):
  images = [torch.zeros(24, 32, 3, dtype=torch.uint8) for _ in range(5)]
  train_config = sta.TrainConfig(scene=None, controller=None, view_selection=sta.RandomSamplerConfig(batch_size=1),
                                 cloud_init=sta.CloudInitConfig(num_neighbors=3, initial_point_scale=0.5, initial_alpha=0.5),
                                 total_steps=100, eval_steps=10, target_points=10, device="cpu", save_output=False,
                                 output_path=str(tmp_path), **config)
  data = sta.TensorDataset(_table(), images)
  trainer = sta.Trainer(train_config, _StubScene(), _StubController(), data, sta.LoggerWithState(sta.NullLogger()),
                        train_config.view_selection.create(torch.arange(5)))
  values = iter(ssims)
  trainer.evaluate = lambda: dict(train_ssim=next(values), train_psnr=20.0)
  return trainer


def test_train_config_defaults():
  trainer_fields = sta.TrainConfig.__dataclass_fields__
  defaults = {k: f.default for k, f in trainer_fields.items()}
  assert defaults["log_interval"] == 10 and defaults["densify_interval"] == 100 and defaults["max_ssim_regression"] == 0.04
  assert defaults["num_logged_images"] == 8 and defaults["log_worst_images"] == 2 and defaults["log_details"] is False
  assert (defaults["ssim_weight"], defaults["mse_weight"], defaults["l1_weight"], defaults["ssim_levels"]) == (0.0, 0.0, 0.0, 4)
  assert defaults["vis_clusters"] == 1024 and defaults["antialias"] is False and defaults["blur_cov"] == 0.3
  assert defaults["save_checkpoints"] is False and defaults["save_output"] is True and defaults["log_images"] is True
  assert defaults["min_step_rate"] is None


def test_checkpoint_aborts_below_the_first_evaluation(tmp_path):
  trainer = _stub_trainer(tmp_path, [0.5, 0.6, 0.45])
  trainer.checkpoint()
  trainer.step = 10
  trainer.checkpoint()
  assert [e["train_ssim"] for e in trainer.evaluation_log] == [0.5, 0.6] and [e["step"] for e in trainer.evaluation_log] == [0, 10]
  assert trainer.last_checkpoint == 10 and trainer.scene.checkpoints_logged == 2
  with pytest.raises(sta.NoProgressException, match="untrained"):
    trainer.checkpoint()
  assert len(trainer.evaluation_log) == 2


def test_checkpoint_aborts_on_a_regression(tmp_path):
  trainer = _stub_trainer(tmp_path, [0.5, 0.7, 0.67, 0.62], max_ssim_regression=0.04)
  for _ in range(3):                                      # 0.7 -> 0.67 is inside the allowance
    trainer.checkpoint()
  with pytest.raises(sta.NoProgressException, match="regression"):
    trainer.checkpoint()                                  # 0.67 -> 0.62 is not
  assert issubclass(sta.NoProgressException, sta.TrainingException) and issubclass(sta.NaNParameterException, sta.TrainingException)
  assert issubclass(sta.TrainingTimeoutException, sta.TrainingException)


def test_checkpoint_refuses_non_finite_parameters(tmp_path):
  trainer = _stub_trainer(tmp_path, [0.5])
  trainer.scene.weights[1] = float("nan")
  with pytest.raises(sta.NaNParameterException, match="position"):
    trainer.checkpoint()
  assert trainer.evaluation_log == []


def test_state_dict_of_a_fresh_trainer(tmp_path):
  trainer = _stub_trainer(tmp_path, [0.5])
  trainer.checkpoint()
  state = trainer.state_dict()
  assert state["view_clustering"] is None and state["evaluation_log"] == [dict(step=0, train_ssim=0.5, train_psnr=20.0)]
  assert state["step"] == 0 and state["pending_batches"] == [] and sorted(state["view_selection"]) == ["next"]
  assert trainer.is_logging_step and trainer.progress == sta.Progress(0, 100, True) and not trainer.is_training()
  calls = []
  trainer.bind(on_update=lambda: calls.append(1))
  trainer.emit("on_update")
  assert calls == [1]
  trainer.update_config(log_interval=7)
  assert trainer.config.log_interval == 7 and trainer.paths(3).checkpoint == tmp_path / "checkpoint" / "checkpoint_3.pt"
  assert trainer.paths().cameras == tmp_path / "cameras.json" and (tmp_path / "point_cloud" / "iteration_0").is_dir()


def test_batches_are_selected_ahead_and_kept_in_the_state(tmp_path):
  torch.manual_seed(0)
  trainer = _stub_trainer(tmp_path, [], prefetch=3)
  batches = trainer.iter_batches()
  first = next(batches)
  assert len(first) == 1 and first[0].image.dtype is torch.float32 and tuple(first[0].image.shape) == (24, 32, 3)
  pending = [b.tolist() for b in trainer.state_dict()["pending_batches"]]
  assert len(pending) == 2
  assert [next(batches)[0].image_idx] == pending[0] and [next(batches)[0].image_idx] == pending[1]
  assert trainer.load_batch(torch.tensor([4, 2]))[1].image_idx == 2


def test_the_prefetch_thread_keeps_order_and_hands_errors_over():
  def load(idx):
    if int(idx[0]) == 3:
      raise KeyError("image 3")
    return [int(i) for i in idx]
  loader = _Prefetcher(load)
  for i in (1, 2, 3, 4):
    loader.submit(torch.tensor([i, i + 10]))
  assert loader.next() == [1, 11] and loader.next() == [2, 12]
  with pytest.raises(KeyError):
    loader.next()
  assert loader.next() == [4, 14]
  loader.stop()
  assert not loader._thread.is_alive()
