"""The scene's detailed logs and the ``Trainer`` end to end on the GPU.

Scene logging: an ``MLPScene`` of 1500 points after three optimizer steps and one more backward; every histogram of
``log_gradients`` / ``log_optimizer_state`` / ``log_params`` against the fp64 oracle of the same tensors
(tests/histogram_oracle.py: tallies exact, counts under the flip rule, sums inside their bounds), and none of them
changes a parameter, a gradient or optimizer state.

Trainer: ``synthetic.scene_b`` with 6 cameras at 96 x 64, targets rendered from the true scene and quantised to uint8,
the cloud the true positions subsampled to 1500; 24 steps with evaluations at 0, 12 and 24, detailed logs every 4 steps,
a densify round at 10, outputs into a temporary directory; then a checkpoint restored and run beside the live
trainer, the three samplers for 8 steps each, and the NaN check."""
import json

import numpy as np
import pytest
import torch

import histogram_oracle as ho
import splat_trainer_amd as sta
from splat_trainer_amd import ply_io, synthetic

pytestmark = pytest.mark.gpu

W, H, CAMERAS, POINTS = 96, 64, 6, 1500
PARAMETERS = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                  rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))
SCENE = sta.MLPSceneConfig(parameters=PARAMETERS, reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
                           color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=3, lr_diffuse=1e-2, lr_specular=1e-2),
                           lr_glo_feature=0.1, image_features=8, point_features=8)


@pytest.fixture(scope="module")
def dataset():
  g, cams = synthetic.scene_b(4000, W, H, sh_degree=1, seed=4, num_cameras=CAMERAS, sigma_px=2.5)
  gd = g.to("cuda")
  with torch.no_grad():
    images = [(sta.render_gaussians(gd, c.to("cuda"), sta.RasterConfig(), use_sh=True).image.clamp(0, 1) * 255).round()
              .to(torch.uint8).cpu() for c in cams]
  keep = torch.randperm(4000, generator=torch.Generator().manual_seed(1))[:POINTS]
  cloud = sta.PointCloud(g.position[keep], (0.5 + 0.282094791773878 * g.feature[keep, :, 0]).clamp(0, 1))
  projection = sta.Projections(intrinsics=cams[0].projection[None], image_size=torch.tensor([[W, H]]),
                               depth_range=torch.tensor([[0.1, 100.0]]))
  table = sta.MultiCameraTable(camera_t_world=torch.stack([c.T_camera_world for c in cams]),
                               camera_idx=torch.zeros(CAMERAS, dtype=torch.int64), projection=projection,
                               image_names=[f"view/{i}.png" for i in range(CAMERAS)],
                               labels=torch.tensor([2, 2, 2, 2, 2, 3]))          # the last view is validation as well
  return sta.TensorDataset(table, images, cloud=cloud)


def _config(tmp_path, view_selection=None, **over):
  kw = dict(scene=SCENE, controller=sta.TargetConfig(prune_rate=0.025, min_views=2, densify_prune_interval=10),
            view_selection=view_selection or sta.RandomSamplerConfig(batch_size=1),
            cloud_init=sta.CloudInitConfig(num_neighbors=3, initial_point_scale=0.5, initial_alpha=0.5),
            total_steps=24, eval_steps=12, log_interval=4, log_details=True, target_points=1800, l1_weight=0.8, ssim_weight=0.2,
            ssim_levels=2, vis_clusters=32, device="cuda", save_output=True, output_path=str(tmp_path), seed=3, prefetch=2)
  kw.update(over)
  return sta.TrainConfig(**kw)


class _Recorder(sta.NullLogger):
  """Keeps the histograms it is handed, by name."""

  def __init__(self):
    self.histograms = {}

  def log_histogram(self, name, values, num_bins=None):
    self.histograms.setdefault(name, []).append(values)


def _tree_equal(a, b, path=""):
  if isinstance(a, torch.Tensor):
    assert isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a, b), path
  elif isinstance(a, dict):
    assert sorted(a, key=str) == sorted(b, key=str), path
    for k in a:
      _tree_equal(a[k], b[k], f"{path}/{k}")
  elif isinstance(a, (list, tuple)):
    assert len(a) == len(b), path
    for i, (x, y) in enumerate(zip(a, b)):
      _tree_equal(x, y, f"{path}/{i}")
  else:
    assert a == b, path


# ---------------------------------------------------------------------------------------------------------- scene logging
def test_scene_logs_equal_the_oracle_and_change_nothing(dataset, tmp_path):
  torch.manual_seed(2)
  trainer = sta.Trainer.initialize(_config(tmp_path, save_output=False), dataset, sta.NullLogger())
  scene = trainer.scene
  assert scene.num_points == POINTS
  with torch.no_grad():                                                      # GLO rows that are not exact zeros
    scene.color_table.weight.copy_(0.5 * torch.randn(scene.color_table.weight.shape, generator=torch.Generator().manual_seed(6)))
  for i in (0, 2, 4):                                                        # three steps: the optimizer state is spread out
    trainer.training_step(trainer.load_batch(torch.tensor([i])))
  view = trainer.load_batch(torch.tensor([1]))[0]
  rendering = trainer.render(trainer.camera_params(1), 1)
  trainer.compute_losses(rendering, view.image).backward()
  scene.add_rendering(1, rendering)

  from splat_trainer_amd.mlp_scene import _clone_tree
  grads = lambda: {k: scene.points.tensors[k].grad.clone() for k in scene.points.parameter_groups}
  before = _clone_tree(scene.state_dict()), grads(), scene.points.visible.clone()
  logger = _Recorder()
  scene.log_gradients(logger, min_vis=0.1)
  scene.log_optimizer_state(logger)
  scene.log_params(logger)
  scene.log_checkpoint(logger)
  torch.cuda.synchronize()
  _tree_equal(before[0], scene.state_dict(), "state")
  _tree_equal(before[1], grads(), "grad")
  assert torch.equal(before[2], scene.points.visible)

  pts = scene.points
  host = lambda t: t.detach().reshape(t.shape[0], -1).cpu().numpy()
  visible = host(pts.visible)[:, 0]
  rows = np.nonzero(visible > np.float32(0.1))[0]
  assert 0 < rows.size < POINTS
  expected = {}
  for key in pts.parameter_groups:
    expected[f"log10_grad/{key}"] = (host(pts.tensors[key].grad), dict(rows=rows, mode=1, min_value=1e-16))
    expected[f"log10_norm_grad/{key}"] = (host(pts.tensors[key].grad), dict(rows=rows, weight=visible, eps=scene.config.vis_smooth,
                                                                            mode=1, min_value=1e-16))
  for key, state in pts.tensor_state.items():
    for k, v in state.items():
      expected[f"optimizer/{key}/{k}"] = (host(v), dict(mode=1, min_value=1e-16))
  scale = torch.exp(pts.log_scaling.detach())
  expected.update({"params/opacity": (host(torch.sigmoid(pts.alpha_logit)), {}), "params/log_scale": (host(pts.log_scaling), {}),
                   "params/feature": (host(pts.feature), {}), "params/glo_feature": (host(scene.color_table.weight), {}),
                   "params/stable_rank": (host((scale.sum(1) / scale.max(1).values)[:, None]), {}),
                   "params/aspect": (host((scale.max(1).values / (scale.min(1).values + 1e-4))[:, None]), {})})
  assert sorted(logger.histograms) == sorted(expected)
  assert all(len(v) == (2 if k.startswith("params/") else 1) for k, v in logger.histograms.items())     # log_checkpoint logs them again
  some_kept = 0
  for name, (values, kw) in expected.items():
    hist = logger.histograms[name][0]
    assert isinstance(hist, sta.Histogram) and hist.device.type == "cuda" and hist.num_bins == 64
    cls, t = ho.entries(values, **kw)
    kept = t[cls == ho.KEPT]
    some_kept += kept.size > 0
    ho.check_histogram(name, hist, cls, kept, 64, None, True)
  assert some_kept >= len(expected) - 2


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def trained(dataset, tmp_path_factory):
  tmp_path = tmp_path_factory.mktemp("trainer")
  torch.manual_seed(0)
  history = sta.HistoryLogger()
  recorder = _Recorder()
  updates = []
  trainer = sta.Trainer.initialize(_config(tmp_path), dataset, sta.CompositeLogger(history, recorder))
  trainer.bind(on_update=lambda: updates.append(trainer.step))
  start_points = trainer.scene.num_points
  metrics = trainer.train()
  return dict(trainer=trainer, metrics=metrics, history=history, recorder=recorder, updates=updates, path=tmp_path,
              start_points=start_points)


def test_training_finishes_and_improves(trained):
  trainer, history = trained["trainer"], trained["history"]
  assert trainer.step == 24 and not trainer.is_training() and trainer._prefetcher is None
  log = trainer.evaluation_log
  print("evaluation log:", log)
  assert [e["step"] for e in log] == [0, 12, 24]
  assert log[-1]["train_psnr"] > log[0]["train_psnr"]
  assert trained["metrics"]["train_psnr"] == log[-1]["train_psnr"] and "val_cc_psnr" in trained["metrics"]
  assert isinstance(trainer.view_clustering, sta.ViewClustering)
  assert tuple(trainer.view_clustering.cluster_visibility.shape) == (CAMERAS, 32)
  assert trained["updates"] == [4, 8, 12, 16, 20, 24]
  assert len(history["train/loss/total"]) == 6 and len(history["train/metrics/psnr"]) == 6             # logging steps only
  assert all(np.isfinite(history["train/loss/total"])) and len(history["eval_train/psnr"]) == 3
  assert trainer.scene.num_points != trained["start_points"]                                           # densified at 10
  names = trained["recorder"].histograms
  for name in ("rendering/log10_prune_cost", "rendering/log10_visibility", "log10_grad/position", "log10_norm_grad/feature",
               "optimizer/position/exp_avg", "params/opacity", "eval_train/points_visible", "densify/prune_cost"):
    assert name in names, sorted(names)
  assert len(names["rendering/log10_split_score"]) == 6 and isinstance(names["rendering/log10_split_score"][0], sta.Histogram)
  assert names["log10_grad/position"][-1].total > 0


def test_outputs_are_on_disk(trained):
  path = trained["path"]
  cameras = json.loads((path / "cameras.json").read_text())
  assert len(cameras) == CAMERAS and cameras[2]["img_name"] == "view/2.png" and cameras[0]["width"] == W
  initial = ply_io.read_ply(path / "point_cloud" / "iteration_0" / "point_cloud.ply")
  assert initial.shape[0] == POINTS and initial.dtype.names[:3] == ("x", "y", "z")
  assert sta.find_checkpoint(path).name == "checkpoint_24.pt"
  final = ply_io.read_gaussians(path / "point_cloud" / "iteration_24" / "point_cloud.ply", with_sh=True)
  assert final.position.shape[0] == trained["trainer"].scene.num_points


def test_a_restored_trainer_continues_bit_for_bit(trained, dataset):
  live = trained["trainer"]
  state, workspace = sta.load_checkpoint(trained["path"])
  assert workspace == trained["path"] and state["step"] == 24 and len(state["evaluation_log"]) == 3
  assert state["view_clustering"] is not None and len(state["pending_batches"]) == 1
  restored = sta.Trainer.from_state_dict(live.config, dataset, sta.NullLogger(), state)
  assert restored.step == 24 and restored.evaluation_log == live.evaluation_log
  _tree_equal(live.scene.state_dict(), restored.scene.state_dict(), "scene before")
  for trainer in (live, restored):
    torch.manual_seed(11)
    batches = trainer.iter_batches()
    for _ in range(2):
      trainer.training_step(next(batches))
      trainer.controller.step(trainer.progress)
  assert live.step == restored.step == 26
  _tree_equal(live.scene.state_dict(), restored.scene.state_dict(), "scene after")
  _tree_equal(live.controller.state_dict(), restored.controller.state_dict(), "controller after")
  _tree_equal(live.view_selection.state_dict(), restored.view_selection.state_dict(), "sampler after")


@pytest.mark.parametrize("sampler", ["random", "batch_overlap", "target_overlap"])
def test_every_sampler_trains(dataset, tmp_path, sampler):
  view_selection = dict(random=sta.RandomSamplerConfig(batch_size=2),
                        batch_overlap=sta.BatchOverlapSamplerConfig(batch_size=2, overlap_temperature=0.5),
                        target_overlap=sta.TargetOverlapConfig(batch_size=2, history_size=2))[sampler]
  torch.manual_seed(1)
  config = _config(tmp_path, view_selection, total_steps=8, eval_steps=8, log_details=False, save_output=False)
  trainer = sta.Trainer.initialize(config, dataset, sta.NullLogger())
  metrics = trainer.train()
  assert trainer.step == 8 and [e["step"] for e in trainer.evaluation_log] == [0, 8]
  assert np.isfinite(metrics["train_psnr"]) and isinstance(trainer.view_clustering, sta.ViewClustering)
  assert not (tmp_path / "cameras.json").exists()


def test_a_nan_parameter_stops_the_checkpoint(dataset, tmp_path):
  trainer = sta.Trainer.initialize(_config(tmp_path, save_output=False), dataset, sta.NullLogger())
  with torch.no_grad():
    trainer.scene.points.position[5, 1] = float("nan")
  with pytest.raises(sta.NaNParameterException, match="position"):
    trainer.checkpoint()
  assert trainer.evaluation_log == []
