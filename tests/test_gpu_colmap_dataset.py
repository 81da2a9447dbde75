"""``COLMAPDataset`` on the GPU: the native resize gives the bytes of the host path, resident images are handed out on the
device, and a scene exported with ``export_colmap`` trains exactly as the same data held in a ``TensorDataset``."""
import types

import pytest
import torch

import colmap_scene as cs
import splat_trainer_amd as sta
from splat_trainer_amd import synthetic
from test_gpu_trainer import CAMERAS, H, POINTS, W, _config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(tmp_path_factory, built_libs):
  path = tmp_path_factory.mktemp("colmap")
  cs.write(path)
  return path


@pytest.mark.parametrize("scale", [dict(image_scale=0.5), dict(resize_longest=37)], ids=["image_scale", "resize_longest"])
def test_device_path_gives_the_host_path_bytes(scene, scale):
  host = sta.COLMAPDataset(scene, device="cpu", **scale).load_images()
  native = sta.COLMAPDataset(scene, device="cuda", **scale).load_images()
  resident = sta.COLMAPDataset(scene, resident=True, **scale)                  # device: the current one
  assert resident.device.type == "cuda"
  loader = types.SimpleNamespace(device=torch.device("cuda"))                   # what Trainer.load_data reads of a trainer
  for h, n, r in zip(host, native, resident.load_images()):
    assert not n.image.is_cuda and n.image.dtype is torch.uint8 and torch.equal(n.image, h.image)
    assert r.image.is_cuda and r.image.dtype is torch.uint8 and torch.equal(r.image.cpu(), h.image)
    a, b = sta.Trainer.load_data(loader, r), sta.Trainer.load_data(loader, h)
    assert a.image.is_cuda and a.image.dtype is torch.float32 and torch.equal(a.image, b.image)
  assert [v.image.is_cuda for v in resident.train()] == [True] * len(resident.train_idx)


def _train(config, dataset):
  torch.manual_seed(0)
  history = sta.HistoryLogger()
  trainer = sta.Trainer.initialize(config, dataset, history)
  trainer.train()
  return trainer, history


def test_an_exported_scene_trains_like_the_same_data_in_memory(tmp_path, built_libs):
  """The scene of tests/test_gpu_trainer.py's fixture, through files: 12 steps improve the PSNR, and the losses are,
  bit for bit, those of the same images, table and cloud in a TensorDataset."""
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
                               image_names=[f"view/{i}.png" for i in range(CAMERAS)], labels=torch.tensor([2, 2, 2, 2, 2, 3]))
  sta.export_colmap(tmp_path / "scene", table, images, cloud)

  files = sta.COLMAPDataset(tmp_path / "scene", test_every=6, normalize=sta.NormalizationConfig(centering=False))
  assert files.num_images == CAMERAS and files.image_names == [f"view_{i}.png" for i in range(CAMERAS)]
  assert files.pointcloud().num_points == POINTS
  for view, image in zip(files.load_images(), images):
    assert torch.equal(view.image, image)
  assert (files.camera_t_world - torch.stack([c.T_camera_world for c in cams])).abs().max() < 1e-5
  memory = sta.TensorDataset(files.camera_table, [v.image for v in files.load_images()], cloud=files.pointcloud(),
                             normalization=files.normalize)
  assert torch.equal(memory.train_idx, files.train_idx) and torch.equal(memory.val_idx, files.val_idx)

  over = dict(total_steps=12, eval_steps=12, log_interval=1)
  trainer, history = _train(_config(tmp_path / "a", **over), files)
  assert trainer.step == 12 and not trainer.is_training()
  log = trainer.evaluation_log
  print("evaluation log:", log)
  assert [e["step"] for e in log] == [0, 12] and log[-1]["train_psnr"] > log[0]["train_psnr"]
  losses = history["train/loss/total"]
  assert len(losses) == 12
  _, history_memory = _train(_config(tmp_path / "b", **over), memory)
  assert history_memory["train/loss/total"] == losses                            # the files add nothing but I/O
