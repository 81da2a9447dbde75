"""Depth fusion on the device (csrc/fusion.hip) against tests/fusion_oracle.py, bit for bit: the cases of
tests/fusion_cases.py that tests/test_fusion_host.py runs on the host, one end-to-end fusion of rendered depth maps, and
the device and host paths on the same inputs."""
import numpy as np
import pytest
import torch

import fusion_cases as cases
import splat_trainer_amd as sta
from splat_trainer_amd import fusion, ply_io, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend(built_libs):
  return cases.DeviceBackend()


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_case(backend, name):
  cases.CASES[name](backend)


@pytest.fixture(scope="module")
def rendered(built_libs):
  """The plane z = 4 rendered from three 64 x 48 cameras shifted along x by 0, 0.25 and 0.5: (cameras, renderings)."""
  gaussians, cameras = synthetic.plane(64, 48)
  gaussians = gaussians.to("cuda")
  cameras = [c.to("cuda") for c in cameras]
  with torch.no_grad():
    renderings = [sta.render_gaussians(gaussians, c, sta.RasterConfig(), use_sh=False, render_median_depth=True)
                  for c in cameras]
  return cameras, renderings


@pytest.mark.parametrize("voxel", [None, 0.25])
def test_fuse_scene_of_a_rendered_plane(rendered, voxel):
  cameras, renderings = rendered
  config = sta.FusionConfig(rel_tol=0.01, min_agree=2, max_violate=0, num_sources=2, voxel_size=voxel)
  got = sta.fuse_scene(lambda camera, idx: renderings[idx], cameras, config)
  depths = [r.median_depth_image.cpu().numpy() for r in renderings]
  images = [r.image.cpu().numpy() for r in renderings]
  cams = [(c.T_camera_world.cpu().numpy(), c.projection.cpu().numpy(), c.near_plane) for c in cameras]
  want = cases.oracle_fusion(depths, images, cams, [[1, 2], [0, 2], [1, 0]], 0.01, 2, 0, voxel)
  print("kept per view", want[3], "points", want[0].shape[0])
  assert all(k > 0 for k in want[3])                                       # the oracle's own kept counts
  cases.check_fusion(got, want)
  assert abs(float(got[0].points[:, 2].median()) - 4.0) < 0.05             # the plane


def test_device_and_host_return_the_same_bytes(rendered):
  cameras, renderings = rendered
  config = sta.FusionConfig(min_agree=1, num_sources=2, voxel_size=0.3)
  depths, images = [r.median_depth_image for r in renderings], [r.image for r in renderings]
  dev_cloud, dev_agree = sta.fuse_depth_maps(depths, images, cameras, config)
  host_cloud, host_agree = sta.fuse_depth_maps([d.cpu() for d in depths], [i.cpu() for i in images],
                                               [c.to("cpu") for c in cameras], config)
  assert dev_cloud.num_points > 0 and not host_cloud.points.is_cuda
  cases.same(dev_cloud.points.cpu().numpy(), host_cloud.points.numpy())
  cases.same((dev_cloud.colors.cpu() * 255).round().to(torch.uint8).numpy(), (host_cloud.colors * 255).round().to(torch.uint8).numpy())
  cases.same(dev_agree.cpu().numpy(), host_agree.numpy())
  rng = np.random.default_rng(9)
  pts = torch.from_numpy(rng.normal(0, 3, (70001, 3)).astype(np.float32))
  col = torch.from_numpy(rng.integers(0, 256, (70001, 3)).astype(np.uint8))
  for d, h in zip(sta.voxel_downsample(pts.cuda(), col.cuda(), 0.21, (0.1, 0.2, -0.3)), sta.voxel_downsample(pts, col, 0.21, (0.1, 0.2, -0.3))):
    cases.same(d.cpu().numpy(), h.numpy())


def test_host_reads_are_the_documented_ones(rendered, monkeypatch):
  """With cameras on the device: one read for all the cameras, one per view (its kept count), one more (K) with a voxel
  size; depth_consistency makes the one camera read and none with HostCamera records."""
  cameras, renderings = rendered
  depths, images = [r.median_depth_image for r in renderings], [r.image for r in renderings]
  reads = []

  def counted(name):
    original = getattr(torch.Tensor, name)

    def wrapper(self, *args, **kwargs):
      to_host = name != "to" or any(str(a) == "cpu" for a in list(args) + list(kwargs.values()))
      if self.is_cuda and to_host:
        reads.append(name)
      return original(self, *args, **kwargs)
    monkeypatch.setattr(torch.Tensor, name, wrapper)
  for name in ("cpu", "item", "tolist", "numpy", "to", "__bool__", "__int__", "__float__"):
    counted(name)
  V = len(cameras)
  sta.fuse_depth_maps(depths, images, cameras, sta.FusionConfig(num_sources=2))
  assert reads == ["cpu"] + ["item"] * V, reads
  del reads[:]
  sta.fuse_depth_maps(depths, images, cameras, sta.FusionConfig(num_sources=2, voxel_size=0.25))
  assert reads == ["cpu"] + ["item"] * (V + 1), reads
  del reads[:]
  sources = list(zip(depths[1:], cameras[1:]))
  sta.depth_consistency(depths[0], cameras[0], sources, 0.01)
  assert reads == ["cpu"], reads
  del reads[:]
  on_host = fusion.read_cameras(cameras)
  assert reads == ["cpu"]
  del reads[:]
  sta.depth_consistency(depths[0], on_host[0], list(zip(depths[1:], on_host[1:])), 0.01)
  assert sta.select_sources(on_host, 2) == [[1, 2], [0, 2], [1, 0]] and reads == []


W, H, CAMERAS, POINTS = 96, 64, 6, 1500


@pytest.fixture(scope="module")
def trainer(built_libs, tmp_path_factory):
  """An untrained Trainer on scene B: 6 cameras at 96 x 64 (the last one validation as well), 1500 nearly opaque points."""
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
  dataset = sta.TensorDataset(table, images, cloud=cloud)
  parameters = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                    rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))
  scene = sta.MLPSceneConfig(parameters=parameters, reg_weight=dict(scale=0.1, opacity=1.0, aspect=0.01, specular=0.5),
                             color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=3, lr_diffuse=1e-2, lr_specular=1e-2),
                             lr_glo_feature=0.1, image_features=8, point_features=8)
  config = sta.TrainConfig(scene=scene, controller=sta.TargetConfig(prune_rate=0.025, min_views=2, densify_prune_interval=10),
                           view_selection=sta.RandomSamplerConfig(batch_size=1),
                           cloud_init=sta.CloudInitConfig(num_neighbors=3, initial_point_scale=0.5, initial_alpha=0.95),
                           total_steps=24, eval_steps=12, log_interval=4, target_points=1800, l1_weight=0.8, ssim_weight=0.2,
                           ssim_levels=2, vis_clusters=32, device="cuda", save_output=False,
                           output_path=str(tmp_path_factory.mktemp("fusion_trainer")), seed=3, prefetch=2)
  trainer = sta.Trainer.initialize(config, dataset, sta.NullLogger())
  yield trainer
  trainer.close()


def test_trainer_fused_cloud(trainer, tmp_path):
  """Trainer.fused_cloud is fuse_scene over the trainer's own renders of the training views, taken back to the dataset's
  coordinates; write_fused_cloud writes that cloud."""
  fusion_config = sta.FusionConfig(rel_tol=0.05, min_agree=1, num_sources=3, voxel_size=0.02)
  cloud = trainer.fused_cloud(fusion_config)
  indexes = [int(v.image_idx) for v in trainer.dataset.train(shuffle=False)]
  cameras = [trainer.camera_params(i) for i in indexes]
  want, _ = sta.fuse_scene(lambda c, i: trainer.render(c, i, render_median_depth=True), cameras, fusion_config, indexes)
  want = trainer.unnormalize.transform_cloud(want)
  print("fused points", cloud.num_points)
  assert cloud.num_points > 0
  assert torch.equal(cloud.points, want.points) and torch.equal(cloud.colors, want.colors)
  assert trainer.fused_cloud(fusion_config, which="val").num_points == 0      # one validation view: no sources, no votes
  with pytest.raises(ValueError):
    trainer.fused_cloud(which="test")
  path = tmp_path / "fused.ply"
  written = trainer.write_fused_cloud(path, fusion_config)
  vertex = ply_io.read_ply(path)
  assert len(vertex) == written.num_points == cloud.num_points
  assert np.array_equal(np.stack([vertex["x"], vertex["y"], vertex["z"]], 1), cloud.points.cpu().numpy())


def test_fuse_scene_takes_a_scene_object(trainer):
  """An MLPScene handed over directly is rendered with render_median_depth=True, under no_grad."""
  indexes = [int(v.image_idx) for v in trainer.dataset.train(shuffle=False)]
  cameras = [trainer.camera_params(i) for i in indexes]
  config = sta.FusionConfig(rel_tol=0.05, min_agree=1, num_sources=3)
  scene = trainer.scene
  assert isinstance(scene, sta.MLPScene)
  got, got_agree = sta.fuse_scene(scene, cameras, config, indexes)
  with torch.no_grad():
    renderings = [scene.render(c, i, render_median_depth=True) for c, i in zip(cameras, indexes)]
  want, want_agree = sta.fuse_depth_maps([r.median_depth_image for r in renderings], [r.image for r in renderings], cameras,
                                         config)
  assert got.num_points > 0 and not got.points.requires_grad
  assert torch.equal(got.points, want.points) and torch.equal(got.colors, want.colors) and torch.equal(got_agree, want_agree)
