"""``COLMAPDataset`` and ``export_colmap`` on the host (``device="cpu"``: the resize goes through the host shim) on the
directory of tests/colmap_scene.py: images against the arrays and the resize oracle, projections against the reference's
formula, the split, the poses against a normalised inverse worked out here in float64, the cloud, the refusals, and an
export read back."""
import numpy as np
import pytest
import torch

import colmap_scene as cs
import image_oracle as io
import splat_trainer_amd as sta
from splat_trainer_amd import colmap_io as cio
from splat_trainer_amd.camera_table import Label
from splat_trainer_amd.dataset import split_every


@pytest.fixture(scope="module")
def scene(tmp_path_factory, built_libs):
  path = tmp_path_factory.mktemp("colmap")
  return (path,) + cs.write(path)


def _dataset(scene, **kw):
  return sta.COLMAPDataset(scene[0], device="cpu", test_every=4, **kw)


def test_unscaled_images_come_back_byte_for_byte(scene):
  path, cameras, images, points, pixels = scene
  ds = _dataset(scene)
  assert ds.num_images == 9 and ds._images is None                            # lazy
  views = ds.load_images()
  assert ds.load_images() is views                                            # once
  assert [v.filename for v in views] == [im.name for im in images] == ds.camera_table.image_names
  assert [v.image_idx for v in views] == list(range(9))
  for view, im in zip(views, images):
    assert view.image.dtype is torch.uint8 and not view.image.is_cuda
    assert np.array_equal(view.image.numpy(), pixels[im.image_id])
  assert "COLMAPDataset(" in repr(ds) and "num_train=6" in repr(ds) and "num_val=3" in repr(ds)


@pytest.mark.parametrize("scale", [dict(image_scale=0.5), dict(resize_longest=37)], ids=["image_scale", "resize_longest"])
def test_scaled_images_and_projections(scene, scale):
  path, cameras, images, points, pixels = scene
  ds = _dataset(scene, **scale)
  proj = ds.camera_table.projections
  for k, (camera_id, cam) in enumerate(sorted(cameras.items())):                 # one row per camera, ascending id
    s, (w, h) = cs.scaled_size(cam.width, cam.height, **scale)
    assert proj.image_size[k].tolist() == [w, h] and proj.image_size.dtype is torch.int32
    assert torch.equal(proj.intrinsics[k], torch.tensor(cam.params * s, dtype=torch.float32))
    assert proj.depth_range[k].tolist() == pytest.approx([0.1, 100.0])
  for view, im in zip(ds.load_images(), images):
    cam = cameras[im.camera_id]
    _, (w, h) = cs.scaled_size(cam.width, cam.height, **scale)
    want = io.resize_area(pixels[im.image_id][None], h, w)[0]
    assert tuple(view.image.shape) == (h, w, 3) and np.array_equal(view.image.numpy(), want)


def test_split_labels_and_camera_indices(scene):
  path, cameras, images, points, pixels = scene
  ds = _dataset(scene)
  train, val = split_every(9, 4)
  assert torch.equal(ds.train_idx, train) and torch.equal(ds.val_idx, val) and val.tolist() == [0, 4, 8]
  table = ds.camera_table
  assert isinstance(table, sta.MultiCameraTable) and table.num_images == 9 and ds.camera_table is table
  labels = table._labels.tolist()
  assert [bool(Label(v) & Label.Validation) for v in labels] == [i in (0, 4, 8) for i in range(9)]
  assert [bool(Label(v) & Label.Training) for v in labels] == [i % 4 != 0 for i in range(9)]
  camera_rows = {camera_id: k for k, camera_id in enumerate(sorted(cameras))}
  assert table._camera_idx.tolist() == [camera_rows[im.camera_id] for im in images]
  assert [v.image_idx for v in ds.train()] == train.tolist() and [v.image_idx for v in ds.val()] == val.tolist()
  assert sorted(v.image_idx for v in ds.train(shuffle=True)) == train.tolist()
  assert [v.filename for v in ds.loader(torch.tensor([5, 1]))] == [images[5].name, images[1].name]


def _rotations(images):
  R = []
  for im in images:
    w, x, y, z = im.qvec / np.linalg.norm(im.qvec)
    R.append(np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]))
  return np.stack(R)


def _expected_normalization(images, config):
  """(translation, scaling, camera_t_world) in float64 from the definition: world_t_camera = (q, t) inverted, the
  translation minus the mean centre, the scaling one over the (lower) median distance to the (k - 1)-th nearest other
  centre, camera_t_world the inverse of the moved world_t_camera."""
  R = _rotations(images)
  world_t_camera = np.stack([np.linalg.inv(np.block([[R[k], im.tvec[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]))
                             for k, im in enumerate(images)])
  centres = world_t_camera[:, :3, 3]
  translation = -centres.mean(axis=0) if config.centering else np.zeros(3)
  scaling = 1.0
  if config.scaling_method == "median_knn":
    dist = np.linalg.norm(centres[:, None] - centres[None], axis=-1)
    kth = np.sort(dist, axis=1)[:, config.normalize_knn - 1]
    scaling = 1.0 / np.sort(kth)[(len(images) - 1) // 2]
  moved = world_t_camera.copy()
  moved[:, :3, 3] = scaling * (centres + translation)
  return translation, scaling, np.linalg.inv(moved)


@pytest.mark.parametrize("config", [sta.NormalizationConfig(),
                                    sta.NormalizationConfig(centering=True, scaling_method="median_knn", normalize_knn=3)],
                         ids=["default", "median_knn"])
def test_poses_cloud_and_to_original(scene, config):
  path, cameras, images, points, pixels = scene
  ds = _dataset(scene, normalize=config)
  translation, scaling, camera_t_world = _expected_normalization(images, config)
  assert config.scaling_method == "none" or abs(scaling - 1.0) > 1e-3
  assert ds.camera_t_world.dtype is torch.float32 and tuple(ds.camera_t_world.shape) == (9, 4, 4)
  assert np.abs(ds.camera_t_world.numpy().astype(np.float64) - camera_t_world).max() < 1e-6
  assert ds.normalize.scaling == pytest.approx(scaling, rel=1e-12)
  cloud = ds.pointcloud()
  assert isinstance(cloud, sta.PointCloud) and cloud.num_points == 200 and cloud.points.dtype is torch.float32
  assert torch.equal(cloud.colors, torch.tensor(points.rgb, dtype=torch.float32) / 255.0)
  assert np.abs(cloud.points.numpy() - scaling * (points.xyz + translation)).max() < 2e-6
  back = ds.to_original.transform_points(cloud.points)
  assert np.abs(back.numpy() - points.xyz).max() < 2e-6


def test_model_without_points_has_no_cloud(tmp_path, built_libs):
  cs.write(tmp_path)
  (tmp_path / "sparse" / "0" / "points3D.bin").unlink()
  assert sta.COLMAPDataset(tmp_path, device="cpu").pointcloud() is None


def test_refusals(tmp_path, scene, built_libs):
  with pytest.raises(ValueError, match="either resize_longest or image_scale"):
    _dataset(scene, image_scale=0.5, resize_longest=32)
  with pytest.raises(ValueError, match="only shrinks"):
    _dataset(scene, image_scale=1.5)
  with pytest.raises(ValueError, match="only shrinks"):
    _dataset(scene, resize_longest=65)                                        # above the larger camera's 64
  cs.write(tmp_path, bad_camera=cio.Camera("SIMPLE_RADIAL", 64, 48, np.array([60.0, 32.0, 24.0, 0.01])))
  with pytest.raises(ValueError, match="SIMPLE_RADIAL.*undistorted"):
    sta.COLMAPDataset(tmp_path, device="cpu")
  wrong = tmp_path / "wrong"
  _, images, _, _ = cs.write(wrong)
  from PIL import Image
  Image.fromarray(np.zeros((48, 63, 3), np.uint8)).save(wrong / "images" / images[2].name)      # image id 5: camera 3, 64 x 48
  with pytest.raises(ValueError, match=r"im 005\.png is 63 x 48, its camera is 64 x 48"):
    sta.COLMAPDataset(wrong, device="cpu").load_images()


def test_simple_pinhole_is_accepted(tmp_path, built_libs):
  cs.write(tmp_path, bad_camera=cio.Camera("SIMPLE_PINHOLE", 64, 48, np.array([61.0, 31.5, 24.5])))
  ds = sta.COLMAPDataset(tmp_path, device="cpu", image_scale=0.5)
  assert ds.projections.intrinsics[0].tolist() == [30.5, 30.5, 15.75, 12.25]


@pytest.mark.parametrize("ext", [".bin", ".txt"])
def test_export_read_back(scene, tmp_path, ext):
  config = sta.NormalizationConfig(centering=True, scaling_method="median_knn", normalize_knn=3)
  ds = _dataset(scene, normalize=config, image_scale=0.5)
  views = ds.load_images()
  sta.export_colmap(tmp_path, ds.camera_table, views, ds.pointcloud(), ext=ext, normalization=ds.normalize)
  assert sorted(p.name for p in (tmp_path / "sparse" / "0").iterdir()) == sorted(f"{s}{ext}" for s in ("cameras", "images", "points3D"))
  _, records, _ = cio.read_model(tmp_path / "sparse" / "0")
  assert all(r.qvec[0] >= 0 for r in records) and all("/" not in r.name for r in records)
  assert records[0].name == ds.image_names[0].replace("/", "_")
  again = sta.COLMAPDataset(tmp_path, device="cpu", test_every=4, normalize=config)
  assert (again.camera_t_world - ds.camera_t_world).abs().max() < 1e-5
  assert torch.equal(again.projections.intrinsics, ds.projections.intrinsics)
  assert torch.equal(again.projections.image_size, ds.projections.image_size)
  assert again.camera_idx == ds.camera_idx
  for a, b in zip(again.load_images(), views):
    assert torch.equal(a.image, b.image)
  assert torch.equal(again.pointcloud().colors, ds.pointcloud().colors)
  assert (again.pointcloud().points - ds.pointcloud().points).abs().max() < 1e-5
  # without the normalisation the normalised coordinates themselves are written
  sta.export_colmap(tmp_path / "n", ds.camera_table, [v.image for v in views], None, ext=ext)
  plain = sta.COLMAPDataset(tmp_path / "n", device="cpu", normalize=sta.NormalizationConfig(centering=False))
  assert (plain.camera_t_world - ds.camera_t_world).abs().max() < 1e-5 and plain.pointcloud() is None
