"""TSDF meshing on the device (csrc/mesh.hip) against tests/mesh_oracle.py, bit for bit: the cases of tests/mesh_cases.py
that tests/test_mesh_host.py runs on the host, the mesh of a rendered plane on the device and host paths, the host reads
of an extraction, and Trainer.mesh."""
import numpy as np
import pytest
import torch

import mesh_cases as cases
import splat_trainer_amd as sta
from splat_trainer_amd import ply_io
from test_gpu_fusion import rendered, trainer      # noqa: F401  the fusion tests' fixtures: the rendered plane (three
#                                                    64 x 48 views of z = 4) and an untrained Trainer on scene B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend(built_libs):
  return cases.DeviceBackend()


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_case(backend, name):
  cases.CASES[name](backend)


def test_mesh_scene_of_a_rendered_plane_on_device_and_host(rendered):
  cameras, renderings = rendered
  config = sta.TsdfConfig(voxel_size=0.1, fusion=sta.FusionConfig(rel_tol=0.01, min_agree=1, num_sources=2))
  got = sta.mesh_scene(lambda camera, idx: renderings[idx], cameras, config)
  depths, images = [r.median_depth_image.cpu() for r in renderings], [r.image.cpu() for r in renderings]
  host = sta.mesh_depth_maps(depths, images, [c.to("cpu") for c in cameras], config)
  print("plane:", got, "z from", float(got.vertices[:, 2].min()), "to", float(got.vertices[:, 2].max()))
  assert got.num_faces > 1000 and got.vertices.is_cuda and not host.vertices.is_cuda
  cases.same(got.vertices.cpu().numpy(), host.vertices.numpy())
  cases.same(got.colors.cpu().numpy(), host.colors.numpy())
  cases.same(got.faces.cpu().numpy(), host.faces.numpy())
  assert float((got.vertices[:, 2] - 4.0).abs().max()) < 0.1               # within a voxel of the plane
  assert int(got.faces.min()) >= 0 and int(got.faces.max()) < got.num_vertices


def test_host_reads_of_an_extraction_are_v_and_f(rendered, monkeypatch):
  """integrate with cameras on the device: one read for all of them; extract: two, the vertex and the face count."""
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
  volume = sta.TsdfVolume((-2.5, -2.0, 3.0), (60, 41, 21), 0.1, "cuda")
  volume.integrate(depths, images, cameras)
  assert reads == ["cpu"], reads
  del reads[:]
  mesh = volume.extract()
  assert reads == ["item", "item"], reads
  del reads[:]
  assert mesh.num_faces > 1000
  V = len(cameras)
  sta.mesh_depth_maps(depths, images, cameras, sta.TsdfConfig(voxel_size=0.1))
  assert reads == ["cpu"] + ["item"] * V + ["cpu"] + ["item"] * 2, reads      # cameras, the cloud's rows, its box, V and F


def test_trainer_mesh(trainer, tmp_path):
  """Trainer.mesh is mesh_scene over the trainer's own renders of the training views, taken back to the dataset's
  coordinates; write_mesh writes that mesh."""
  indexes = [int(v.image_idx) for v in trainer.dataset.train(shuffle=False)]
  cameras = [trainer.camera_params(i) for i in indexes]
  cloud, _ = sta.fuse_scene(lambda c, i: trainer.render(c, i, render_median_depth=True), cameras,
                            sta.FusionConfig(min_agree=0, max_violate=255, num_sources=0), indexes)
  extent = float((cloud.points.max(0).values - cloud.points.min(0).values).max())
  config = sta.TsdfConfig(voxel_size=extent / 60, max_voxels=2 ** 22)
  mesh = trainer.mesh(config)
  want = sta.mesh_scene(lambda c, i: trainer.render(c, i, render_median_depth=True), cameras, config, indexes)
  want = want.transformed(trainer.unnormalize)
  print("trainer mesh", mesh)
  assert mesh.num_faces > 0
  assert torch.equal(mesh.vertices, want.vertices) and torch.equal(mesh.colors, want.colors) and torch.equal(mesh.faces, want.faces)
  with pytest.raises(ValueError):
    trainer.mesh(which="test")
  with pytest.raises(ValueError, match="fits"):
    trainer.mesh(sta.TsdfConfig(voxel_size=extent / 2000, max_voxels=2 ** 20))
  path = tmp_path / "mesh.ply"
  written = trainer.write_mesh(path, config)
  vertices, colors, faces = ply_io.read_mesh(path)
  assert written.num_faces == mesh.num_faces
  assert np.array_equal(vertices, mesh.vertices.cpu().numpy()) and np.array_equal(faces, mesh.faces.cpu().numpy())
  assert np.array_equal(colors, mesh.colors.cpu().numpy())
