"""TSDF meshing on the host: the shim (libgsr_hostmath.so, the arithmetic of csrc/gsr_mesh.h compiled for the CPU) and
the package's CPU path against tests/mesh_oracle.py, bit for bit.  The cases are in tests/mesh_cases.py;
tests/test_gpu_mesh.py runs the same ones on the device."""
import numpy as np
import pytest
import torch

import hostmath
import mesh_cases as cases
import splat_trainer_amd as sta
from splat_trainer_amd import mesh, ply_io


@pytest.fixture(scope="module")
def backend(built_libs):
  return cases.HostBackend(hostmath.load(built_libs))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_case(backend, name):
  cases.CASES[name](backend)


def _volume():
  return sta.TsdfVolume((0.0, 0.0, 0.0), (3, 3, 3), 0.5)


def test_arguments_are_checked():
  depth = torch.ones(4, 5)
  cam = cases.camera(np.eye(4), [5, 5, 2.5, 2], 4, 5)
  for bad in (dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(origin=(0.0, float("inf"), 0.0)),
              dict(origin=(0.0, 0.0)), dict(dims=(3, 3)), dict(dims=(3, -1, 3)), dict(dims=(1024, 1024, 1024)),
              dict(trunc=0.0), dict(trunc=float("inf")), dict(near=float("nan"))):
    args = dict(dict(origin=(0.0, 0.0, 0.0), dims=(3, 3, 3), voxel_size=0.5), **bad)
    with pytest.raises(ValueError):
      sta.TsdfVolume(**args)
  with pytest.raises(ValueError):
    _volume().integrate([depth], None, [cam, cam])
  with pytest.raises(ValueError):
    _volume().integrate([depth.double()], None, [cam])
  with pytest.raises(ValueError):
    _volume().integrate([torch.ones(5, 4)], None, [cam])                        # not the camera's size
  with pytest.raises(ValueError):
    _volume().integrate([depth], [torch.ones(4, 5)], [cam])                     # an image without channels
  for min_weight in (0, -1, 1.5, True):
    with pytest.raises(ValueError):
      _volume().extract(min_weight)
  for config in (sta.TsdfConfig(voxel_size=-1.0), sta.TsdfConfig(voxel_size=0.5, trunc=0.0),
                 sta.TsdfConfig(voxel_size=0.5, min_weight=0), sta.TsdfConfig(voxel_size=0.5, bounds=((0, 0, 0), (1, 1))),
                 sta.TsdfConfig(voxel_size=0.5, bounds=((0, 0, 0), (1, 0, 1))),
                 sta.TsdfConfig(voxel_size=0.5, bounds=((0, 0, 0), (1, 1, float("nan")))),
                 sta.TsdfConfig(voxel_size=0.5, fusion=sta.FusionConfig(min_agree=300))):
    with pytest.raises(ValueError):
      sta.mesh_depth_maps([depth], None, [cam], config)
  with pytest.raises(ValueError):
    sta.mesh_depth_maps([], None, [], sta.TsdfConfig(voxel_size=0.5))
  with pytest.raises(ValueError):
    sta.mesh_depth_maps([torch.zeros(4, 5)], None, [cam], sta.TsdfConfig(voxel_size=0.5))      # no valid depth, no box
  with pytest.raises(ValueError):
    sta.TriangleMesh(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
  assert _volume().integrate([], None, []).views == 0


def test_a_volume_counts_its_views_and_refuses_more_than_65535():
  volume = _volume()
  depth = torch.ones(4, 5)
  cam = cases.camera(np.eye(4), [5, 5, 2.5, 2], 4, 5)
  volume.integrate([depth, depth], None, [cam, cam])
  assert volume.views == 2 and mesh.MAX_VIEWS == 65535
  volume.views = 65534
  volume.integrate([depth], None, [cam])
  before = volume.state.clone()
  with pytest.raises(ValueError):
    volume.integrate([depth], None, [cam])
  assert torch.equal(volume.state, before)
  # the cap is what keeps sum_d inside int32: 65535 samples of the largest Q
  assert 65535 * 32768 < 2 ** 31 <= 65537 * 32768


def test_max_voxels_names_a_voxel_size_that_fits():
  depth = torch.ones(4, 5)
  cam = cases.camera(np.eye(4), [5, 5, 2.5, 2], 4, 5)
  bounds = ((-1.0, -1.0, 0.0), (1.0, 1.0, 2.0))
  with pytest.raises(ValueError, match="a voxel size of .* fits") as error:
    sta.mesh_depth_maps([depth], None, [cam], sta.TsdfConfig(voxel_size=0.01, bounds=bounds, max_voxels=30 ** 3))
  fits = float(str(error.value).rsplit("a voxel size of ", 1)[1].split(" ")[0])
  assert 0.01 < fits < 0.09
  sta.mesh_depth_maps([depth], None, [cam], sta.TsdfConfig(voxel_size=fits, bounds=bounds, max_voxels=30 ** 3))
  assert mesh._box_dims(np.array([-1.28] * 3), np.array([1.28] * 3), 0.08) == (33, 33, 33)


def test_bounds_from_the_cloud_and_floater_removal():
  """bounds=None: the box of every valid depth's point, grown by trunc.  With a fusion config a floater that no other
  view confirms is dropped before integration and leaves no surface."""
  depths, images, cams = cases.fusion_cases.plane_views()
  depths = [np.full_like(d, 4.0) for d in depths[:2]]     # two 16 x 12 views of the plane z = 4, 0.25 apart along x
  depths[1][3:9, 13:16] = 2.0                             # a floater at the edge of view 1 that view 0 does not see
  cameras = [cases.camera(T, proj, d.shape[0], d.shape[1], near) for (T, proj, near), d in zip(cams, depths)]
  t_depths = [torch.from_numpy(d) for d in depths]
  config = sta.TsdfConfig(voxel_size=0.1, trunc=0.3)
  with_floater = sta.mesh_depth_maps(t_depths, None, cameras, config)
  assert with_floater.num_faces > 0 and float(with_floater.vertices[:, 2].min()) < 2.5
  lo = with_floater.vertices.min(0).values
  assert float(lo[2]) >= 2.0 - 0.3 - 1e-6                # the lattice starts trunc before the nearest point
  fusion = sta.FusionConfig(rel_tol=0.01, min_agree=1, max_violate=0, num_sources=1)
  cleaned = sta.mesh_depth_maps(t_depths, None, cameras, sta.TsdfConfig(voxel_size=0.1, trunc=0.3, fusion=fusion))
  assert cleaned.num_faces > 0 and float(cleaned.vertices[:, 2].min()) > 3.5
  assert abs(float(cleaned.vertices[:, 2].median()) - 4.0) < 0.05


def test_mesh_scene_and_the_transform_on_the_host():
  """mesh_scene with a render function, and TriangleMesh.transformed by a Normalization."""
  depths, images, cams = cases.sphere_views()
  cameras = [cases.camera(T, proj, H, W, 0.1) for T, proj, H, W in cams]

  def render(camera, idx):
    return sta.Rendering(image=torch.from_numpy(images[idx]), camera=camera, points=None,
                         median_depth_image=torch.from_numpy(depths[idx]))
  config = sta.TsdfConfig(voxel_size=0.16, bounds=((-1.28,) * 3, (1.28,) * 3), near=0.1)
  got = sta.mesh_scene(render, cameras, config)
  want = sta.mesh_depth_maps([torch.from_numpy(d) for d in depths], [torch.from_numpy(i) for i in images], cameras, config)
  assert got.num_faces > 500
  for a, b in ((got.vertices, want.vertices), (got.colors, want.colors), (got.faces, want.faces)):
    assert torch.equal(a, b)
  norm = sta.Normalization(config=None, translation=torch.tensor([1.0, -2.0, 0.5]), scaling=2.0)
  moved = got.transformed(norm)
  assert torch.equal(moved.vertices, 2.0 * (got.vertices + torch.tensor([1.0, -2.0, 0.5])))
  assert moved.faces is got.faces and moved.colors is got.colors
  with pytest.raises(ValueError):
    sta.mesh_scene(render, cameras, config, image_indexes=[0])


def test_write_mesh_and_read_mesh_round_trip(tmp_path):
  rng = np.random.default_rng(7)
  vertices = rng.normal(0, 3, (50, 3)).astype(np.float32)
  vertices[0] = (np.float32(1e-45), -0.0, np.float32(3e38))
  colors = rng.integers(0, 256, (50, 3)).astype(np.uint8)
  faces = rng.integers(0, 50, (77, 3)).astype(np.int32)
  path = tmp_path / "mesh.ply"
  ply_io.write_mesh(path, vertices, colors, faces)
  head = path.read_bytes().split(b"end_header\n")[0].decode("ascii").split("\n")
  assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 50"]
  assert "property list uchar int vertex_indices" in head and "element face 77" in head
  assert path.stat().st_size == len("\n".join(head)) + len("end_header\n") + 50 * 15 + 77 * 13
  got = ply_io.read_mesh(path)
  for g, w in zip(got, (vertices, colors, faces)):
    cases.same(g, w)
  vertex = ply_io.read_ply(path)                                   # the vertex element alone reads as a cloud
  assert len(vertex) == 50 and np.array_equal(vertex["red"], colors[:, 0])
  ply_io.write_mesh(path, vertices[:0], colors[:0], faces[:0])     # an empty mesh
  assert [a.shape for a in ply_io.read_mesh(path)] == [(0, 3), (0, 3), (0, 3)]
  sta.TriangleMesh(torch.from_numpy(vertices), torch.from_numpy(colors), torch.from_numpy(faces)).save_ply(path)
  cases.same(ply_io.read_mesh(path)[2], faces)


def test_write_mesh_and_read_mesh_check_their_arguments(tmp_path):
  v, c, f = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8), np.zeros((2, 3), np.int32)
  path = tmp_path / "bad.ply"
  for bad in ((v.astype(np.float64), c, f), (v, c.astype(np.float32), f), (v, c, f.astype(np.int64)), (v[:, :2], c[:, :2], f),
              (v, c[:3], f), (v, c, f[:, :2]), (v, c, f + 4), (v, c, f - 1)):
    with pytest.raises(ValueError):
      ply_io.write_mesh(path, *bad)
  path.write_bytes(b"not a ply at all")
  with pytest.raises(ValueError):
    ply_io.read_mesh(path)
  ply_io.write_ply(path, np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])))      # a cloud: no face element
  with pytest.raises(ValueError):
    ply_io.read_mesh(path)
  ply_io.write_mesh(path, v, c, f)
  path.write_bytes(path.read_bytes()[:-5])
  with pytest.raises(ValueError):
    ply_io.read_mesh(path)
