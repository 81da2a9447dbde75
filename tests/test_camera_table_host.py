"""CPU checks of the camera tables: the host build of the pose maths (csrc/gsr_camera_table.h through the shim) against the
fp64 oracle, the analytic gradient formulas against autograd, and the plain-torch containers, tables and normalisation of
splat_trainer_amd.camera_table / .normalization."""
import numpy as np
import pytest
import torch

import camera_table_oracle as co
import hostmath
import splat_trainer_amd as sta
from splat_trainer_amd import camera_table as ct


@pytest.fixture(scope="module")
def shim(built_libs):
  return hostmath.load(built_libs)


@pytest.fixture(scope="module")
def measured(shim):
  """The shim's largest errors against fp64 on the measurement inputs, per form: {form: (forward, backward, formulas)}."""
  out = {}
  for name, ql, tl, il, qr, tr, ir, G in co.measurement_inputs():
    T, rc_f = co.shim_forward(shim, ql, tl, il, qr, tr, ir)
    got, rc_b = co.shim_backward(shim, ql, tl, il, qr, tr, ir, G)
    assert rc_f == 0 and rc_b == 0
    want = co.backward_fp64(ql, tl, il, qr, tr, ir, G)
    auto = co.autograd_fp64(ql, tl, il, qr, tr, ir, G)
    out[name] = (co.forward_error(T, co.forward_fp64(ql, tl, il, qr, tr, ir), tl, tr),
                 co.backward_error(got, want, ql, tl, il, qr, tr, ir),
                 co.backward_error(want, auto, ql, tl, il, qr, tr, ir))
  return out


@pytest.mark.parametrize("form", ["single", "rig"])
def test_shim_matches_the_fp64_oracle_within_the_measured_error(measured, form):
  forward, backward, _ = measured[form]
  print(f"{form}: forward {forward:.3e} (stored {co.MEASURED_FORWARD[form]:.1e}), backward {backward:.3e} "
        f"(stored {co.MEASURED_BACKWARD[form]:.1e})")
  assert forward <= co.MEASURED_FORWARD[form]
  assert backward <= co.MEASURED_BACKWARD[form]
  # the stored figure is the measurement rounded up, not a loose cap
  assert forward > 0.5 * co.MEASURED_FORWARD[form] and backward > 0.5 * co.MEASURED_BACKWARD[form]
  assert co.BOUND_FORWARD[form] == co.MARGIN * co.MEASURED_FORWARD[form] and co.MARGIN == 4.0


@pytest.mark.parametrize("form", ["single", "rig"])
def test_analytic_backward_matches_autograd_to_fp64_rounding(measured, form):
  print(f"{form}: analytic vs autograd {measured[form][2]:.3e}")
  assert measured[form][2] < 1e-13


def test_zero_quaternion_is_the_identity_rotation(shim):
  q, t = co.tables(3, 1)
  q[1] = 0.0
  T, rc = co.shim_forward(shim, q, t, np.arange(3))
  assert rc == 0
  assert np.array_equal(T[1, :3, :3], np.eye(3, dtype=np.float32)) and np.array_equal(T[1, :3, 3], t[1])
  assert np.array_equal(T[:, 3], np.tile(np.float32([0, 0, 0, 1]), (3, 1)))
  assert co.forward_error(T, co.forward_fp64(q, t, np.arange(3)), t) <= co.MEASURED_FORWARD["single"]
  # at q = 0 the rotation is stationary (it is quadratic in q^); below the clamp, |q| < eps, the gradient is dq^ / eps,
  # as F.normalize's autograd gives
  q[2] = co.tables(1, 8, unit=True)[0][0] * np.float32(1e-13)
  G = co.upstream(3, 2)
  got, _ = co.shim_backward(shim, q, t, np.arange(3), None, None, None, G)
  want = co.autograd_fp64(q, t, np.arange(3), None, None, None, G)
  assert not got[0][1].any() and not want[0][1].any()
  assert np.allclose(got[0][2], want[0][2], rtol=1e-5, atol=0) and np.abs(want[0][2]).max() > 1e9


def test_unselected_rows_get_exact_zeros_and_repeats_are_summed_in_batch_order(shim):
  ql, tl = co.tables(5, 3)
  il = np.array([3, 0, 3, 4, 0, 3, 1])
  G = co.upstream(7, 4)
  (d_q, d_t, _, _), rc = co.shim_backward(shim, ql, tl, il, None, None, None, G)
  assert rc == 0 and not d_q[2].any() and not d_t[2].any()
  assert np.array_equal(d_t[3], (G[0, :3, 3] + G[2, :3, 3]) + G[5, :3, 3])          # increasing batch position


def test_an_index_outside_the_table_is_an_error_code_not_a_fault(shim):
  ql, tl = co.tables(4, 5)
  T, rc = co.shim_forward(shim, ql, tl, np.array([1, 4, -1]))
  assert rc == -1
  assert np.array_equal(T[1], T[2]) and np.array_equal(T[1], co.shim_forward(shim, ql, tl, np.array([0]))[0][0])
  assert co.shim_backward(shim, ql, tl, np.array([1, 4]), None, None, None, co.upstream(2, 6))[1] == -1
  empty, rc = co.shim_forward(shim, ql, tl, np.zeros(0, dtype=np.int64))
  assert rc == 0 and empty.shape == (0, 4, 4)


# ---- containers ---------------------------------------------------------------------------------------------------------

def rigid(n, seed, spread=3.0):
  q, t = co.tables(n, seed, unit=True)
  T = torch.eye(4).repeat(n, 1, 1)
  T[:, :3, :3] = co.rotmat(torch.as_tensor(q))
  T[:, :3, 3] = torch.as_tensor(t) * (spread / co.T_MAX)
  return T


def projections(n):
  return sta.Projections(intrinsics=torch.tensor([[100.0 + i, 110.0 + i, 64.0, 48.0] for i in range(n)]),
                         image_size=torch.tensor([[128, 96]] * n), depth_range=torch.tensor([[0.1, 100.0 + i] for i in range(n)]))


def cameras(n=6, seed=0):
  return sta.Cameras(camera_t_world=rigid(n, seed), projection=projections(n), camera_idx=torch.arange(n) % 2,
                     frame_idx=torch.arange(n) // 2, labels=torch.tensor([2, 1, 2, 2, 1, 3][:n]),
                     image_names=[f"im{i}.png" for i in range(n)], batch_size=(n,))


def test_cameras_index_in_all_four_forms():
  c = cameras()
  assert c.batch_size == (6,) and len(c) == 6 and c.projection.batch_size == (6,)
  one = c[4]
  assert one.batch_size == () and one.image_names == ["im4.png"] and torch.equal(one.camera_t_world, c.camera_t_world[4])
  part = c[1:4]
  assert part.batch_size == (3,) and part.image_names == ["im1.png", "im2.png", "im3.png"]
  assert torch.equal(part.projection.intrinsics, c.intrinsics[1:4])
  picked = c[torch.tensor([5, 0, 5])]
  assert picked.image_names == ["im5.png", "im0.png", "im5.png"] and torch.equal(picked.frame_idx, torch.tensor([2, 0, 2]))
  masked = c[torch.tensor([True, False, False, True, False, False])]
  assert masked.image_names == ["im0.png", "im3.png"] and torch.equal(masked.image_sizes, c.image_sizes[[0, 3]])
  p = c.projection[torch.tensor([2])]
  assert p.batch_size == (1,) and torch.equal(p.depth_range, c.projection.depth_range[2:3])
  assert c.to("cpu").device == torch.device("cpu")
  assert sta.CameraBatch.of(c).camera_t_world.shape == (6, 4, 4)


def test_item_labels_and_camera_params():
  c = cameras()
  assert c.has_label(sta.Label.Training).tolist() == [0, 2, 3, 5] and c.has_label(sta.Label.Validation).tolist() == [1, 4, 5]
  assert c.count_label(sta.Label.Validation) == 3
  assert c.with_label(sta.Label.Validation).image_names == ["im1.png", "im4.png", "im5.png"]
  for cam in (c[3].item(), c[3:4].item()):
    assert isinstance(cam, sta.Camera) and cam.image_name == "im3.png" and cam.camera_idx == 1 and cam.frame_idx == 1
    assert cam.image_size == (128, 96) and cam.depth_range == pytest.approx((0.1, 103.0)) and cam.label == sta.Label.Training
    assert cam.has_label(sta.Label.Training) and not cam.has_label(sta.Label.Validation)
  with pytest.raises(ValueError):
    c.item()
  params = cam.to_camera_params()
  assert isinstance(params, sta.CameraParams) and params.image_size == (128, 96)
  assert torch.equal(params.projection, c.intrinsics[3]) and torch.equal(params.T_camera_world, c.camera_t_world[3])
  assert params.near_plane == pytest.approx(0.1) and params.far_plane == pytest.approx(103.0)
  half = cam.resized(0.5)
  assert half.image_size == (64, 48) and torch.equal(half.intrinsics, cam.intrinsics * 0.5)
  assert half.image_name == cam.image_name and torch.equal(half.camera_t_world, cam.camera_t_world)


def test_scaled_and_translated_keep_rotations_and_move_positions_as_the_reference_states():
  c = cameras()
  R = c.camera_t_world[:, :3, :3]
  v = torch.tensor([0.5, -1.0, 2.0])
  for moved, target in ((c.translated(v), c.positions + v), (c.scaled(2.5), c.positions * 2.5)):
    assert torch.equal(moved.camera_t_world[:, :3, :3], R) and torch.equal(moved.rotations, c.rotations)
    # move_to(t = p): camera_t_world's translation becomes -(R p), camera_table.py:243-249
    assert torch.allclose(moved.camera_t_world[:, :3, 3], -(R @ target.unsqueeze(-1)).squeeze(-1), atol=1e-6)
    assert moved.image_names == c.image_names and torch.equal(moved.labels, c.labels)
  one = c[2].item()
  assert torch.equal(one.translated(v).camera_t_world[:3, :3], one.camera_t_world[:3, :3])
  assert torch.allclose(one.scaled(2.0).camera_t_world[:3, 3],
                        -(one.camera_t_world[:3, :3] @ (one.position * 2.0)), atol=1e-6)


def test_clamp_near_and_replace():
  c = cameras()
  clamped = c.clamp_near(0.5)
  assert torch.equal(clamped.projection.depth_range[:, 0], torch.full((6,), 0.5))
  assert torch.equal(clamped.projection.depth_range[:, 1], c.projection.depth_range[:, 1])
  assert torch.equal(clamped.camera_t_world, c.camera_t_world) and torch.equal(c.projection.depth_range[:, 0], torch.full((6,), 0.1))
  with pytest.raises(TypeError):
    c.replace(nonsense=1)


def test_camera_scene_extents_takes_the_norm_over_the_cameras():
  c = cameras()
  centre, diagonal = sta.camera_scene_extents(c)
  p = c.positions
  assert torch.allclose(centre, p.mean(dim=0))
  assert diagonal == pytest.approx(float(((p - p.mean(dim=0)) ** 2).sum(dim=0).sqrt().max()) * 1.1, rel=1e-6)


def test_pose_adjacency_is_symmetric_and_largest_on_its_diagonal():
  poses = cameras(6, seed=4).world_t_camera
  a = sta.pose_adjacency(poses, poses)
  assert a.shape == (6, 6) and torch.allclose(a, a.t(), atol=1e-6)
  assert torch.equal(a.argmax(dim=1), torch.arange(6)) and torch.allclose(a.diagonal(), torch.ones(6), atol=1e-5)
  c = cameras(6, seed=4)
  assert torch.equal(sta.camera_adjacency_matrix(c), a)
  assert sta.camera_similarity(c, poses[2]).shape == (6, 1)


def test_camera_json_keys():
  out = sta.camera_json(cameras())
  assert len(out) == 6 and [o["id"] for o in out] == list(range(6))
  assert set(out[0]) == {"id", "position", "rotation", "fx", "fy", "cx", "cy", "width", "height", "near", "far", "img_name"}
  assert out[3]["img_name"] == "im3.png" and out[3]["width"] == 128 and out[3]["height"] == 96 and out[3]["fx"] == 103.0
  assert len(out[0]["position"]) == 3 and len(out[0]["rotation"]) == 3


# ---- tables --------------------------------------------------------------------------------------------------------------

def rig_table():
  return sta.CameraRigTable(rig_t_world=rigid(3, 1), camera_t_rig=rigid(2, 2), projection=projections(2),
                            image_names=[f"f{i // 2}c{i % 2}" for i in range(6)], labels=torch.tensor([2, 2, 1, 1, 2, 2]))


def multi_table():
  return sta.MultiCameraTable(camera_t_world=rigid(5, 3), camera_idx=torch.tensor([0, 1, 1, 0, 1]), projection=projections(2),
                              image_names=[f"m{i}" for i in range(5)], labels=torch.tensor([2, 2, 1, 2, 2]))


def test_pose_table_holds_unit_quaternions_of_its_matrices():
  m = rigid(9, 5)
  table = sta.PoseTable(m)
  assert len(table) == 9 and table.q.shape == (9, 4) and table.q.dtype is torch.float32
  assert not table.q.requires_grad and not table.t.requires_grad
  assert torch.allclose(co.rotmat(table.q.double()), m[:, :3, :3].double(), atol=1e-6) and torch.equal(table.t, m[:, :3, 3])
  half_turn = torch.eye(4).repeat(3, 1, 1)                 # the three branches the trace does not take
  for i, d in enumerate(([1, -1, -1], [-1, 1, -1], [-1, -1, 1])):
    half_turn[i, :3, :3] = torch.diag(torch.tensor(d, dtype=torch.float32))
  assert torch.allclose(co.rotmat(sta.PoseTable(half_turn).q.double()), half_turn[:, :3, :3].double(), atol=1e-6)
  table.q.data *= 3.0
  assert torch.allclose(table.normalize().q.norm(dim=1), torch.ones(9), atol=1e-6)
  with pytest.raises(ValueError):
    sta.PoseTable(torch.eye(3))


def test_forward_needs_the_hip_device():
  with pytest.raises(sta.GsplatHipError, match="HIP device"):
    sta.PoseTable(rigid(3, 6))(torch.tensor([0]))
  with pytest.raises(sta.GsplatHipError, match="HIP device"):
    rig_table()[0]
  with pytest.raises(sta.GsplatHipError, match="HIP device"):
    multi_table().cameras


def test_state_dict_round_trip_of_both_tables():
  a, b = rig_table(), multi_table()
  assert set(a.state_dict()) == {"_labels", "_camera_projection.intrinsics", "_camera_projection.image_size",
                                 "_camera_projection.depth_range", "_camera_poses.camera_t_rig.t",
                                 "_camera_poses.camera_t_rig.q", "_camera_poses.rig_t_world.t", "_camera_poses.rig_t_world.q"}
  assert set(b.state_dict()) == {"_labels", "_camera_idx", "_camera_projection.intrinsics", "_camera_projection.image_size",
                                 "_camera_projection.depth_range", "_camera_t_world.t", "_camera_t_world.q"}
  assert not any(p.requires_grad for p in list(a.parameters()) + list(b.parameters()))
  for table, other in ((a, sta.CameraRigTable(rigid(3, 7), rigid(2, 8), projections(2), [""] * 6, torch.zeros(6, dtype=torch.int64))),
                       (b, sta.MultiCameraTable(rigid(5, 9), torch.zeros(5, dtype=torch.int64), projections(2), [""] * 5,
                                                torch.zeros(5, dtype=torch.int64)))):
    other.load_state_dict(table.state_dict())
    for key, value in table.state_dict().items():
      assert torch.equal(other.state_dict()[key], value), key
  assert (len(a), a.num_frames, a.num_projections, a.num_images) == (6, 3, 2, 6)
  assert (len(b), b.num_frames, b.num_projections) == (5, 5, 2) and b.image_names[3] == "m3"
  assert a.projections.image_size.dtype is torch.int64 and a.device == torch.device("cpu")


# ---- normalisation ----------------------------------------------------------------------------------------------------------

def test_normalization_inverse_undoes_rigid_and_points():
  config = sta.NormalizationConfig(centering=True, scaling_method="none")
  points = torch.randn(50, 3, generator=torch.Generator().manual_seed(0)) * 4 + 7
  centred = config.get_transform(points)
  assert centred.scaling == 1.0 and torch.allclose(centred.transform_points(points).mean(dim=0), torch.zeros(3), atol=1e-5)
  norm = sta.Normalization(config=config, translation=torch.tensor([1.0, -2.0, 0.5]), scaling=0.25)
  assert torch.allclose(norm.inverse.transform_points(norm.transform_points(points)), points, atol=1e-5)
  assert torch.allclose(norm.transform_points(points), 0.25 * (points + norm.translation))
  m = rigid(4, 10)
  back = norm.inverse.transform_rigid(norm.transform_rigid(m))
  assert torch.allclose(back, m, atol=1e-5) and torch.equal(norm.transform_rigid(m)[:, :3, :3], m[:, :3, :3])
  c = cameras()
  moved = norm.transform_cameras(c)
  assert torch.equal(moved.rotations, c.rotations)
  with pytest.raises(ValueError):
    sta.NormalizationConfig(scaling_method="nonsense").get_transform(points)
  with pytest.raises(ValueError, match="at most"):
    sta.median_knn(points, k=20)


def test_new_names_are_exported():
  for name in ("Label", "Projections", "Camera", "Cameras", "PoseTable", "RigPoseTable", "CameraTable", "CameraRigTable",
               "MultiCameraTable", "camera_scene_extents", "pose_adjacency", "camera_similarity", "camera_adjacency_matrix",
               "camera_json", "Normalization", "NormalizationConfig"):
    assert name in sta.__all__ and hasattr(sta, name), name
  assert issubclass(sta.CameraRigTable, sta.CameraTable) and ct.check_indices() is None
