"""The pose-table kernels (csrc/camera_table.hip) on the device against the fp64 oracle at the bound measured on the host
build (tests/camera_table_oracle.py: MARGIN x the shim's own error), the tables built on them, and median_knn."""
import numpy as np
import pytest
import torch

import camera_table_oracle as co
import splat_trainer_amd as sta
from splat_trainer_amd import _lib
from splat_trainer_amd import camera_table as ct

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def block_size():
  return int(_lib.load().gsr_pose_block_size())


def dev(a, grad=False):
  return None if a is None else torch.as_tensor(a).to(DEV).requires_grad_(grad)


def run(ql, tl, il, qr=None, tr=None, ir=None, G=None):
  """(T, (d_ql, d_tl, d_qr, d_tr)) of the native calls as numpy arrays."""
  leaves = [dev(a, grad=True) for a in (ql, tl, qr, tr)]
  T = sta.pose_matrices(leaves[0], leaves[1], dev(il), leaves[2], leaves[3], dev(ir))
  grads = (None,) * 4
  if G is not None:
    T.backward(dev(G))
    grads = tuple(None if l is None else l.grad.cpu().numpy() for l in leaves)
  return T.detach().cpu().numpy(), grads


def case(name):
  rng = np.random.default_rng(100)
  if name == "single A=5 B=7":                          # row 3 three times, row 2 never
    return co.tables(5, 20) + (np.array([3, 0, 3, 4, 0, 3, 1]), None, None, None)
  if name == "rig 2x3 B=8":                             # repeats in both indices
    return co.tables(2, 21) + (np.array([1, 0, 1, 1, 0, 0, 1, 0]),) + co.tables(3, 22) + (np.array([2, 2, 0, 2, 1, 0, 0, 2]),)
  if name == "single B=1":
    return co.tables(6, 23) + (np.array([4]), None, None, None)
  if name == "rig B=1":
    return co.tables(3, 24) + (np.array([2]),) + co.tables(4, 25) + (np.array([1]),)
  if name == "single B=65":                             # one more than a wave
    return co.tables(9, 26) + (rng.integers(0, 9, 65), None, None, None)
  if name == "rig B=65":
    return co.tables(4, 27) + (rng.integers(0, 4, 65),) + co.tables(7, 28) + (rng.integers(0, 7, 65),)
  if name == "single A=1":
    return co.tables(1, 29) + (np.zeros(5, dtype=np.int64), None, None, None)
  if name == "rig A=1":
    return co.tables(1, 30) + (np.zeros(5, dtype=np.int64),) + co.tables(1, 31) + (np.zeros(5, dtype=np.int64),)
  A = block_size() + 1                                  # one more row than a block of the backward launch
  if name == "single A=block+1":
    return co.tables(A, 32) + (np.concatenate([rng.integers(0, A, 40), [A - 1, 0]]), None, None, None)
  if name == "rig A=block+1":                           # the left table's last row and the right table's rows share a block
    return co.tables(A, 33) + (np.concatenate([rng.integers(0, A, 40), [A - 1, 0]]),) + co.tables(A, 34) + (
        np.concatenate([rng.integers(0, A, 40), [0, A - 1]]),)
  raise KeyError(name)


CASES = ["single A=5 B=7", "rig 2x3 B=8", "single B=1", "rig B=1", "single B=65", "rig B=65", "single A=1", "rig A=1",
         "single A=block+1", "rig A=block+1"]


@pytest.mark.parametrize("name", CASES)
def test_forward_and_backward_match_the_fp64_oracle(name):
  ql, tl, il, qr, tr, ir = case(name)
  form = "single" if qr is None else "rig"
  G = co.upstream(len(il), 40)
  T, grads = run(ql, tl, il, qr, tr, ir, G)
  forward = co.forward_error(T, co.forward_fp64(ql, tl, il, qr, tr, ir), tl, tr)
  backward = co.backward_error(grads, co.autograd_fp64(ql, tl, il, qr, tr, ir, G), ql, tl, il, qr, tr, ir)
  print(f"{name}: forward {forward:.3e} (bound {co.BOUND_FORWARD[form]:.1e}), backward {backward:.3e} "
        f"(bound {co.BOUND_BACKWARD[form]:.1e})")
  assert np.array_equal(T[:, 3], np.tile(np.float32([0, 0, 0, 1]), (len(il), 1)))
  assert forward <= co.BOUND_FORWARD[form]
  assert backward <= co.BOUND_BACKWARD[form]
  for d, idx in ((grads[0], il), (grads[1], il), (grads[2], ir), (grads[3], ir)):
    if d is not None:
      unselected = np.setdiff1d(np.arange(d.shape[0]), idx)
      assert not d[unselected].any(), "a row no image selected must come back as exact zeros"
  if name == "single A=5 B=7":
    assert np.array_equal(grads[1][3], (G[0, :3, 3] + G[2, :3, 3]) + G[5, :3, 3])      # three terms, in batch order
    assert not grads[0][2].any() and not grads[1][2].any()


def test_zero_quaternion_gives_the_identity():
  q, t = co.tables(3, 41)
  q[1] = 0.0
  T, _ = run(q, t, np.arange(3))
  assert np.array_equal(T[1, :3, :3], np.eye(3, dtype=np.float32)) and np.array_equal(T[1, :3, 3], t[1])


def test_an_empty_batch_returns_an_empty_result():
  q, t = co.tables(3, 42)
  T = sta.pose_matrices(dev(q), dev(t), torch.zeros(0, dtype=torch.int64, device=DEV))
  assert T.shape == (0, 4, 4) and T.dtype is torch.float32 and T.is_cuda
  q2, t2 = co.tables(2, 43)
  empty = torch.zeros(0, dtype=torch.int64, device=DEV)
  assert sta.pose_matrices(dev(q), dev(t), empty, dev(q2), dev(t2), empty).shape == (0, 4, 4)


def test_a_bad_index_raises_and_leaves_the_device_usable():
  q, t = co.tables(4, 44)
  table_q, table_t = dev(q, grad=True), dev(t, grad=True)
  ct.check_indices()
  with pytest.raises(sta.GsplatHipError, match="out of range"):            # a host index: checked before the launch
    sta.pose_matrices(table_q, table_t, torch.tensor([0, 4]))
  with pytest.raises(sta.GsplatHipError, match="out of range"):
    sta.pose_matrices(table_q, table_t, torch.tensor([-1]))
  bad = sta.pose_matrices(table_q, table_t, torch.tensor([1, 4, -1, 2], device=DEV))      # a device index: flagged
  with pytest.raises(sta.GsplatHipError, match="outside its rows"):
    ct.check_indices()
  ct.check_indices()                                                        # the flag is cleared
  good = sta.pose_matrices(table_q, table_t, torch.tensor([1, 0, 0, 2], device=DEV))
  assert torch.equal(bad, good)                                             # the launch read row 0 instead
  bad.sum().backward()                                                      # the backward flags it too, in bounds
  with pytest.raises(sta.GsplatHipError, match="outside its rows"):
    ct.check_indices()
  want = co.forward_fp64(q, t, np.array([1, 0, 0, 2]))
  assert co.forward_error(good.detach().cpu().numpy(), want, t) <= co.BOUND_FORWARD["single"]
  ct.check_indices()


@pytest.mark.parametrize("name", ["rig 2x3 B=8", "rig A=block+1", "single B=65"])
def test_two_runs_are_bit_identical(name):
  ql, tl, il, qr, tr, ir = case(name)
  G = co.upstream(len(il), 45)
  T1, g1 = run(ql, tl, il, qr, tr, ir, G)
  T2, g2 = run(ql, tl, il, qr, tr, ir, G)
  assert np.array_equal(T1, T2)
  for a, b in zip(g1, g2):
    assert (a is None and b is None) or np.array_equal(a, b)


def test_only_the_tables_that_ask_get_a_gradient():
  ql, tl, il, qr, tr, ir = case("rig 2x3 B=8")
  G = co.upstream(len(il), 46)
  _, full = run(ql, tl, il, qr, tr, ir, G)
  q_r, t_r = dev(qr, grad=True), dev(tr, grad=True)
  T = sta.pose_matrices(dev(ql), dev(tl), dev(il), q_r, t_r, dev(ir))
  T.backward(dev(G))
  assert np.array_equal(q_r.grad.cpu().numpy(), full[2]) and np.array_equal(t_r.grad.cpu().numpy(), full[3])


def test_tables_build_cameras_from_image_indices():
  from test_camera_table_host import multi_table, projections, rig_table, rigid
  table = rig_table().to(DEV)
  image_idx = torch.tensor([5, 0, 3])
  cams = table(image_idx)
  assert isinstance(cams, sta.Cameras) and cams.batch_size == (3,) and cams.device.type == "cuda"
  assert cams.frame_idx.tolist() == [2, 0, 1] and cams.camera_idx.tolist() == [1, 0, 1]
  assert cams.image_names == ["f2c1", "f0c0", "f1c1"] and cams.labels.tolist() == [2, 2, 1]
  want = (rigid(2, 2)[[1, 0, 1]].double() @ rigid(3, 1)[[2, 0, 1]].double())
  assert torch.allclose(cams.camera_t_world.cpu().double(), want, atol=1e-5)
  assert torch.equal(cams.projection.intrinsics.cpu(), projections(2).intrinsics[[1, 0, 1]])
  assert len(table.cameras) == 6 and table[4].image_names == ["f2c0"]
  assert sta.CameraBatch.of(table.cameras).camera_t_world.shape == (6, 4, 4)
  assert torch.allclose(table._camera_poses.world_t_rig.cpu() @ rigid(3, 1), torch.eye(4).expand(3, 4, 4), atol=1e-5)
  camera = table[3].item().to_camera_params()
  assert camera.image_size == (128, 96) and camera.T_camera_world.shape == (4, 4)
  multi = multi_table().to(DEV)
  cams = multi(torch.tensor([4, 1], device=DEV))
  assert cams.camera_idx.tolist() == [1, 1] and cams.frame_idx.tolist() == [4, 1] and cams.image_names == ["m4", "m1"]
  assert torch.allclose(cams.camera_t_world.cpu(), rigid(5, 3)[[4, 1]], atol=1e-5)
  assert torch.allclose(multi._camera_t_world[2].cpu(), rigid(5, 3)[2], atol=1e-5)
  with pytest.raises(sta.GsplatHipError, match="out of range"):
    table[6]


def test_median_knn_matches_fp64_brute_force():
  points = torch.randn(500, 3, generator=torch.Generator().manual_seed(3)) * 2.0
  d = torch.cdist(points.double(), points.double()).sort(dim=1).values
  for k in (2, 10, 17):
    want = float(torch.median(d[:, k - 1]))
    got = float(sta.median_knn(points.to(DEV), k=k))
    print(f"median_knn k={k}: {got:.7f} vs {want:.7f}")
    # tests/test_gpu_neighbours.py holds a distance (estimate_scale against fp64) to 1e-6 relative; an order statistic of
    # values that each move by that much moves by no more
    assert abs(got - want) / want < KNN_DISTANCE_TOL
  assert float(sta.median_knn(points.to(DEV), k=1)) == 0.0
  norm = sta.NormalizationConfig(scaling_method="median_knn", normalize_knn=10).get_transform(points.to(DEV))
  assert norm.scaling == pytest.approx(1.0 / float(torch.median(d[:, 9])), rel=2e-6)


KNN_DISTANCE_TOL = 1e-6
