"""The 3-D smoothing filter without a GPU: the oracle's own consistency (tests/filter3d_oracle.py), the float32
restatement of the kernels' stable form against the plain fp64 definition over the ranges the scene can reach, the
per-row and per-pair maths of csrc/gsr_filter3d.h compiled for the host (the shim) against the same oracles, the derived
binding, and that a scene with the filter off carries nothing new.

`python tests/test_filter3d_host.py` prints the measured figures (profiles/r17_filter3d.txt)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter3d_oracle as fo  # noqa: E402
import hostmath  # noqa: E402
import visibility_oracle as vo  # noqa: E402
import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import _lib, visibility as vis  # noqa: E402

ROWS = 200_000
BOUND_OUT, BOUND_GRAD = fo.MARGIN * fo.RESTATEMENT_OUT, fo.MARGIN * fo.RESTATEMENT_GRAD


def _note(line: str):
  print(line)


@pytest.fixture(scope="module")
def shim(built_libs):
  return hostmath.load(built_libs)


@pytest.fixture(scope="module")
def rows():
  ls, a, rate = fo.random_rows(ROWS, seed=1)
  c64 = fo.variance_fp64(rate)
  return dict(ls=ls, a=a, rate=rate, c32=fo.variance_f32(rate), c64=c64, out=fo.smooth_fp64(ls, a, c64),
              partials=fo.partials_fp64(ls, a, c64))


# ------------------------------------------------------------------------------------------------- oracle self-checks
def test_oracle_preserves_the_integral():
  """opacity' prod sigma'_j == opacity prod sigma_j: what the normalisation is for."""
  ls, a, rate = fo.random_rows(20_000, seed=2)
  out_ls, out_a = fo.smooth_fp64(ls, a, fo.variance_fp64(rate))
  sig = lambda x: 1.0 / (1.0 + np.exp(-x))
  before = sig(a.astype(np.float64)) * np.exp(ls.astype(np.float64).sum(1))
  after = sig(out_a) * np.exp(out_ls.sum(1))
  err = np.max(np.abs(after / before - 1.0))
  _note(f"integral: max |after / before - 1| = {err:.2e}")
  # a', fp64, comes out of logit(q) with 1 - q as small as sigmoid(-12) = 6e-6: 2^-53 / 6e-6 = 2e-11 relative on 1 - q, and
  # q itself is good to a few 2^-53; the three logs add as many
  assert err < 1e-10


def test_oracle_tends_to_the_identity():
  ls, a, _ = fo.random_rows(5_000, seed=3, corners=False)
  zero = fo.smooth_fp64(ls, a, np.zeros(len(a)))
  assert np.max(np.abs(zero[0] - ls)) < 1e-14 and fo.out_error(zero[1], a) < 1e-10
  previous = None
  for c in (1e-6, 1e-10, 1e-14):
    # |ls' - ls| = log1p(c exp(-2 ls)) / 2 <= c exp(16) / 2, and |a' - a| <= |lc| / (1 - q) <= 1.5 c exp(16) / sigmoid(-12): linear in c
    out_ls, out_a = fo.smooth_fp64(ls, a, np.full(len(a), c))
    gap = max(np.max(np.abs(out_ls - ls)), np.max(np.abs(out_a - a)))
    assert gap <= 2.0 * c * np.exp(16.0) / 6e-6 and (previous is None or gap < previous)
    previous = gap


def test_oracle_gradients_agree_with_central_differences():
  ls, a, _ = fo.random_rows(4_000, seed=4, corners=False)
  ls, a = ls.astype(np.float64) / 4, a.astype(np.float64) / 2          # well inside fp64's range for a difference quotient
  c = 10.0 ** np.random.default_rng(5).uniform(-3, 1, len(a))
  dls_dls, da_da, da_dls, _ = fo.partials_fp64(ls, a, c)
  h = 1e-5
  f = lambda ls_, a_: fo.smooth_fp64(ls_, a_, c)
  num_da = (f(ls, a + h)[1] - f(ls, a - h)[1]) / (2 * h)
  assert np.max(np.abs(num_da - da_da) / np.abs(da_da)) < 1e-7          # h^2 f''' / 6 and 2^-53 / h
  for j in range(3):
    e = np.zeros(3)
    e[j] = h
    up, down = f(ls + e, a), f(ls - e, a)
    num_ls = (up[0][:, j] - down[0][:, j]) / (2 * h)
    num_a = (up[1] - down[1]) / (2 * h)
    assert np.max(np.abs(num_ls - dls_dls[:, j])) < 1e-7
    assert np.max(np.abs(num_a - da_dls[:, j]) / np.maximum(np.abs(da_dls[:, j]), 1e-3)) < 1e-6


# ------------------------------------------------------------------------- the float32 restatement against plain fp64
def test_restatement_stays_inside_four_times_its_measured_error(rows):
  got_ls, got_a = fo.smooth_f32(rows["ls"], rows["a"], rows["c32"])
  e_ls, e_a = fo.out_error(got_ls, rows["out"][0]), fo.out_error(got_a, rows["out"][1])
  e_p = fo.partial_errors(fo.partials_f32(rows["ls"], rows["a"], rows["c32"]), rows["partials"])
  _note(f"restatement vs plain fp64, {ROWS} rows: ls' {e_ls:.2e}  a' {e_a:.2e} of max(1, |value|) (bound {BOUND_OUT:.2e}); "
        f"d ls'/d ls {e_p[0]:.2e}  d a'/d a {e_p[1]:.2e}  d a'/d ls {e_p[2]:.2e} relative (bound {BOUND_GRAD:.2e}); "
        f"a' reaches {rows['out'][1].min():.1f}")
  assert np.isfinite(got_ls).all() and np.isfinite(got_a).all()
  assert max(e_ls, e_a) < BOUND_OUT
  # d ls'_j / d ls_j = 1 / (1 + u_j) was not measured with the other two: it is a subset of their operations (one exp, one
  # product, one sum, one division), so the same bound holds it
  assert max(e_p) < BOUND_GRAD


def test_naive_form_breaks_the_bound(rows):
  """logit(sigmoid(a) coef) in float32 cancels in 1 - q: the check above would catch a regression to it."""
  naive = fo.naive_f32(rows["ls"], rows["a"], rows["c32"])
  finite = np.isfinite(naive)
  e = fo.out_error(naive[finite], rows["out"][1][finite])
  _note(f"naive float32 logit: {e:.2e} of max(1, |value|) on the {finite.mean():.4f} of the rows where it is finite")
  assert e > 100 * BOUND_OUT


def test_rows_without_added_variance_are_copied(shim):
  ls, a, rate = fo.random_rows(1_000, seed=6)
  rate[::3] = 0
  keep = rate == 0
  g = np.random.default_rng(7).standard_normal((1_000, 4)).astype(np.float32)
  g_ls, g_a = np.ascontiguousarray(g[:, :3]), np.ascontiguousarray(g[:, 3])
  for fwd, bwd in ((fo.shim_forward(shim, ls, a, rate), fo.shim_backward(shim, ls, a, rate, g_ls, g_a)),
                   (fo.smooth_f32(ls, a, fo.variance_f32(rate)), fo.backward_f32(ls, a, fo.variance_f32(rate), g_ls, g_a))):
    assert fwd[0][keep].tobytes() == ls[keep].tobytes() and fwd[1][keep].tobytes() == a[keep].tobytes()
    assert bwd[0][keep].tobytes() == g_ls[keep].tobytes() and bwd[1][keep].tobytes() == g_a[keep].tobytes()
    assert not np.array_equal(fwd[0][~keep], ls[~keep])
  zero = fo.shim_forward(shim, ls, a, rate, strength=0.0)
  assert zero[0].tobytes() == ls.tobytes() and zero[1].tobytes() == a.tobytes()


def test_header_maths_on_the_host_matches_the_oracle(shim, rows):
  """csrc/gsr_filter3d.h compiled for the host (same source as the device, the host's libm): inside the same bound."""
  n = 50_000
  ls, a, rate = rows["ls"][:n], rows["a"][:n], rows["rate"][:n]
  got_ls, got_a = fo.shim_forward(shim, ls, a, rate)
  e = fo.out_error(got_ls, rows["out"][0][:n]), fo.out_error(got_a, rows["out"][1][:n])
  zeros3, ones3 = np.zeros((n, 3), np.float32), np.ones((n, 3), np.float32)
  zeros1, ones1 = np.zeros(n, np.float32), np.ones(n, np.float32)
  dls_dls, _ = fo.shim_backward(shim, ls, a, rate, ones3, zeros1)
  da_dls, da_da = fo.shim_backward(shim, ls, a, rate, zeros3, ones1)
  e_p = fo.partial_errors((dls_dls, da_da, da_dls), tuple(t[:n] for t in rows["partials"]))
  _note(f"header maths on the host vs plain fp64, {n} rows: ls' {e[0]:.2e}  a' {e[1]:.2e};  partials " +
        "  ".join(f"{x:.2e}" for x in e_p))
  assert max(e) < BOUND_OUT and max(e_p) < BOUND_GRAD


# ------------------------------------------------------------------------------------------------------ sampling rate
@pytest.mark.parametrize("V", [1, 5, 65])
@pytest.mark.parametrize("margin", [0.0, 0.15])
def test_host_rate_sits_in_the_fp64_sandwich(shim, V, margin):
  cams = fo.ring_cameras(V)
  records = vo.camera_batch(vis, cams).records().numpy()
  focal = fo.focal_of(cams[1])
  assert (cams[1][:, 0] > cams[1][:, 1]).any() or V == 1
  points = fo.ring_points(4099, seed=V)
  b = fo.rate_bounds_fp64(points, records, focal, margin)
  rate = fo.shim_sampling_rate(shim, points, records, focal, margin)
  unsampled, undecided = float(np.mean(b["U"] == 0)), float(np.mean(b["L"] != b["U"]))
  _note(f"host rate V={V} margin={margin}: unsampled {unsampled:.3f}  L != U {undecided:.2e}  band pairs {b['band']}")
  assert undecided <= 1e-3
  if V >= 64:
    assert 0.10 <= unsampled <= 0.30
  assert fo.inside_sandwich(rate, b).all()
  assert np.array_equal(rate == 0, b["U"] == 0) or undecided > 0
  # the likely wrong implementations leave the sandwich
  if margin > 0:
    assert not fo.inside_sandwich(fo.shim_sampling_rate(shim, points, records, focal, 0.0), b).all()
  no_far = records.copy()
  no_far[:, 15] = 1e9
  assert not fo.inside_sandwich(fo.shim_sampling_rate(shim, points, no_far, focal, margin), b).all()
  only_fx = fo.shim_sampling_rate(shim, points, records, cams[1][:, 0].copy(), margin)
  assert V == 1 or not fo.inside_sandwich(only_fx, b).all()


def test_sandwich_bites_on_every_point_of_the_constructed_scene(shim):
  cams = fo.ring_cameras(65)
  records = vo.camera_batch(vis, cams).records().numpy()
  focal = fo.focal_of(cams[1])
  points = fo.far_from_every_bound(1000)
  b = fo.rate_bounds_fp64(points, records, focal, 0.15)
  assert b["band"] == 0 and np.array_equal(b["L"], b["U"])
  assert 0.4 < np.mean(b["U"] == 0) < 0.6
  rate = fo.shim_sampling_rate(shim, points, records, focal, 0.15)
  assert fo.inside_sandwich(rate, b).all()
  assert np.array_equal(rate == 0, b["U"] == 0)


# ------------------------------------------------------------------------------------------------------------ binding
def test_entry_points_are_in_the_derived_binding():
  f, fp, i64, vp = C.c_float, "const float*", "int64_t", "void*"
  want = {
      "gsr_sampling_rate": ("int", [fp, i64, fp, fp, i64, "float", "float*", vp]),
      "gsr_filter3d_forward": ("int", [fp, fp, fp, i64, "float", "float*", "float*", vp]),
      "gsr_filter3d_backward": ("int", [fp, fp, fp, i64, "float", fp, fp, "float*", "float*", vp]),
  }
  for name, signature in want.items():
    assert _lib.FUNCTIONS[name] == signature, name
    restype, argtypes = _lib.PROTOTYPES[name]
    assert restype is C.c_int and len(argtypes) == len(signature[1])
    assert [t is f for t in argtypes] == [s == "float" for s in signature[1]]
    assert [t is C.c_int64 for t in argtypes] == [s == i64 for s in signature[1]]
    assert all(t is C.c_void_p for t, s in zip(argtypes, signature[1]) if s.endswith("*"))


def test_library_exports_the_entry_points(built_libs):
  lib = C.CDLL(built_libs[0])
  for name in ("gsr_sampling_rate", "gsr_filter3d_forward", "gsr_filter3d_backward"):
    assert hasattr(lib, name)


# -------------------------------------------------------------------------------------------------------------- scene
def test_filter_is_off_by_default_and_adds_no_state():
  fields = sta.MLPSceneConfig.__dataclass_fields__
  assert fields["filter_3d"].default == 0.0
  parameters = dict(position=dict(lr=0.003, type="local_vector"), log_scaling=dict(lr=0.005),
                    rotation=dict(lr=0.001, type="vector"), alpha_logit=dict(lr=0.01), feature=dict(lr=0.5, type="vector"))
  config = sta.MLPSceneConfig(parameters=parameters, reg_weight=dict(scale=0.1), filter_3d=0,
                              color_model=sta.ColorModelConfig(hidden_layers=1, sh_degree=2))
  g = sta.Gaussians3D(position=torch.randn(10, 3), rotation=torch.randn(10, 4), log_scaling=torch.randn(10, 3),
                      alpha_logit=torch.randn(10, 1), feature=torch.rand(10, 3))
  scene = config.from_color_gaussians(g, 2, "cpu", seed=0)
  state = scene.state_dict()
  assert sorted(state) == ["color_model", "color_opt", "color_table", "glo_opt", "points"]
  assert sorted(state["points"]["tensors"]) == ["alpha_logit", "feature", "log_scaling", "position", "rotation", "visible"]
  assert scene._filtered_gaussians().log_scaling is scene.points.log_scaling
  with pytest.raises(ValueError, match="filter_3d > 0"):
    scene.update_filter([])


def test_smooth_gaussians_checks_its_arguments():
  g = sta.Gaussians3D(position=torch.randn(10, 3), rotation=torch.randn(10, 4), log_scaling=torch.randn(10, 3),
                      alpha_logit=torch.randn(10, 1), feature=torch.rand(10, 3))
  with pytest.raises(sta.GsplatHipError, match="HIP device only"):
    sta.smooth_gaussians(g, torch.ones(10))
  with pytest.raises(ValueError, match="shape"):
    sta.smooth_gaussians(g, torch.ones(9))
  with pytest.raises(ValueError, match="shape"):
    sta.smooth_gaussians(g, torch.ones(10, 1))
  with pytest.raises(ValueError, match="float32"):
    sta.smooth_gaussians(g, torch.ones(10, dtype=torch.float64))
  with pytest.raises(ValueError, match="unseen"):
    sta.sampling_rate([], torch.zeros(3, 3), unseen="max")


if __name__ == "__main__":
  sys.exit(pytest.main([__file__, "-s", "-q"]))
