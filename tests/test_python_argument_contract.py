"""The argument contract of the Python wrappers: which exception each public entry point raises for tensors it rejects,
with which words, BEFORE it reaches the device.  Host only: every case below ends in the wrapper's own checks, on CPU
tensors.  (Left out on purpose: a tensor on another device than its neighbours, which no CPU machine can build; the GPU
tests of the modules cover it.)

One table, in the manner of test_abi_argument_contract.py: (entry point, arguments, exception type, a fragment of the
message).  The fragments hold what a caller reads the message for -- the tensor's name and the fault -- and not its
whole wording.  Where two faults meet the table pins which one is reported: within one tensor a wrong shape before a
wrong dtype and both before the device; the colour model alone looks at the device first.  A CPU tensor is a
GsplatHipError in most modules and a ValueError in neighbours, visibility, bilateral and evaluation, as their docstrings
say.
"""
import pytest
import torch

import splat_trainer_amd as sta
from splat_trainer_amd import densify, optim
from splat_trainer_amd.controller import mcmc_draws
from splat_trainer_amd.controller_math import PointState
from splat_trainer_amd.reg import scene_post_step

HIP = sta.GsplatHipError
F16, F64, I32, I64 = torch.float16, torch.float64, torch.int32, torch.int64


def f(*shape, dtype=torch.float32):
  return torch.zeros(*shape, dtype=dtype)


# ---- argument builders: a valid CPU argument set per entry point, with one field replaced ---------------------------
def points(M=5, **over):
  fields = dict(idx=torch.arange(M), depths=torch.ones(M, 1), opacity=torch.rand(M), screen_scale=torch.ones(M, 2),
                visibility=torch.ones(M), prune_cost=f(M), split_score=f(M), attributes=sta.Colors(f(M, 3), f(M, 3)))
  fields.update(over)
  return sta.RenderedPoints(**fields)


def reg(log_scaling=None, **over):
  return lambda: sta.reg_loss(points(**over), f(9, 3) if log_scaling is None else log_scaling, dict(scale=1.0))


def post_step(rotation=None, log_scaling=None):
  return lambda: scene_post_step(f(4, 4) if rotation is None else rotation, f(4, 3) if log_scaling is None else log_scaling)


def noise(**over):
  a = dict(position=f(4, 3), log_scaling=f(4, 3), rotation=f(4, 4), alpha_logit=f(4, 1),
           points_in_view=f(4, dtype=torch.int16))
  a.update(over)
  return lambda: sta.mcmc_noise(a["position"], a["log_scaling"], a["rotation"], a["alpha_logit"], a["points_in_view"],
                                min_views=1, opacity_threshold=0.1, noise_level=1.0, seed=0, step=0)


def poses(q=None, t=None, indices=None):
  return lambda: sta.pose_matrices(f(3, 4) if q is None else q, f(3, 3) if t is None else t,
                                   torch.tensor([0]) if indices is None else indices)


COLOR = sta.ColorModel(sta.ColorModelConfig(hidden_layers=1, sh_degree=2), glo_features=4, point_features=4)


def colors(**over):
  a = dict(point_features=f(5, 4), positions=f(5, 3), cam_pos=f(3), glo_feature=f(1, 4))
  a.update(over)
  return lambda: COLOR(a["point_features"], a["positions"], a["cam_pos"], a["glo_feature"])


def gaussians(N=10, **over):
  a = dict(position=f(N, 3), rotation=f(N, 4), log_scaling=f(N, 3), alpha_logit=f(N, 1), feature=f(N, 3))
  a.update(over)
  return sta.Gaussians3D(**a)


def smooth(rate=None, strength=0.2, **over):
  return lambda: sta.smooth_gaussians(gaussians(**over), f(10) if rate is None else rate, strength)


CAMERAS = sta.CameraBatch(torch.eye(4)[None], torch.ones(1, 4), torch.tensor([[8, 8]]), torch.tensor([[0.1, 10.0]]))
CAMERA = sta.CameraParams(torch.eye(4), torch.ones(4), (32, 32))


def state_update(**over):
  return lambda: densify.point_state_update(PointState.new_zeros(4, device="cpu"), torch.arange(2),
                                            **dict(dict(visibility=f(2)), **over))


def sh_eval(sh=None, positions=None, indexes=None, cam=None):
  return lambda: sta.evaluate_sh_at(f(6, 3, 4) if sh is None else sh, f(6, 3) if positions is None else positions,
                                    torch.arange(2) if indexes is None else indexes, f(3) if cam is None else cam)


def grids(*shape, dtype=torch.float32):
  return f(*(shape or (2, 12, 4, 4, 4)), dtype=dtype)


CASES = [
    # ---- reg: reg_loss, scene_post_step -- shapes and dtypes of all tensors first, the device last
    ("reg_loss", reg(opacity=[0.0] * 5), ValueError, "points.opacity must be a torch.Tensor"),
    ("reg_loss", reg(opacity=f(5, dtype=F64)), ValueError, "points.opacity must be torch.float32"),
    ("reg_loss", reg(idx=torch.arange(5, dtype=I32)), ValueError, "points.idx must be torch.int64"),
    ("reg_loss", reg(idx=f(5, 1, dtype=I64)), ValueError, "points.idx must be"),
    ("reg_loss", reg(depths=f(5, 2)), ValueError, r"points.depths must be \(5, 1\) or \(5,\)"),
    ("reg_loss", reg(visibility=f(4)), ValueError, r"points.visibility must be \(5,\)"),
    ("reg_loss", reg(attributes=sta.Colors(f(5, 2), f(5, 2))), ValueError, r"points.attributes.specular must be \(5, 3\)"),
    ("reg_loss", reg(log_scaling=f(9)), ValueError, "log_scaling must be an"),
    ("reg_loss", reg(log_scaling=f(9, 4)), ValueError, r"log_scaling must be \(9, 3\)"),
    ("reg_loss", reg(), HIP, r"points.idx is on cpu.*regulariser.*no CPU fallback"),
    ("reg_loss", reg(visibility=f(5, dtype=F16)), ValueError, "points.visibility must be torch.float32"),   # dtype < device
    ("reg_loss", reg(log_scaling=f(9, 2)), ValueError, r"log_scaling must be \(9, 3\)"),                    # shape < device
    ("scene_post_step", post_step(rotation=f(4, 3)), ValueError, r"rotation must be \(4, 4\)"),
    ("scene_post_step", post_step(log_scaling=f(4, 3, dtype=F64)), ValueError, "log_scaling must be torch.float32"),
    ("scene_post_step", post_step(log_scaling=f(5, 3)), ValueError, r"log_scaling must be \(4, 3\)"),
    ("scene_post_step", post_step(rotation=f(4, 8)[:, ::2]), ValueError, "contiguous"),                  # contiguity < device
    ("scene_post_step", post_step(), HIP, r"rotation is on cpu.*regulariser.*no CPU fallback"),
    # ---- controller: mcmc_noise, mcmc_draws -- tensor by tensor: shape, dtype, device
    ("mcmc_noise", noise(position=None), ValueError, "position must be a .*NoneType"),
    ("mcmc_noise", noise(position=f(4, 2)), ValueError, "position must .*shape"),
    ("mcmc_noise", noise(position=f(4)), ValueError, "position must .*shape"),
    ("mcmc_noise", noise(position=f(4, 3, dtype=F64)), ValueError, "position must be torch.float32"),    # dtype < device
    ("mcmc_noise", noise(position=f(4, 2, dtype=F64)), ValueError, "position must .*shape"),             # shape < dtype
    ("mcmc_noise", noise(), HIP, r"position is on cpu.*MCMC noise step.*no CPU fallback"),
    ("mcmc_noise", noise(rotation=f(4, 3)), HIP, "position is on cpu"),                          # position wholly first
    ("mcmc_noise", noise(points_in_view=f(4, dtype=I32)), HIP, "position is on cpu"),
    ("mcmc_draws", lambda: mcmc_draws(4, 0, 0, device="cpu"), HIP, "HIP device only.*no CPU fallback"),
    # ---- neighbours: knn, estimate_scale, assign_clusters, kmeans_iter, kmeans -- a CPU tensor is a ValueError
    ("knn", lambda: sta.knn([[0.0, 0.0, 0.0]], 1), ValueError, "points must be a torch.Tensor"),
    ("knn", lambda: sta.knn(f(5, 2), 1), ValueError, "points must .*shape"),
    ("knn", lambda: sta.knn(f(5), 1), ValueError, "points must .*shape"),
    ("knn", lambda: sta.knn(f(5, 3, dtype=F64), 1), ValueError, r"points must be \S*float32"),            # dtype < device
    ("knn", lambda: sta.knn(f(5, 2, dtype=F64), 1), ValueError, "points must .*shape"),                  # shape < dtype
    ("knn", lambda: sta.knn(f(5, 3), 1), ValueError, "points .*HIP device.*no CPU fallback"),
    ("knn", lambda: sta.knn(f(5, 3), 0), ValueError, "points .*HIP device"),                             # points < k
    ("estimate_scale", lambda: sta.estimate_scale(f(5, 4)), ValueError, "points must .*shape"),
    ("estimate_scale", lambda: sta.estimate_scale(f(5, 3, dtype=F16)), ValueError, r"points must be \S*float32"),
    ("estimate_scale", lambda: sta.estimate_scale(f(5, 3)), ValueError, "points .*HIP device"),
    ("assign_clusters", lambda: sta.assign_clusters(None, f(2, 3)), ValueError, "x must be a torch.Tensor"),
    ("assign_clusters", lambda: sta.assign_clusters(f(5, 2), f(2, 3)), ValueError, "x must .*shape"),
    ("assign_clusters", lambda: sta.assign_clusters(f(5, 3), f(2, 3)), ValueError, "x .*HIP device"),
    ("assign_clusters", lambda: sta.assign_clusters(f(5, 3), f(2, 2)), ValueError, "x .*HIP device"),   # x < centroids
    ("kmeans_iter", lambda: sta.kmeans_iter(f(5, 3, dtype=F64), f(2, 3)), ValueError, r"x must be \S*float32"),
    ("kmeans_iter", lambda: sta.kmeans_iter(f(5, 3), f(2, 3), iters=0), ValueError, "x .*HIP device"),  # x < iters
    ("kmeans", lambda: sta.kmeans(f(3, 5, 3), 2), ValueError, "x must .*shape"),
    ("kmeans", lambda: sta.kmeans(f(5, 3), 2), ValueError, "x .*HIP device"),
    # ---- camera_table: pose_matrices -- both shapes, both dtypes, the device, then the indices
    ("pose_matrices", poses(q=f(3, 3)), ValueError, r"the pose table.*q must be \(A, 4\)"),
    ("pose_matrices", poses(t=f(2, 3)), ValueError, r"the pose table.*t .*\(2, 3\)"),
    ("pose_matrices", poses(q=f(3, 4, dtype=F64)), ValueError, "the pose table.*float32"),               # dtype < device
    ("pose_matrices", poses(q=f(3, 3, dtype=F64)), ValueError, r"the pose table.*q must be \(A, 4\)"),    # shape < dtype
    ("pose_matrices", poses(), HIP, "pose table.*HIP device.*no CPU fallback"),
    ("pose_matrices", poses(indices=torch.tensor([7])), HIP, "pose table.*HIP device"),               # table < indices
    # ---- color_model: ColorModel.forward -- tensor by tensor: tensor, DEVICE, dtype; the shapes afterwards
    ("ColorModel.forward", colors(point_features=[1.0]), ValueError, "point_features must be a torch.Tensor"),
    ("ColorModel.forward", colors(), HIP, r"point_features is on cpu.*colour model.*no CPU fallback"),
    ("ColorModel.forward", colors(point_features=f(5, 4, dtype=F16)), HIP, "point_features is on cpu"),   # device < dtype
    ("ColorModel.forward", colors(point_features=f(5, 3)), HIP, "point_features is on cpu"),              # device < shape
    ("ColorModel.forward", colors(positions=None), HIP, "point_features is on cpu"),             # the first tensor first
    # ---- filter3d: smooth_gaussians, sampling_rate
    ("smooth_gaussians", smooth(strength=-1.0), ValueError, "strength"),
    ("smooth_gaussians", smooth(log_scaling=f(10, 2)), ValueError, r"log_scaling must be \(N, 3\)"),
    ("smooth_gaussians", smooth(alpha_logit=f(10)), ValueError, "alpha_logit"),
    ("smooth_gaussians", smooth(log_scaling=f(10, 3, dtype=F16)), ValueError, "float32"),
    ("smooth_gaussians", smooth(rate=[1.0] * 10), ValueError, "rate must be a .*list"),
    ("smooth_gaussians", smooth(rate=f(9)), ValueError, "rate must .*shape"),
    ("smooth_gaussians", smooth(rate=f(10, 1)), ValueError, "rate must .*shape"),
    ("smooth_gaussians", smooth(rate=f(10, dtype=F64)), ValueError, r"rate must be \S*float32"),          # dtype < device
    ("smooth_gaussians", smooth(rate=f(9, dtype=F64)), ValueError, "rate must .*shape"),                 # shape < dtype
    ("smooth_gaussians", smooth(), HIP, r"log_scaling is on cpu.*3-D smoothing filter.*HIP device only"),
    ("sampling_rate", lambda: sta.sampling_rate(CAMERAS, f(3, 3), unseen="max"), ValueError, "unseen"),
    ("sampling_rate", lambda: sta.sampling_rate(CAMERAS, f(3, 3), margin=-0.1), ValueError, "margin"),
    ("sampling_rate", lambda: sta.sampling_rate(CAMERAS, [[0.0] * 3]), ValueError, "points must be a torch.Tensor"),
    ("sampling_rate", lambda: sta.sampling_rate(CAMERAS, f(3, 2)), ValueError, "points must .*shape"),
    ("sampling_rate", lambda: sta.sampling_rate(CAMERAS, f(3, 3, dtype=F64)), ValueError, r"points must be \S*float32"),
    ("sampling_rate", lambda: sta.sampling_rate(CAMERAS, f(3, 3)), ValueError, "points .*HIP device"),
    ("sampling_rate", lambda: sta.sampling_rate(None, f(3, 3)), ValueError, "cannot read cameras"),    # cameras < points
    # ---- visibility: the frustum queries (a CPU tensor is a ValueError)
    ("frustum_counts", lambda: sta.frustum_counts(CAMERAS, f(3, 2)), ValueError, "points must .*shape"),
    ("frustum_counts", lambda: sta.frustum_counts(CAMERAS, f(3, 3, dtype=F16)), ValueError, r"points must be \S*float32"),
    ("frustum_counts", lambda: sta.frustum_counts(CAMERAS, f(3, 3)), ValueError, "points .*HIP device.*no CPU fallback"),
    ("point_visibility", lambda: sta.point_visibility(CAMERAS, None), ValueError, "points must be a torch.Tensor"),
    ("point_visibility", lambda: sta.point_visibility(CAMERAS, f(3, 3)), ValueError, "points .*HIP device"),
    ("camera_counts", lambda: sta.camera_counts(CAMERAS, f(3)), ValueError, "points must .*shape"),
    ("camera_counts", lambda: sta.camera_counts([CAMERA], f(3, 3)), ValueError, "points .*HIP device"),
    ("CameraBatch", lambda: sta.CameraBatch(torch.eye(4), torch.ones(1, 4), torch.tensor([[8, 8]]), f(1, 2)),
     ValueError, "camera_t_world must .*shape"),
    ("CameraBatch", lambda: sta.CameraBatch(torch.eye(4)[None], None, torch.tensor([[8, 8]]), f(1, 2)),
     ValueError, "intrinsics must be a torch.Tensor"),
    ("CameraBatch", lambda: sta.CameraBatch(torch.eye(4)[None], f(1, 4, dtype=F64), torch.tensor([[8, 8]]), f(1, 2)),
     ValueError, r"intrinsics must be \S*float32"),
    ("CameraBatch", lambda: sta.CameraBatch(torch.eye(4)[None], f(1, 4), f(1, 2), f(1, 2)),
     ValueError, "image_sizes must be an integer tensor"),
    # ---- densify: select_n, compact_rows, point_state_update -- the device first
    ("select_n", lambda: densify.select_n(f(5), 2), HIP, "select_n runs only on a HIP device.*no CPU fallback"),
    ("select_n", lambda: densify.select_n(f(5, 2), 2), HIP, "select_n runs only on a HIP device"),       # device < shape
    ("select_n", lambda: densify.select_n(f(5), -1), HIP, "select_n runs only on a HIP device"),          # device < n
    ("compact_rows", lambda: densify.compact_rows(f(5, dtype=torch.bool), []), HIP, "1-D CUDA bool mask"),
    ("compact_rows", lambda: densify.compact_rows(f(5), []), HIP, "1-D CUDA bool mask"),
    ("point_state_update", state_update(), HIP, "contiguous float32 CUDA state tensors"),
    ("point_state_update", state_update(visible_sum=f(3)), HIP, "contiguous float32 CUDA state tensors"),
    # ---- loss: fused_ssim, clamped_mse_loss, clamped_l1_loss -- the shape first
    ("fused_ssim", lambda: sta.fused_ssim(f(1, 3, 16, 16), f(1, 3, 16, 16), padding="full"), ValueError, "padding"),
    ("fused_ssim", lambda: sta.fused_ssim(f(3, 16, 16), f(3, 16, 16)), ValueError, r"\(B,C,H,W\)"),       # shape < device
    ("fused_ssim", lambda: sta.fused_ssim(f(1, 3, 16, 16), f(1, 3, 16, 12)), ValueError, "equal shape"),
    ("fused_ssim", lambda: sta.fused_ssim(f(1, 3, 16, 16), f(1, 3, 16, 16)), HIP, "fused_ssim runs only on a HIP device"),
    ("fused_ssim", lambda: sta.fused_ssim(f(1, 3, 8, 8), f(1, 3, 8, 8), padding="valid"), HIP, "HIP device"),  # device < size
    ("clamped_mse_loss", lambda: sta.clamped_mse_loss(f(8, 8, 3), f(8, 8, 3)), HIP, "pixel losses run only on a HIP device"),
    ("clamped_mse_loss", lambda: sta.clamped_mse_loss(f(8, 8, 3, dtype=F16), f(8, 8, 3)), HIP, "HIP device"),
    ("clamped_l1_loss", lambda: sta.clamped_l1_loss(f(8, 8, 3), f(8, 8, 3)), HIP, "pixel losses run only on a HIP device"),
    # ---- evaluation: fit_colors_batch, image_metrics -- a CPU tensor is a ValueError
    ("fit_colors_batch", lambda: sta.fit_colors_batch(f(4, 4, 3), f(4, 5, 3)), ValueError, "same shape"),   # shape < device
    ("fit_colors_batch", lambda: sta.fit_colors_batch(f(4, 4, 4), f(4, 4, 4)), ValueError, "three channels"),
    ("fit_colors_batch", lambda: sta.fit_colors_batch(f(4, 4, 3), f(4, 4, 3)), ValueError, "HIP device.*no CPU fallback"),
    ("fit_colors_batch", lambda: sta.fit_colors_batch(f(4, 4, 3), f(4, 4, 3), num_iters=99), ValueError, "HIP device"),
    ("image_metrics", lambda: sta.image_metrics(f(16, 16, 4), f(16, 16, 4)), ValueError, r"\(H, W, 3\)"),
    ("image_metrics", lambda: sta.image_metrics(f(16, 16, 3), f(16, 12, 3)), ValueError, "equal shape"),
    ("image_metrics", lambda: sta.image_metrics(f(16, 16, 3), f(16, 16, 3)), ValueError, "HIP device.*no CPU fallback"),
    ("image_metrics", lambda: sta.image_metrics(f(8, 8, 3), f(8, 8, 3)), ValueError, "HIP device"),       # device < size
    # ---- optim: point_basis_rows
    ("point_basis_rows", lambda: optim.point_basis_rows(f(4, 3), f(4, 4)), HIP, "point_basis_rows runs only on a HIP device"),
    ("point_basis_rows", lambda: optim.point_basis_rows(f(4, 3, dtype=F16), f(4, 4)), HIP, "HIP device"),
    # ---- sh: evaluate_sh_at -- the device first
    ("evaluate_sh_at", sh_eval(), HIP, "evaluate_sh_at runs only on a HIP device.*no CPU fallback"),
    ("evaluate_sh_at", sh_eval(sh=f(6, 3, 5)), HIP, "evaluate_sh_at runs only on a HIP device"),          # device < shape
    ("evaluate_sh_at", sh_eval(indexes=torch.arange(2, dtype=I32)), HIP, "evaluate_sh_at runs only"),     # device < dtype
    # ---- renderer: project_to_image, render_projected, render_gaussians -- the device first
    ("project_to_image", lambda: sta.project_to_image(gaussians(), CAMERA, sta.RasterConfig()), HIP,
     "rasterizer path runs only on a HIP device.*no CPU fallback"),
    ("project_to_image", lambda: sta.project_to_image(gaussians(position=f(10, 3, dtype=torch.int8)), CAMERA,
                                                      sta.RasterConfig()), HIP, "rasterizer path runs only"),
    ("render_projected", lambda: sta.render_projected(torch.arange(4), f(4, 6), f(4, 3), f(4, 1), CAMERA,
                                                      sta.RasterConfig()), HIP, "rasterizer path runs only on a HIP device"),
    ("render_projected", lambda: sta.render_projected(torch.arange(4), f(4, 6), f(4), f(4, 1), CAMERA, sta.RasterConfig()),
     HIP, "rasterizer path runs only"),                                                               # device < shape
    ("render_gaussians", lambda: sta.render_gaussians(gaussians(), CAMERA), HIP, "rasterizer path runs only"),
    # ---- bilateral: bilateral_correct, bilateral_tv_loss -- the grids first; a CPU tensor is a ValueError
    ("bilateral_correct", lambda: sta.bilateral_correct(grids(12, 4, 4, 4), 0, f(8, 8, 3)), ValueError, "grids must have shape"),
    ("bilateral_correct", lambda: sta.bilateral_correct(grids(2, 12, 1, 4, 4), 0, f(8, 8, 3)), ValueError, "grid dimensions"),
    ("bilateral_correct", lambda: sta.bilateral_correct(grids(dtype=F64), 0, f(8, 8, 3)), ValueError,
     "contiguous float32"),                                                                           # dtype < device
    ("bilateral_correct", lambda: sta.bilateral_correct(grids(), 0, f(8, 8, 3)), ValueError, "HIP device.*no CPU fallback"),
    ("bilateral_correct", lambda: sta.bilateral_correct(grids(), 0, f(8, 8, 4)), ValueError, "HIP device"),  # grids < image
    ("bilateral_tv_loss", lambda: sta.bilateral_tv_loss(grids(2, 11, 4, 4, 4)), ValueError, "grids must have shape"),
    ("bilateral_tv_loss", lambda: sta.bilateral_tv_loss(grids()), ValueError, "HIP device.*no CPU fallback"),
    # ---- sh_fit: ShFit -- the degree, the shape, the device
    ("ShFit", lambda: sta.ShFit(f(5, 3), 7), ValueError, "sh_degree"),
    ("ShFit", lambda: sta.ShFit([[0.0] * 3], 2), ValueError, "positions must be a .*list"),
    ("ShFit", lambda: sta.ShFit(f(5, 2), 2), ValueError, "positions must .*shape"),                      # shape < device
    ("ShFit", lambda: sta.ShFit(f(5), 2), ValueError, "positions must .*shape"),
    ("ShFit", lambda: sta.ShFit(f(5, 3), 2), HIP, r"positions is on cpu.*SH fit.*HIP device only"),
    ("ShFit", lambda: sta.ShFit(f(5, 3, dtype=F64), 2), HIP, "positions is on cpu"),                  # (dtype: converted)
    ("fit_sh", lambda: sta.fit_sh(None, None, [], [], f(5, 3)), HIP, "positions is on cpu"),
]


@pytest.mark.parametrize("entry, call, error, fragment", CASES,
                         ids=[f"{i:03d}-{c[0]}" for i, c in enumerate(CASES)])
def test_python_argument_contract(entry, call, error, fragment):
  with pytest.raises(error, match=fragment) as raised:
    call()
  assert type(raised.value) is error, (entry, type(raised.value))          # the documented type itself, not a subclass
