"""MI355X-native differentiable Gaussian-splat rasterizer: drop-in for the taichi_splatting calls
splat-trainer makes at its render boundary.

Import as ``splat_trainer_amd`` (the repo-root shim ``splat_trainer_amd.py`` loads this directory,
whose name carries a hyphen)."""
from .data_types import (CameraParams, Gaussians3D, RasterConfig, RenderedPoints, Rendering,
                         pop_raster_config)
from .renderer import GradOut, frustum_cull, project_to_image, render_gaussians, render_projected
from .sh import ShFactorCollector, evaluate_sh_at
from .loss import clamped_l1_loss, clamped_mse_loss, fused_ssim, reference_loss
from ._lib import GsplatHipError
from .bilateral import (BilateralCorrector, BilateralCorrectorConfig, BilateralGrid, bilateral_correct,
                        bilateral_tv_loss)
from .neighbours import assign_clusters, estimate_scale, kmeans, kmeans_iter, knn
from .color_model import ColorModel, ColorModelConfig, Colors
from .reg import reg_loss
from .mlp_scene import MLPScene, MLPSceneConfig
from .visibility import (BatchOverlapSampler, BatchOverlapSamplerConfig, CameraBatch, PointClusters, RandomSampler,
                         RandomSamplerConfig, ViewClustering, balanced_cloud, balanced_points, camera_counts, crop_cloud,
                         foreground_points, foreground_visibility, frustum_counts, inverse_ndc_depth, point_visibility,
                         random_cloud, random_ndc, random_points, sample_batch, sample_batch_grouped,
                         sample_with_temperature, select_batch, sinkhorn)
from .evaluation import (Evaluation, compute_psnr, evaluate_scene, fit_colors, fit_colors_batch, image_metrics,
                         mse_to_psnr)
from .filter3d import sampling_rate, smooth_gaussians
from .sh_fit import ShFit, fit_sh
from .controller import (Controller, ControllerConfig, DisabledConfig, DisabledController, MCMCConfig, MCMCController,
                         Progress, TargetConfig, TargetController, densify_and_prune, grow_points, growth_target,
                         mcmc_noise, relocate_points, relocate_rescale, relocate_rows, relocate_weights, weighted_draws)
from .camera_table import (Camera, CameraRigTable, CameraTable, Cameras, Label, MultiCameraTable, PoseTable, Projections,
                           RigPoseTable, camera_adjacency_matrix, camera_json, camera_scene_extents, camera_similarity,
                           check_indices, pose_adjacency, pose_matrices)
from .normalization import Normalization, NormalizationConfig, median_knn
from .histogram import Histogram, tensor_histogram
from .image import resize_area
from .undistort import LensCamera, Undistortion, optimal_pinhole, remap, undistort_map
from .fusion import (FusionConfig, depth_consistency, fuse_depth_maps, fuse_scene, select_sources,
                     voxel_downsample)
from .mesh import TriangleMesh, TsdfConfig, TsdfVolume, mesh_depth_maps, mesh_scene
from .normals import depth_normals, geometry_features, normal_consistency_loss, splat_normals
from .colmap_io import read_model, write_model
from .colmap import COLMAPDataset, export_colmap
from .logger import (CompositeLogger, HistoryLogger, Logger, LoggerWithState, NullLogger, StateLogger, StateTree,
                     StepValue)
from .dataset import Dataset, ImageView, PointCloud, TensorDataset, expand_index, partition_stride, split_every
from .cloud_init import (CloudInitConfig, from_pointcloud, from_scaled_pointcloud, get_initial_gaussians,
                         to_pointcloud)
from .visibility import TargetOverlap, TargetOverlapConfig
from .trainer import (NaNParameterException, NoProgressException, TrainConfig, Trainer, TrainerState,
                      TrainingException, TrainingTimeoutException, find_checkpoint, load_checkpoint)
from .compat import TaichiQueue, check_finite, count_nonfinite, random_3d_gaussians, random_camera

__all__ = ["CameraParams", "Gaussians3D", "RasterConfig", "RenderedPoints", "Rendering", "pop_raster_config",
           "frustum_cull", "project_to_image", "render_projected", "render_gaussians", "evaluate_sh_at",
           "GsplatHipError", "GradOut", "fused_ssim", "clamped_mse_loss", "clamped_l1_loss", "reference_loss", "ShFactorCollector", "TaichiQueue", "count_nonfinite",
           "check_finite", "random_camera", "random_3d_gaussians", "BilateralCorrector", "BilateralCorrectorConfig",
           "BilateralGrid", "bilateral_correct", "bilateral_tv_loss", "knn", "estimate_scale", "assign_clusters",
           "kmeans_iter", "kmeans", "ColorModel", "ColorModelConfig", "Colors", "reg_loss", "MLPScene", "MLPSceneConfig",
           "CameraBatch", "point_visibility", "camera_counts", "frustum_counts", "crop_cloud", "random_ndc",
           "inverse_ndc_depth", "random_points", "balanced_points", "random_cloud", "balanced_cloud",
           "foreground_visibility", "foreground_points", "PointClusters", "ViewClustering", "sample_with_temperature",
           "select_batch", "sample_batch", "sample_batch_grouped", "sinkhorn", "BatchOverlapSampler",
           "BatchOverlapSamplerConfig", "RandomSampler", "RandomSamplerConfig", "Evaluation", "compute_psnr",
           "mse_to_psnr", "fit_colors", "fit_colors_batch", "image_metrics", "evaluate_scene", "sampling_rate",
           "smooth_gaussians", "ShFit", "fit_sh", "Progress", "ControllerConfig", "Controller", "DisabledConfig",
           "DisabledController", "TargetConfig", "TargetController", "MCMCConfig", "MCMCController", "densify_and_prune",
           "mcmc_noise", "Label", "Projections", "Camera", "Cameras", "PoseTable", "RigPoseTable", "CameraTable",
           "CameraRigTable", "MultiCameraTable", "camera_scene_extents", "pose_adjacency", "camera_similarity",
           "camera_adjacency_matrix", "camera_json", "pose_matrices", "check_indices", "Normalization",
           "NormalizationConfig", "median_knn", "Histogram", "tensor_histogram", "Logger", "NullLogger", "CompositeLogger",
           "StateLogger", "HistoryLogger", "LoggerWithState", "StateTree", "StepValue", "ImageView", "Dataset",
           "PointCloud", "TensorDataset", "split_every", "partition_stride", "expand_index", "CloudInitConfig",
           "from_pointcloud", "from_scaled_pointcloud", "to_pointcloud", "get_initial_gaussians", "TargetOverlapConfig",
           "TargetOverlap", "TrainConfig", "TrainerState", "TrainingException", "NaNParameterException",
           "NoProgressException", "TrainingTimeoutException", "find_checkpoint", "load_checkpoint", "Trainer",
           "resize_area", "LensCamera", "Undistortion", "optimal_pinhole", "undistort_map", "remap", "read_model",
           "write_model", "COLMAPDataset", "export_colmap", "weighted_draws", "relocate_weights", "relocate_rescale",
           "relocate_rows", "relocate_points", "grow_points", "growth_target", "FusionConfig", "depth_consistency",
           "select_sources", "fuse_depth_maps", "voxel_downsample", "fuse_scene", "TsdfConfig", "TsdfVolume", "TriangleMesh",
           "mesh_depth_maps", "mesh_scene", "splat_normals", "geometry_features", "depth_normals",
           "normal_consistency_loss"]
