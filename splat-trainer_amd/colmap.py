"""``COLMAPDataset``: the reference's ``dataset/colmap`` loader without pycolmap and cv2, and ``export_colmap``, its
``scripts/to_colmap.py``.  The model files are read by ``colmap_io``, the images decoded by PIL, and the resize that
``image_scale`` / ``resize_longest`` ask for is the native area resize (``image.resize_area``: csrc/image.hip on the
dataset's device, the same arithmetic on the host when there is no GPU -- the two give the same bytes).

Deliberate deviations from the reference: images come in ascending ``image_id`` (``colmap_io``), so the split is defined
by the files alone; SIMPLE_PINHOLE is accepted beside PINHOLE and any other model raises ``ValueError`` (the reference
asserts) unless ``undistort=True``, which takes SIMPLE_RADIAL, RADIAL and OPENCV cameras too: their images are remapped
onto the optimal pinhole view of the same size (``undistort.Undistortion``, csrc/undistort.hip) before the resize, and
the projection table holds that view; a scale above 1 raises, because the resize only shrinks; the normalisation is fitted on the host in float64
(``median_knn`` over the camera centres needs no device and has no limit on ``normalize_knn``); a model without points
gives ``pointcloud() is None``.  The resize is the exact area mean rounded half up, where cv2's ``INTER_AREA`` computes
the same mean in float ("COLMAP datasets").
"""
from __future__ import annotations

import os
from multiprocessing.pool import ThreadPool
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import colmap_io
from .camera_table import CameraTable, Label, MultiCameraTable, Projections, rotmat_to_unitquat, split_rt
from .dataset import Dataset, ImageView, PointCloud, split_every
from .image import resize_area
from .normalization import Normalization, NormalizationConfig
from .undistort import LensCamera, Undistortion, to_colmap_intrinsics

STAGING_BYTES = 256 << 20            # full-resolution images held at once while loading
DISTORTED_MODELS = ("SIMPLE_RADIAL", "RADIAL", "OPENCV")      # what undistort=True takes beside the pinhole models


def decode_threads() -> int:
  return max(1, min(16, (os.cpu_count() or 2) // 2))


def colmap_projection(camera: colmap_io.Camera, image_scale: Optional[float] = None, resize_longest: Optional[int] = None,
                      undistortion: Optional[Undistortion] = None) -> Tuple[np.ndarray, Tuple[int, int]]:
  """(fx, fy, cx, cy as float64, (width, height)) of a PINHOLE or SIMPLE_PINHOLE camera after the resize: intrinsics
  times the scale and ``round`` of the scaled size, as the reference computes them.  With ``undistortion`` (of this
  camera) the intrinsics are its target's, taken back to COLMAP's pixel-centre convention, whatever the model."""
  if undistortion is not None:
    proj = np.array(to_colmap_intrinsics(undistortion.target), np.float64)
  elif camera.model == "PINHOLE":
    proj = np.array(camera.params, np.float64)
  elif camera.model == "SIMPLE_PINHOLE":
    f, cx, cy = (float(v) for v in camera.params)
    proj = np.array([f, f, cx, cy], np.float64)
  else:
    raise ValueError(f"camera model {camera.model} is not supported: only PINHOLE and SIMPLE_PINHOLE are, so the images "
                     "must be undistorted first (COLMAP's image_undistorter, or undistort=True for "
                     f"{', '.join(DISTORTED_MODELS)})")
  w, h = int(camera.width), int(camera.height)
  if resize_longest is not None:
    image_scale = resize_longest / max(w, h)
  if image_scale is not None:
    if not 0 < image_scale <= 1:
      raise ValueError(f"the image scale must be in (0, 1], got {image_scale} for a {w} x {h} camera: the resize only shrinks")
    proj = proj * image_scale
    w, h = max(1, round(w * image_scale)), max(1, round(h * image_scale))
  return proj, (w, h)


def quat_to_rotmat(q: np.ndarray) -> np.ndarray:
  """(n, 4) quaternions w x y z (normalised here) -> (n, 3, 3), float64."""
  q = np.asarray(q, np.float64).reshape(-1, 4)
  w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
  return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                   2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                   2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def fit_normalization(config: NormalizationConfig, centres: np.ndarray) -> Normalization:
  """``config.get_transform`` of the camera centres (n, 3), on the host in float64: the translation is minus their mean,
  the scaling one over the median distance to the ``normalize_knn - 1``-th nearest other centre (the lower median, as
  ``torch.median`` takes it)."""
  centres = np.asarray(centres, np.float64).reshape(-1, 3)
  if config.scaling_method == "none":
    scale = 1.0
  elif config.scaling_method == "median_knn":
    k, n = int(config.normalize_knn), centres.shape[0]
    if not 1 <= k <= n:
      raise ValueError(f"median_knn with normalize_knn={k} needs at least that many cameras, got {n}")
    dist = np.sqrt(((centres[:, None, :] - centres[None, :, :]) ** 2).sum(-1))
    kth = np.sort(dist, axis=1)[:, k - 1]                     # column 0 is the centre itself
    scale = float(np.sort(kth)[(n - 1) // 2])
    if not scale > 0:
      raise ValueError(f"median_knn with normalize_knn={k}: the median distance is {scale}")
  else:
    raise ValueError(f"Unknown scaling method: {config.scaling_method}, options are: none, median_knn")
  mean = centres.mean(axis=0) if config.centering else np.zeros(3)
  return Normalization(config=config, translation=torch.from_numpy(-mean).to(torch.float32), scaling=1.0 / scale)


def _normalized_poses(normalization: Normalization, R: np.ndarray, centres: np.ndarray) -> torch.Tensor:
  """camera_t_world (n, 4, 4) float32 of cameras with rotation R (world -> camera) at ``normalization``(centres)."""
  moved = normalization.scaling * (centres + normalization.translation.to(torch.float64).numpy())
  T = np.tile(np.eye(4), (R.shape[0], 1, 1))
  T[:, :3, :3] = R
  T[:, :3, 3] = -np.einsum("nij,nj->ni", R, moved)
  return torch.from_numpy(T).to(torch.float32)


class COLMAPDataset(Dataset):
  def __init__(self, base_path: Union[str, Path], model_dir: str = "sparse/0", image_dir: str = "images",
               image_scale: Optional[float] = None, resize_longest: Optional[int] = None, test_every: int = 8,
               depth_range: Tuple[float, float] = (0.1, 100.0), normalize: NormalizationConfig = NormalizationConfig(),
               device=None, resident: bool = False, undistort: bool = False):
    if image_scale is not None and resize_longest is not None:
      raise ValueError("Specify either resize_longest or image_scale (not both)")
    self.base_path, self.image_dir = str(base_path), image_dir
    self.image_scale, self.resize_longest = image_scale, resize_longest
    self.camera_depth_range = [float(f) for f in depth_range]
    if device is None:
      device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
    self.device, self.resident = torch.device(device), bool(resident)
    self._images = None
    self._camera_table = None

    cameras, images, self._points = colmap_io.read_model(Path(base_path) / model_dir)
    if not images:
      raise ValueError(f"{Path(base_path) / model_dir}: the model has no images")
    id_to_camera_idx, projections, self.source_sizes = {}, [], []
    self.undistortions: List[Optional[Undistortion]] = []                       # per camera; None: a pinhole as it is
    for i, (camera_id, camera) in enumerate(cameras.items()):                   # ascending camera id
      lens = LensCamera.from_colmap(camera) if undistort and camera.model in DISTORTED_MODELS else None
      self.undistortions.append(Undistortion(lens) if lens is not None else None)
      proj, size = colmap_projection(camera, image_scale, resize_longest, self.undistortions[-1])
      projections.append((proj, size))
      self.source_sizes.append((int(camera.width), int(camera.height)))
      id_to_camera_idx[camera_id] = i
    self.projections = Projections(
        intrinsics=torch.tensor(np.stack([p for p, _ in projections]), dtype=torch.float32),
        image_size=torch.tensor([s for _, s in projections], dtype=torch.int32),
        depth_range=torch.tensor([self.camera_depth_range] * len(projections), dtype=torch.float32))
    for image in images:
      if image.camera_id not in id_to_camera_idx:
        raise ValueError(f"image {image.image_id} ({image.name}) refers to camera {image.camera_id}, which the model lacks")

    R = quat_to_rotmat(np.stack([image.qvec for image in images]))               # camera_t_world = [R | t]
    centres = -np.einsum("nji,nj->ni", R, np.stack([image.tvec for image in images]))
    self.normalize = fit_normalization(normalize, centres)
    self.camera_t_world = _normalized_poses(self.normalize, R, centres)
    self.image_names = [image.name for image in images]
    self.image_ids = [image.image_id for image in images]
    self.camera_idx = [id_to_camera_idx[image.camera_id] for image in images]
    self.num_cameras = len(images)
    self.train_idx, self.val_idx = split_every(self.num_cameras, test_every)      # evenly distributed validation images

  def __repr__(self) -> str:
    args = []
    if self.image_scale is not None:
      args += [f"image_scale={self.image_scale}"]
    if self.resize_longest is not None:
      args += [f"resize_longest={self.resize_longest}"]
    args += [f"near={self.camera_depth_range[0]:.3f}", f"far={self.camera_depth_range[1]:.3f}"]
    args += [f"normalization={self.normalize}"]
    args += [f"num_train={len(self.train_idx)}", f"num_val={len(self.val_idx)}"]
    return f"COLMAPDataset({self.base_path} {', '.join(args)})"

  @property
  def to_original(self) -> Normalization:
    return self.normalize.inverse

  @property
  def num_images(self) -> int:
    return len(self.image_names)

  # ---- images ----
  def _decode(self, i: int) -> torch.Tensor:
    from PIL import Image
    file = Path(self.base_path) / self.image_dir / self.image_names[i]
    if not file.is_file():
      raise FileNotFoundError(f"load_images: file {file} does not exist")
    with Image.open(file) as im:
      pixels = np.asarray(im.convert("RGB"))
    want = self.source_sizes[self.camera_idx[i]]
    if (pixels.shape[1], pixels.shape[0]) != want:
      raise ValueError(f"{file} is {pixels.shape[1]} x {pixels.shape[0]}, its camera is {want[0]} x {want[1]}")
    return torch.from_numpy(pixels.copy())

  def _load(self) -> List[torch.Tensor]:
    """Every image, decoded by a pool of threads, undistorted where its camera asks for it and resized, one batch of
    one camera's images at a time: no more than
    STAGING_BYTES of full-resolution pixels (or one image) are held at once."""
    out: List[Optional[torch.Tensor]] = [None] * self.num_images
    on_device = self.device.type == "cuda"
    with ThreadPool(processes=decode_threads()) as pool:
      for cam in range(len(self.source_sizes)):
        rows = [i for i in range(self.num_images) if self.camera_idx[i] == cam]
        (ws, hs), (wd, hd) = self.source_sizes[cam], (int(v) for v in self.projections.image_size[cam])
        per_batch = max(1, STAGING_BYTES // (3 * ws * hs))
        for k in range(0, len(rows), per_batch):
          batch = rows[k:k + per_batch]
          stack = torch.stack(pool.map(self._decode, batch))
          if on_device:
            stack = stack.to(self.device)
          if self.undistortions[cam] is not None:                                 # at full resolution, before the resize
            stack = self.undistortions[cam](stack)
          if (wd, hd) != (ws, hs):
            stack = resize_area(stack, (hd, wd))
          if on_device and not self.resident:
            stack = stack.cpu()
          for i, image in zip(batch, stack):
            out[i] = image
    return out

  def load_images(self) -> List[ImageView]:
    """Loads the images on first use (an expensive operation) and returns one ``ImageView`` per image, in table order:
    uint8 (H, W, 3), in host memory, or on the dataset's device with ``resident=True``."""
    if self._images is None:
      self._images = [ImageView(name, i, image) for i, (name, image) in enumerate(zip(self.image_names, self._load()))]
    return self._images

  def loader(self, idx: torch.Tensor, shuffle: bool = False) -> List[ImageView]:
    images = self.load_images()
    rows = torch.as_tensor(idx).reshape(-1).cpu()
    if shuffle:
      rows = rows[torch.randperm(rows.shape[0])]
    return [images[int(i)] for i in rows.tolist()]

  def train(self, shuffle: bool = False) -> List[ImageView]:
    return self.loader(self.train_idx, shuffle=shuffle)

  def val(self) -> List[ImageView]:
    return self.loader(self.val_idx)

  # ---- geometry ----
  @property
  def camera_table(self) -> MultiCameraTable:
    if self._camera_table is None:
      labels = torch.zeros((self.num_images,), dtype=torch.int32)
      labels[self.train_idx] |= Label.Training.value
      labels[self.val_idx] |= Label.Validation.value
      self._camera_table = MultiCameraTable(camera_t_world=self.camera_t_world, projection=self.projections,
                                            camera_idx=torch.tensor(self.camera_idx, dtype=torch.long), labels=labels,
                                            image_names=self.image_names)
    return self._camera_table

  def pointcloud(self) -> Optional[PointCloud]:
    if len(self._points) == 0:
      return None
    xyz = torch.tensor(self._points.xyz, dtype=torch.float32)
    rgb = torch.tensor(self._points.rgb, dtype=torch.float32) / 255.0
    return PointCloud(self.normalize.transform_points(xyz), rgb)


def export_colmap(path: Union[str, Path], camera_table: CameraTable, images: Sequence, cloud: Optional[PointCloud] = None,
                  ext: str = ".bin", normalization: Optional[Normalization] = None) -> None:
  """Writes a COLMAP directory: ``sparse/0`` with one PINHOLE camera per row of the projection table (ids from 1), one
  image per row of ``camera_table`` (ids from 1, quaternions w x y z with w >= 0), the cloud's points with empty tracks,
  and ``images/<name>`` as PNG (a ``/`` in a name becomes ``_``, and a name that does not end in ``.png`` gains it).  ``images`` holds one uint8 (H, W, 3) tensor or
  ``ImageView`` per row.  With ``normalization`` -- the one that was applied -- poses and points are taken back through
  its inverse, into the original coordinates."""
  from PIL import Image
  path = Path(path)
  images = [im.image if isinstance(im, ImageView) else im for im in images]
  if len(images) != camera_table.num_images:
    raise ValueError(f"{len(images)} images for a camera table of {camera_table.num_images}")
  if isinstance(camera_table, MultiCameraTable):            # the stored rows: no device needed
    q_xyzw, t = camera_table._camera_t_world.q.detach(), camera_table._camera_t_world.t.detach()
    camera_idx = camera_table._camera_idx
  else:
    cameras = camera_table.cameras
    r, t = split_rt(cameras.camera_t_world.detach())
    q_xyzw, camera_idx = rotmat_to_unitquat(r), cameras.camera_idx
  q_xyzw, t = q_xyzw.cpu().to(torch.float64).numpy(), t.cpu().to(torch.float64).numpy()
  q = q_xyzw[:, [3, 0, 1, 2]] / np.linalg.norm(q_xyzw, axis=1, keepdims=True)
  q = np.where(q[:, :1] < 0, -q, q)
  back = normalization.inverse if normalization is not None else None
  if back is not None:                                      # move the centres, keep the rotations
    R = quat_to_rotmat(q)
    centres = -np.einsum("nji,nj->ni", R, t)
    centres = back.scaling * (centres + back.translation.to(torch.float64).cpu().numpy())
    t = -np.einsum("nij,nj->ni", R, centres)

  projections = camera_table.projections
  intrinsics = projections.intrinsics.detach().cpu().to(torch.float64).numpy()
  sizes = projections.image_size.cpu().tolist()
  cameras = {k + 1: colmap_io.Camera("PINHOLE", int(sizes[k][0]), int(sizes[k][1]), intrinsics[k]) for k in range(len(sizes))}
  names = [name.replace("/", "_") for name in camera_table.image_names]
  names = [name if name.lower().endswith(".png") else name + ".png" for name in names]      # the files are PNG
  if len(set(names)) != len(names):
    raise ValueError("two images would be written to one file name")
  records = [colmap_io.Image(k + 1, q[k], t[k], int(camera_idx[k]) + 1, names[k]) for k in range(len(names))]
  points = None
  if cloud is not None:
    xyz = cloud.points.detach().cpu()
    xyz = back.transform_points(xyz) if back is not None else xyz
    rgb = (cloud.colors.detach().cpu().clamp(0, 1) * 255.0).round().to(torch.uint8)
    points = colmap_io.Points.of(xyz.to(torch.float64).numpy(), rgb.numpy())
  colmap_io.write_model(path / "sparse" / "0", cameras, records, points, ext=ext)
  os.makedirs(path / "images", exist_ok=True)
  for name, image in zip(names, images):
    if image.dtype is not torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
      raise ValueError(f"image {name} must be a uint8 (H, W, 3) tensor, got {image.dtype} {tuple(image.shape)}")
    Image.fromarray(image.cpu().numpy()).save(path / "images" / name, format="PNG")
