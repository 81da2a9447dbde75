"""A small COLMAP directory for the dataset tests, host and GPU alike: two PINHOLE cameras (64 x 48 and 50 x 40), nine
PNG images of random bytes under non-consecutive ids written out of order, and 200 points."""
import numpy as np
from PIL import Image

from splat_trainer_amd import colmap_io as cio

SIZES = {3: (64, 48), 8: (50, 40)}                       # camera id -> (width, height)
IMAGE_IDS = [21, 4, 9, 30, 2, 17, 11, 5, 26]               # as written; the dataset's order is ascending
CAMERA_OF = {21: 3, 4: 8, 9: 3, 30: 3, 2: 8, 17: 3, 11: 8, 5: 3, 26: 8}


def write(path, seed=0, bad_camera=None):
  """Writes the directory and returns (cameras, images by ascending id, points, pixels by image id)."""
  rng = np.random.default_rng(seed)
  cameras = {cid: cio.Camera("PINHOLE", w, h, np.array([0.9 * w + cid, 0.95 * w, w / 2 - 0.25, h / 2 + 0.5]))
             for cid, (w, h) in SIZES.items()}
  if bad_camera is not None:
    cameras[3] = bad_camera
  images, pixels = [], {}
  (path / "images" / "sub").mkdir(parents=True, exist_ok=True)
  for image_id in IMAGE_IDS:
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    name = f"sub/im {image_id:03d}.png" if image_id % 2 else f"im_{image_id:03d}.png"
    images.append(cio.Image(image_id, q, rng.uniform(-2, 2, size=3), CAMERA_OF[image_id], name))
    w, h = SIZES[CAMERA_OF[image_id]]
    pixels[image_id] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    Image.fromarray(pixels[image_id]).save(path / "images" / name)
  points = cio.Points.of(rng.normal(size=(200, 3)) * 2, rng.integers(0, 256, size=(200, 3)), rng.uniform(0, 1, 200))
  cio.write_model(path / "sparse" / "0", cameras, images, points)
  return cameras, sorted(images, key=lambda im: im.image_id), points, pixels


def scaled_size(w, h, image_scale=None, resize_longest=None):
  """The reference's formula (dataset/colmap/dataset.py: colmap_projection): the scale and the rounded size."""
  s = resize_longest / max(w, h) if resize_longest is not None else image_scale
  return s, (round(w * s), round(h * s))
