"""COLMAP sparse models (``cameras``, ``images``, ``points3D`` as ``.bin`` or ``.txt``) read and written with numpy alone:
what the reference gets from ``pycolmap.Reconstruction`` and writes in ``scripts/to_colmap.py``.

``read_model(path)`` returns ``(cameras, images, points)``: ``cameras`` a dict camera id -> ``Camera`` in ascending id,
``images`` a list of ``Image`` in ASCENDING ``image_id`` (pycolmap iterates in whatever order its map has; here the
order is defined, because the train / validation split goes by position), ``points`` a ``Points`` of arrays.  The 2-D
observations of an image and the track of a point are skipped on read and written empty.

Binary layout, little-endian.  cameras.bin: uint64 n, then n x (int32 camera_id, int32 model_id, uint64 width, uint64
height, double params[k(model)]).  images.bin: uint64 n, then n x (uint32 image_id, double q[4] (w x y z), double t[3],
uint32 camera_id, a NUL-terminated name, uint64 m, m x (double x, double y, int64 point3D_id)).  points3D.bin: uint64 n,
then n x (uint64 id, double xyz[3], uint8 rgb[3], double error, uint64 L, L x (int32 image_id, int32 point2D_idx)).
A file is parsed from one ``bytes`` object; a truncated file, a count the file cannot hold, an unknown model id and a
name without its NUL raise ``ValueError`` with the file and the byte offset, and nothing is read past the buffer.
"""
from __future__ import annotations

import os
import struct
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

# model id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
MODEL_IDS = {name: (model_id, count) for model_id, (name, count) in CAMERA_MODELS.items()}


@dataclass
class Camera:
  model: str
  width: int
  height: int
  params: np.ndarray            # float64 [k(model)]


@dataclass
class Image:
  image_id: int
  qvec: np.ndarray              # float64 [4], w x y z: the rotation of camera_t_world
  tvec: np.ndarray              # float64 [3]: its translation
  camera_id: int
  name: str


@dataclass
class Points:
  ids: np.ndarray               # uint64 [P]
  xyz: np.ndarray               # float64 [P, 3]
  rgb: np.ndarray               # uint8 [P, 3]
  error: np.ndarray             # float64 [P]

  def __len__(self) -> int:
    return self.xyz.shape[0]

  @staticmethod
  def of(xyz, rgb, error=None, ids=None) -> "Points":
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = xyz.shape[0]
    return Points(ids=np.arange(1, n + 1, dtype=np.uint64) if ids is None else np.asarray(ids, np.uint64).reshape(n),
                  xyz=xyz, rgb=np.asarray(rgb, np.uint8).reshape(n, 3),
                  error=np.zeros(n, np.float64) if error is None else np.asarray(error, np.float64).reshape(n))


Model = Tuple[Dict[int, Camera], List[Image], Points]


# ---------------------------------------------------------------------------------------------------------------- binary
class _Reader:
  """A cursor over one bytes object; every read is checked against its end."""

  def __init__(self, data: bytes, filename: str):
    self.data, self.filename, self.pos = data, filename, 0

  def fail(self, what: str, pos: Optional[int] = None):
    raise ValueError(f"{self.filename}: {what} at byte {self.pos if pos is None else pos} of {len(self.data)}")

  def need(self, n: int, what: str):
    if n < 0 or self.pos + n > len(self.data):
      self.fail(f"truncated: {what} needs {n} bytes")

  def unpack(self, fmt: str, what: str) -> tuple:
    n = struct.calcsize(fmt)
    self.need(n, what)
    values = struct.unpack_from(fmt, self.data, self.pos)
    self.pos += n
    return values

  def doubles(self, n: int, what: str) -> np.ndarray:
    self.need(8 * n, what)
    values = np.frombuffer(self.data, "<f8", n, self.pos).copy()
    self.pos += 8 * n
    return values

  def count(self, record_bytes: int, what: str) -> int:
    """A uint64 count of records of at least `record_bytes` each: one the rest of the file cannot hold is refused."""
    at = self.pos
    (n,) = self.unpack("<Q", what)
    if n > (len(self.data) - self.pos) // record_bytes:
      self.fail(f"{what} of {n} cannot fit in the {len(self.data) - self.pos} bytes left", at)
    return n

  def skip(self, n: int, what: str):
    self.need(n, what)
    self.pos += n

  def end(self):
    if self.pos != len(self.data):
      self.fail(f"{len(self.data) - self.pos} bytes left over")


def parse_cameras_bin(data: bytes, filename: str = "cameras.bin") -> Dict[int, Camera]:
  r, cameras = _Reader(data, filename), {}
  for _ in range(r.count(24 + 8 * 3, "the camera count")):
    at = r.pos
    camera_id, model_id, width, height = r.unpack("<iiQQ", "a camera record")
    if model_id not in CAMERA_MODELS:
      r.fail(f"unknown camera model id {model_id}", at + 4)
    name, k = CAMERA_MODELS[model_id]
    cameras[camera_id] = Camera(name, width, height, r.doubles(k, f"the {k} parameters of a {name} camera"))
  r.end()
  return dict(sorted(cameras.items()))


def parse_images_bin(data: bytes, filename: str = "images.bin") -> List[Image]:
  r, images = _Reader(data, filename), []
  for _ in range(r.count(4 + 56 + 4 + 1 + 8, "the image count")):
    (image_id,) = r.unpack("<I", "an image id")
    pose = r.doubles(7, "an image's pose")
    (camera_id,) = r.unpack("<I", "an image's camera id")
    nul = data.find(b"\0", r.pos)
    if nul < 0:
      r.fail("an image name without its NUL")
    try:
      name = data[r.pos:nul].decode("utf-8")
    except UnicodeDecodeError:
      r.fail("an image name that is not UTF-8")
    r.pos = nul + 1
    m = r.count(24, "the 2-D point count")
    r.skip(24 * m, "the 2-D points")
    images.append(Image(image_id, pose[:4], pose[4:], camera_id, name))
  r.end()
  return sorted(images, key=lambda image: image.image_id)


def parse_points_bin(data: bytes, filename: str = "points3D.bin") -> Points:
  r = _Reader(data, filename)
  n = r.count(43 + 8, "the point count")
  ids, xyz = np.zeros(n, np.uint64), np.zeros((n, 3), np.float64)
  rgb, error = np.zeros((n, 3), np.uint8), np.zeros(n, np.float64)
  for k in range(n):
    ids[k], xyz[k, 0], xyz[k, 1], xyz[k, 2], rgb[k, 0], rgb[k, 1], rgb[k, 2], error[k] = r.unpack("<Q3d3Bd", "a point record")
    r.skip(8 * r.count(8, "the track length"), "a track")
  r.end()
  return Points(ids, xyz, rgb, error)


def cameras_bin(cameras: Dict[int, Camera]) -> bytes:
  out = [struct.pack("<Q", len(cameras))]
  for camera_id, cam in cameras.items():
    model_id, k = MODEL_IDS[cam.model]
    params = np.asarray(cam.params, "<f8").reshape(-1)
    if params.size != k:
      raise ValueError(f"camera {camera_id}: {cam.model} takes {k} parameters, got {params.size}")
    out += [struct.pack("<iiQQ", camera_id, model_id, cam.width, cam.height), params.tobytes()]
  return b"".join(out)


def images_bin(images: Sequence[Image]) -> bytes:
  out = [struct.pack("<Q", len(images))]
  for im in images:
    name = im.name.encode("utf-8")
    if b"\0" in name:
      raise ValueError(f"image {im.image_id}: a name cannot hold a NUL")
    out += [struct.pack("<I", im.image_id), np.asarray(im.qvec, "<f8").reshape(4).tobytes(),
            np.asarray(im.tvec, "<f8").reshape(3).tobytes(), struct.pack("<I", im.camera_id), name, b"\0",
            struct.pack("<Q", 0)]
  return b"".join(out)


def points_bin(points: Points) -> bytes:
  record = np.dtype([("id", "<u8"), ("xyz", "<f8", 3), ("rgb", "u1", 3), ("error", "<f8"), ("track", "<u8")])
  assert record.itemsize == 51
  rows = np.zeros(len(points), record)
  rows["id"], rows["xyz"], rows["rgb"], rows["error"] = points.ids, points.xyz, points.rgb, points.error
  return struct.pack("<Q", len(points)) + rows.tobytes()


# ------------------------------------------------------------------------------------------------------------------ text
def _fail_line(filename: str, number: int, line: str, why: str):
  raise ValueError(f"{filename}:{number}: {why}: {line.strip()!r}")


def _lines(text: str):
  """(line number, line) of every line that is no comment."""
  return [(k + 1, line.rstrip("\r")) for k, line in enumerate(text.split("\n")) if not line.lstrip().startswith("#")]


def parse_cameras_txt(text: str, filename: str = "cameras.txt") -> Dict[int, Camera]:
  cameras = {}
  for number, line in _lines(text):
    fields = line.split()
    if not fields:
      continue
    try:
      if fields[1] not in MODEL_IDS:
        raise ValueError(f"unknown camera model {fields[1]}")
      params = np.array([float(v) for v in fields[4:]], np.float64)
      if params.size != MODEL_IDS[fields[1]][1]:
        raise ValueError(f"{fields[1]} takes {MODEL_IDS[fields[1]][1]} parameters")
      cameras[int(fields[0])] = Camera(fields[1], int(fields[2]), int(fields[3]), params)
    except (ValueError, IndexError) as e:
      _fail_line(filename, number, line, str(e))
  return dict(sorted(cameras.items()))


def parse_images_txt(text: str, filename: str = "images.txt") -> List[Image]:
  images, lines, k = [], _lines(text), 0
  while k < len(lines):
    number, line = lines[k]
    k += 1
    if not line.strip():
      continue
    fields = line.split(None, 9)                 # the name is the rest of the line: it may hold spaces
    try:
      if len(fields) != 10:
        raise ValueError("an image line has 10 fields")
      pose = np.array([float(v) for v in fields[1:8]], np.float64)
      images.append(Image(int(fields[0]), pose[:4], pose[4:], int(fields[8]), fields[9].strip()))
    except ValueError as e:
      _fail_line(filename, number, line, str(e))
    k += 1                                       # the line of 2-D points, which may be empty
  return sorted(images, key=lambda image: image.image_id)


def parse_points_txt(text: str, filename: str = "points3D.txt") -> Points:
  ids, xyz, rgb, error = [], [], [], []
  for number, line in _lines(text):
    fields = line.split()
    if not fields:
      continue
    try:
      if len(fields) < 8 or (len(fields) - 8) % 2:
        raise ValueError("a point line has 8 fields and a track of pairs")
      ids.append(int(fields[0]))
      xyz.append([float(v) for v in fields[1:4]])
      rgb.append([int(v) for v in fields[4:7]])
      error.append(float(fields[7]))
    except ValueError as e:
      _fail_line(filename, number, line, str(e))
  return Points.of(np.array(xyz, np.float64).reshape(-1, 3), np.array(rgb, np.uint8).reshape(-1, 3), error, ids)


def _numbers(values) -> str:
  return " ".join(repr(float(v)) for v in values)


def cameras_txt(cameras: Dict[int, Camera]) -> str:
  head = f"# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n# Number of cameras: {len(cameras)}\n"
  return head + "".join(f"{camera_id} {cam.model} {cam.width} {cam.height} {_numbers(cam.params)}\n"
                        for camera_id, cam in cameras.items())


def images_txt(images: Sequence[Image]) -> str:
  head = ("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
          f"#   POINTS2D[] as (X, Y, POINT3D_ID)\n# Number of images: {len(images)}\n")
  for im in images:
    if "\n" in im.name or im.name != im.name.strip() or not im.name:
      raise ValueError(f"image {im.image_id}: the text format cannot hold the name {im.name!r}")
  return head + "".join(f"{im.image_id} {_numbers(im.qvec)} {_numbers(im.tvec)} {im.camera_id} {im.name}\n\n" for im in images)


def points_txt(points: Points) -> str:
  head = ("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n"
          f"# Number of points: {len(points)}\n")
  return head + "".join(f"{int(i)} {_numbers(p)} {int(c[0])} {int(c[1])} {int(c[2])} {float(e)!r}\n"
                        for i, p, c, e in zip(points.ids, points.xyz, points.rgb, points.error))


# ----------------------------------------------------------------------------------------------------------------- files
_PARSERS = {".bin": (parse_cameras_bin, parse_images_bin, parse_points_bin),
            ".txt": (parse_cameras_txt, parse_images_txt, parse_points_txt)}
_WRITERS = {".bin": (cameras_bin, images_bin, points_bin), ".txt": (cameras_txt, images_txt, points_txt)}
_FILES = ("cameras", "images", "points3D")


def read_model(path: Union[str, Path], ext: Optional[str] = None) -> Model:
  """The model in directory ``path``: its ``.bin`` files when ``cameras.bin`` is there, otherwise its ``.txt`` files;
  ``ext`` forces one.  A model without a points file has no points."""
  path = Path(path)
  if ext is None:
    ext = ".bin" if (path / "cameras.bin").exists() else ".txt"
  if ext not in _PARSERS:
    raise ValueError(f"ext must be '.bin' or '.txt', got {ext!r}")
  parsed = []
  for stem, parse in zip(_FILES, _PARSERS[ext]):
    file = path / (stem + ext)
    if stem == "points3D" and not file.exists():
      parsed.append(Points.of(np.zeros((0, 3)), np.zeros((0, 3), np.uint8)))
      continue
    if not file.exists():
      raise FileNotFoundError(f"{file}: no COLMAP model here")
    data = file.read_bytes()
    parsed.append(parse(data if ext == ".bin" else data.decode("utf-8"), str(file)))
  return tuple(parsed)


def write_model(path: Union[str, Path], cameras: Dict[int, Camera], images: Sequence[Image], points: Optional[Points] = None,
                ext: str = ".bin") -> None:
  """Writes ``cameras``, ``images`` and ``points3D`` with extension ``ext`` into directory ``path`` (made if missing), in
  the order given, with empty 2-D point lists and empty tracks."""
  if ext not in _WRITERS:
    raise ValueError(f"ext must be '.bin' or '.txt', got {ext!r}")
  path = Path(path)
  os.makedirs(path, exist_ok=True)
  points = Points.of(np.zeros((0, 3)), np.zeros((0, 3), np.uint8)) if points is None else points
  for stem, write, value in zip(_FILES, _WRITERS[ext], (cameras, images, points)):
    data = write(value)
    (path / (stem + ext)).write_bytes(data if ext == ".bin" else data.encode("utf-8"))
