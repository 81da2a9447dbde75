"""COLMAP model files (splat_trainer_amd.colmap_io): write -> read round trips in both formats, the defined image order,
the skipped 2-D point lists and tracks, and every truncation of the binary files."""
import struct

import numpy as np
import pytest

from splat_trainer_amd import colmap_io as cio


def _model(seed=0):
  rng = np.random.default_rng(seed)
  cameras = {7: cio.Camera("SIMPLE_PINHOLE", 640, 480, rng.normal(500, 30, 3)),
             2: cio.Camera("PINHOLE", 1920, 1080, rng.normal(900, 30, 4)),
             11: cio.Camera("OPENCV", 4032, 3024, rng.normal(0, 1, 8))}
  ids = [40, 3, 17, 1000, 5, 2 ** 31 + 9, 12]                              # non-consecutive, out of order
  names = ["a.png", "dir/b.jpg", "with space.png", "d.png", "e e e.jpeg", "f.png", "g.png"]
  images = []
  for k, (image_id, name) in enumerate(zip(ids, names)):
    q = rng.normal(size=4)
    images.append(cio.Image(image_id, q / np.linalg.norm(q), rng.normal(size=3) * 10, [7, 2, 11][k % 3], name))
  points = cio.Points.of(rng.normal(size=(50, 3)) * 3, rng.integers(0, 256, size=(50, 3)), rng.uniform(0, 2, 50),
                         rng.permutation(500)[:50] + 1)
  return cameras, images, points


def _assert_same(got, want, exact=True):
  cameras, images, points = got
  w_cameras, w_images, w_points = want
  assert list(cameras) == sorted(w_cameras)
  for camera_id, cam in cameras.items():
    w = w_cameras[camera_id]
    assert (cam.model, cam.width, cam.height) == (w.model, w.width, w.height)
    assert cam.params.dtype == np.float64 and np.array_equal(cam.params, w.params)
  by_id = sorted(w_images, key=lambda im: im.image_id)
  assert [im.image_id for im in images] == [im.image_id for im in by_id]        # ascending image_id, whatever was written
  for im, w in zip(images, by_id):
    assert (im.camera_id, im.name) == (w.camera_id, w.name)
    assert np.array_equal(im.qvec, w.qvec) and np.array_equal(im.tvec, w.tvec)    # repr() round-trips a double: exact in .txt too
  assert np.array_equal(points.ids, w_points.ids) and np.array_equal(points.rgb, w_points.rgb)
  assert points.xyz.dtype == np.float64 and points.rgb.dtype == np.uint8
  assert np.array_equal(points.xyz, w_points.xyz) and np.array_equal(points.error, w_points.error)


@pytest.mark.parametrize("ext", [".bin", ".txt"])
def test_round_trip(tmp_path, ext):
  model = _model()
  cio.write_model(tmp_path, *model, ext=ext)
  assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{s}{ext}" for s in ("cameras", "images", "points3D"))
  _assert_same(cio.read_model(tmp_path), model)
  _assert_same(cio.read_model(tmp_path, ext), model)


def test_bin_read_equals_txt_read_and_bin_is_preferred(tmp_path):
  model, other = _model(0), _model(1)
  cio.write_model(tmp_path, *model, ext=".bin")
  cio.write_model(tmp_path, *other, ext=".txt")
  _assert_same(cio.read_model(tmp_path), model)                                  # .bin when present
  _assert_same(cio.read_model(tmp_path, ".txt"), other)
  cio.write_model(tmp_path / "t", *model, ext=".txt")
  _assert_same(cio.read_model(tmp_path / "t"), cio.read_model(tmp_path, ".bin"))


def test_text_comments_and_empty_second_lines():
  text = ("# comment\n5 0.5 0.5 0.5 0.5 1 2 3 1 second image.png\n\n"
          "# another\n2 1 0 0 0 0 0 0 1 first.png\n1.5 2.5 -1 3.5 4.5 17\n\n\n")
  images = cio.parse_images_txt(text)
  assert [(im.image_id, im.name) for im in images] == [(2, "first.png"), (5, "second image.png")]
  assert images[1].tvec.tolist() == [1.0, 2.0, 3.0]
  points = cio.parse_points_txt("# c\n9 1 2 3 10 20 30 0.25 4 0 5 1\n3 0 0 0 1 2 3 0\n")
  assert points.ids.tolist() == [9, 3] and points.rgb[0].tolist() == [10, 20, 30] and points.error.tolist() == [0.25, 0.0]
  with pytest.raises(ValueError, match=r"cameras\.txt:2: unknown camera model"):
    cio.parse_cameras_txt("# c\n1 PINHOLEX 4 4 1 1 1 1\n")
  with pytest.raises(ValueError, match=r"cameras\.txt:1: PINHOLE takes 4"):
    cio.parse_cameras_txt("1 PINHOLE 4 4 1 1 1\n")


def _images_with_observations(images, rng):
  """images.bin whose records carry 2-D point lists, put together here field by field."""
  out = [struct.pack("<Q", len(images))]
  for im in images:
    m = int(rng.integers(1, 6))
    out += [struct.pack("<I", im.image_id), struct.pack("<7d", *im.qvec, *im.tvec), struct.pack("<I", im.camera_id),
            im.name.encode() + b"\0", struct.pack("<Q", m)]
    out += [struct.pack("<ddq", rng.normal(), rng.normal(), int(rng.integers(-1, 100))) for _ in range(m)]
  return b"".join(out)


def test_observations_and_tracks_are_skipped():
  cameras, images, points = _model()
  rng = np.random.default_rng(2)
  got = cio.parse_images_bin(_images_with_observations(images, rng))
  want = cio.parse_images_bin(cio.images_bin(images))
  assert [(a.image_id, a.name, a.camera_id) for a in got] == [(b.image_id, b.name, b.camera_id) for b in want]
  assert all(np.array_equal(a.qvec, b.qvec) and np.array_equal(a.tvec, b.tvec) for a, b in zip(got, want))
  out = [struct.pack("<Q", len(points))]
  for k in range(len(points)):
    L = int(rng.integers(0, 5))
    out += [struct.pack("<Q3d3BdQ", int(points.ids[k]), *points.xyz[k], *points.rgb[k].tolist(), points.error[k], L)]
    out += [struct.pack("<ii", int(rng.integers(0, 100)), int(rng.integers(0, 1000))) for _ in range(L)]
  tracked = cio.parse_points_bin(b"".join(out))
  assert np.array_equal(tracked.ids, points.ids) and np.array_equal(tracked.xyz, points.xyz)
  assert np.array_equal(tracked.rgb, points.rgb) and np.array_equal(tracked.error, points.error)


def test_every_truncation_raises_value_error():
  cameras, images, points = _model()
  rng = np.random.default_rng(4)
  files = [(cio.parse_cameras_bin, cio.cameras_bin(cameras)), (cio.parse_images_bin, cio.images_bin(images[:3])),
           (cio.parse_images_bin, _images_with_observations(images[:2], rng)),
           (cio.parse_points_bin, cio.points_bin(cio.Points.of(points.xyz[:3], points.rgb[:3])))]
  for parse, data in files:
    parse(data)
    for cut in range(len(data)):
      with pytest.raises(ValueError, match=r"\.bin: .* at byte \d+ of \d+"):
        parse(data[:cut])
    with pytest.raises(ValueError, match="left over"):
      parse(data + b"\0")


def test_bad_counts_models_and_names():
  cameras, images, _ = _model()
  data = cio.cameras_bin(cameras)
  for count in (2 ** 64 - 1, 2 ** 63, 10 ** 6, len(cameras) + 1):                 # -1 as written by a signed writer, absurd, one too many
    with pytest.raises(ValueError, match=r"cameras\.bin: "):
      cio.parse_cameras_bin(struct.pack("<Q", count) + data[8:])
  bad_model = bytearray(data)
  bad_model[12:16] = struct.pack("<i", 99)
  with pytest.raises(ValueError, match=r"unknown camera model id 99 at byte 12"):
    cio.parse_cameras_bin(bytes(bad_model))
  one = cio.images_bin(images[:1])
  no_nul = one[:8 + 64] + one[8 + 64:].replace(b"\0", b"x")
  with pytest.raises(ValueError, match=r"images\.bin: an image name without its NUL at byte 72"):
    cio.parse_images_bin(no_nul)
  with pytest.raises(ValueError, match="PINHOLE takes 4 parameters"):
    cio.cameras_bin({1: cio.Camera("PINHOLE", 4, 4, np.zeros(3))})


def test_missing_points_file_is_an_empty_cloud(tmp_path):
  cameras, images, points = _model()
  cio.write_model(tmp_path, cameras, images, points)
  (tmp_path / "points3D.bin").unlink()
  assert len(cio.read_model(tmp_path)[2]) == 0
  with pytest.raises(FileNotFoundError):
    cio.read_model(tmp_path / "nowhere")
  with pytest.raises(ValueError, match="ext must be"):
    cio.read_model(tmp_path, ".json")
