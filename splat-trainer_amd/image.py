"""Area resize of uint8 images: what the reference's loader asks ``cv2.resize(..., interpolation=cv2.INTER_AREA)`` for,
as the exact area mean rounded half up, in integers (the contract is in include/gsplat_hip.h under
``gsr_image_resize_area_u8``, the arithmetic in csrc/gsr_image.h).

``resize_area(images, size)`` takes a (B, H, W, C) or (H, W, C) uint8 tensor with C in {1, 3}.  A device tensor goes
through the native kernel (csrc/image.hip) and waits for nothing; a CPU tensor goes through the same arithmetic compiled
for the host (``hm_image_resize_area_u8`` of libgsr_hostmath.so), so the two give the same bytes.  Only downscaling: a
larger size raises.  A missing library is an error on either path.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Tuple

import torch

from . import _lib

HOST_LIB_PATH = os.path.join(_lib.PKG_DIR, "libgsr_hostmath.so")
HOST_HEADER_PATH = os.path.join(_lib.PKG_DIR, "csrc", "hostmath_shim.h")
MAX_SIDE = 32768
# what the package itself calls of the host library: the area resize, the undistortion (undistort.py) and the depth
# fusion (fusion.py) and the TSDF meshing (mesh.py)
HOST_FUNCTIONS = ("hm_image_resize_area_u8", "hm_undistort_map", "hm_undistort_points", "hm_image_remap_u8",
                  "hm_fuse_check", "hm_fuse_mask", "hm_fuse_emit", "hm_voxel_downsample", "hm_tsdf_integrate",
                  "hm_mesh_vertex_mask", "hm_mesh_vertex_emit", "hm_mesh_face_mask", "hm_mesh_face_emit")
_host_lib = None
_lock = threading.Lock()


def _host():
  """The host library with ``HOST_FUNCTIONS`` bound from its header's declarations (once)."""
  global _host_lib
  with _lock:
    if _host_lib is None:
      if not os.path.exists(HOST_LIB_PATH):
        raise _lib.GsplatHipError(f"{HOST_LIB_PATH} not found: build it with `python splat-trainer_amd/build.py`")
      with open(HOST_HEADER_PATH) as f:
        functions = _lib.parse_header(f.read(), prefix="hm_", filename="hostmath_shim.h")[2]
      lib = C.CDLL(HOST_LIB_PATH)
      for name in HOST_FUNCTIONS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.make_prototypes({name: functions[name]}, {})[name]
      _host_lib = lib
  return _host_lib


def resize_area(images: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
  """``images`` (B, Hs, Ws, C) or (Hs, Ws, C) uint8 -> the same with ``size = (Hd, Wd)``, on the same device."""
  if not isinstance(images, torch.Tensor) or images.dtype is not torch.uint8 or images.dim() not in (3, 4):
    raise ValueError("images must be a uint8 tensor of shape (B, H, W, C) or (H, W, C)")
  src = (images if images.dim() == 4 else images.unsqueeze(0)).contiguous()
  B, Hs, Ws, channels = src.shape
  Hd, Wd = int(size[0]), int(size[1])
  if channels not in (1, 3):
    raise ValueError(f"images must have 1 or 3 channels, got {channels}")
  if Hs > MAX_SIDE or Ws > MAX_SIDE:
    raise ValueError(f"images of more than {MAX_SIDE} pixels a side are not supported, got {Ws} x {Hs}")
  if not (0 <= Hd <= Hs and 0 <= Wd <= Ws) or (Hs > 0 and Ws > 0 and (Hd == 0 or Wd == 0)):
    raise ValueError(f"size {(Hd, Wd)} must be non-empty and no larger than the images' {(Hs, Ws)}: only downscaling")
  dst = torch.empty((B, Hd, Wd, channels), dtype=torch.uint8, device=src.device)
  if dst.numel() > 0:
    args = (src.data_ptr(), B, Hs, Ws, channels, dst.data_ptr(), Hd, Wd)
    if src.is_cuda:
      with _lib.on_device(src.device) as stream:
        _lib.call("gsr_image_resize_area_u8", *args, stream)
    else:
      _lib.call("hm_image_resize_area_u8", *args, lib=_host())
  return dst if images.dim() == 4 else dst[0]
