"""Times the TSDF meshing's two halves on the GPU, each beside a torch form written here.

    python tools/mesh_bench.py [--json out.json] [--grid N] [--size WxH]

The scene is the unit sphere seen by 16 cameras at distance 3 (the six axes, the eight cube diagonals and two more), with
analytic z-depth maps of 1920 x 1080 and an image per view, and a volume of 256^3 nodes over [-1.28, 1.28]^3.

integrate    ``TsdfVolume.integrate`` of the 16 views in one launch, handed ``HostCamera`` records (no host read).  The
             torch form does the contract's arithmetic in float64 tensors over all nodes, source after source: transform,
             project, floor, a ``gather`` for the depth and three for the colour, ``where`` for the tests, and adds into
             the six int32 planes.  ``differing`` counts the state integers that differ between the two (the torch form
             is free to contract).  ``kernel_ms`` is the raw ``gsr_tsdf_integrate`` call on a table and host arrays
             built in advance, between two device events: the launch apart from the wrapper's host work.  ``gb_per_s``
             is the paper estimate of the traffic -- 48 B of state per node, and nothing for the depth taps -- over
             ``kernel_ms``.
extract      ``TsdfVolume.extract`` of the integrated volume: mask, offsets, the read of V, vertex emit, mask, offsets,
             the read of F, face emit.  The torch form finds the active cells with eight shifted views and ``nonzero``
             (one read), computes the vertices of those cells in float64, and finds the kept edges per axis with
             ``nonzero`` (three reads); its faces come axis by axis, not in ascending edge order, so only the counts are
             compared.  ``kernels_ms`` is the native form's four kernels and two offset scans alone, on buffers sized
             in advance, between two device events: the extraction apart from its two host reads and allocations.

tools/timing.py's loop: 2 warm-up calls per form, REPS repetitions of one window per form, 3 calls per window, fixed
order; the host clock (``perf_counter`` around a window that ends in a synchronise) for the rows that compare forms,
device events for ``kernels_ms``; lower median and [min, max].  No speed-up is asserted: the tool prints both times and
their ratio.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import splat_trainer_amd as sta  # noqa: E402
from splat_trainer_amd import _lib, fusion  # noqa: E402
from timing import DeviceEvents, HostClock, comparison_row, lower_median, repetitions, spread  # noqa: E402

W, H, GRID, VIEWS = 1920, 1080, 256, 16
FOCAL_PER_WIDTH = 1100.0 / 1920.0
REPS = 5


def look_at(eye):
  eye = np.asarray(eye, np.float64)
  z = -eye / np.linalg.norm(eye)
  up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
  x = np.cross(up, z)
  x /= np.linalg.norm(x)
  T = np.eye(4)
  T[:3, :3] = np.stack([x, np.cross(z, x), z])
  T[:3, 3] = -T[:3, :3] @ eye
  return torch.from_numpy(T.astype(np.float32))


def views():
  """(depth maps, images, cameras) on the device."""
  eyes = [np.eye(3)[a] * s for a in range(3) for s in (1, -1)]
  eyes += [np.array([a, b, c]) / math.sqrt(3.0) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
  eyes += [np.array([1.0, 1.0, 0.0]) / math.sqrt(2.0), np.array([-1.0, 0.0, 1.0]) / math.sqrt(2.0)]
  focal = FOCAL_PER_WIDTH * W
  j = (torch.arange(W, dtype=torch.float64, device="cuda")[None, :] + 0.5 - W / 2) / focal
  i = (torch.arange(H, dtype=torch.float64, device="cuda")[:, None] + 0.5 - H / 2) / focal
  depths, images, cameras = [], [], []
  for eye in eyes[:VIEWS]:
    T = look_at(3.0 * eye)
    c = T[:3, 3].double()
    a, b, cc = j * j + i * i + 1.0, -2.0 * (j * c[0] + i * c[1] + c[2]), float(c @ c) - 1.0
    disc = b * b - 4 * a * cc
    z = (-b - disc.clamp(min=0).sqrt()) / (2 * a)
    depths.append(torch.where(disc > 0, z, torch.zeros_like(z)).to(torch.float32).contiguous())
    colour = torch.tensor(0.5 + 0.5 * eye, dtype=torch.float32, device="cuda")
    images.append(colour.expand(H, W, 3).contiguous())
    cameras.append(sta.CameraParams(T_camera_world=T.cuda(), projection=torch.tensor([focal, focal, W / 2, H / 2]).cuda(),
                                    image_size=(W, H), near_plane=0.1))
  return depths, images, cameras


def new_volume():
  voxel = 2.56 / (GRID - 1)
  return sta.TsdfVolume((-1.28, -1.28, -1.28), (GRID, GRID, GRID), voxel, "cuda")


def torch_integrate(state, volume, depths, images, cameras):
  """The contract of gsr_tsdf_integrate in float64 tensors over all nodes, source after source; adds into `state`."""
  n, voxel, origin, trunc = GRID, volume.voxel_size, volume.origin, volume.trunc
  idx = torch.arange(n, dtype=torch.float64, device="cuda")
  X = (origin[0] + idx * voxel)[None, None, :].expand(n, n, n).reshape(-1)
  Y = (origin[1] + idx * voxel)[None, :, None].expand(n, n, n).reshape(-1)
  Z = (origin[2] + idx * voxel)[:, None, None].expand(n, n, n).reshape(-1)
  for depth, image, camera in zip(depths, images, cameras):
    r, (fx, fy, cx, cy) = camera.pose, (float(v) for v in camera.intrinsics)
    p = [r[k, 0] * X + r[k, 1] * Y + r[k, 2] * Z + r[k, 3] for k in range(3)]
    ok = p[2] > camera.near
    us, vs = fx * (p[0] / p[2]) + cx, fy * (p[1] / p[2]) + cy
    ok = ok & (us >= 0) & (us < W) & (vs >= 0) & (vs < H)
    at = torch.where(ok, vs.floor() * W + us.floor(), torch.zeros_like(us)).to(torch.int64)
    ds = torch.gather(depth.reshape(-1), 0, at).to(torch.float64)
    diff = ds - p[2]
    taken = ok & (ds > 0) & torch.isfinite(ds) & (diff >= -trunc)
    Q = ((diff / trunc).clamp(-1.0, 1.0) * 32768.0 + 0.5).floor().to(torch.int32)
    coloured = taken & (diff <= trunc)
    state[0] += torch.where(taken, Q, torch.zeros_like(Q))
    state[1] += taken
    state[2] += coloured
    rgb = image.reshape(-1, 3)
    for ch in range(3):
      byte = (torch.gather(rgb[:, ch], 0, at).to(torch.float64).clamp(0.0, 1.0) * 255.0 + 0.5).floor().to(torch.int32)
      state[3 + ch] += torch.where(coloured, byte, torch.zeros_like(byte))
  return state


CORNERS = [(k & 1, (k >> 1) & 1, (k >> 2) & 1) for k in range(8)]


def torch_extract(state, volume, min_weight=1):
  """Surface nets with shifted views, where and nonzero: (vertices, colours, faces; the faces axis by axis)."""
  n, voxel, origin = GRID, volume.voxel_size, volume.origin
  planes = state.reshape(6, n, n, n)

  def corner(plane, k):
    dx, dy, dz = CORNERS[k]
    return planes[plane, dz:n - 1 + dz, dy:n - 1 + dy, dx:n - 1 + dx]
  valid, negs = None, 0
  for k in range(8):
    v = corner(1, k) >= min_weight
    valid = v if valid is None else valid & v
    negs = negs + (corner(0, k) < 0).to(torch.int32)
  active = (valid & (negs != 0) & (negs != 8)).reshape(-1)
  at = active.nonzero().reshape(-1)                                     # a host read: the count sizes the result
  cells = n - 1
  ci = [at % cells, (at // cells) % cells, at // (cells * cells)]
  m = [corner(0, k).reshape(-1)[at].to(torch.float64) / corner(1, k).reshape(-1)[at].to(torch.float64) for k in range(8)]
  acc = [torch.zeros(at.shape[0], dtype=torch.float64, device="cuda") for _ in range(3)]
  count = torch.zeros(at.shape[0], dtype=torch.float64, device="cuda")
  for a in range(3):
    u, v = (a + 1) % 3, (a + 2) % 3
    for ov in range(2):
      for ou in range(2):
        A = (ou << u) | (ov << v)
        B = A | (1 << a)
        cross = (m[A] < 0) != (m[B] < 0)
        t = m[A] / (m[A] - m[B])
        acc[a] = acc[a] + torch.where(cross, t, torch.zeros_like(t))
        acc[u] = acc[u] + cross * float(ou)
        acc[v] = acc[v] + cross * float(ov)
        count = count + cross
  vertices = torch.stack([(origin[k] + (ci[k].to(torch.float64) + acc[k] / count) * voxel).to(torch.float32) for k in range(3)], 1)
  nc = sum(corner(2, k).reshape(-1)[at].to(torch.int64) for k in range(8))
  colours = torch.stack([torch.where(nc > 0, (2 * sum(corner(3 + ch, k).reshape(-1)[at].to(torch.int64) for k in range(8)) + nc)
                                     // (2 * nc).clamp(min=1), torch.full_like(nc, 255)).to(torch.uint8) for ch in range(3)], 1)
  cell_vertex = torch.full((cells, cells, cells), -1, dtype=torch.int32, device="cuda")      # [z, y, x]
  cell_vertex.reshape(-1)[at] = torch.arange(at.shape[0], dtype=torch.int32, device="cuda")
  sums, weights = planes[0], planes[1]
  faces = []
  for axis in range(3):                                                  # tensors are [z, y, x]: axis a is dim 2 - a
    u, v = (axis + 1) % 3, (axis + 2) % 3

    def cut(t, lo, hi):                                                  # nodes 1 .. n - 2 on u and v, lo .. hi on the axis
      index = [slice(None)] * 3
      index[2 - axis], index[2 - u], index[2 - v] = slice(lo, hi), slice(1, n - 1), slice(1, n - 1)
      return t[tuple(index)]
    lower, upper = cut(sums, 0, n - 1), cut(sums, 1, n)
    cross = (cut(weights, 0, n - 1) >= min_weight) & (cut(weights, 1, n) >= min_weight) & ((lower < 0) != (upper < 0))
    quad = []
    for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
      index = [slice(None)] * 3
      index[2 - axis], index[2 - u], index[2 - v] = slice(0, n - 1), slice(1 + du, n - 1 + du), slice(1 + dv, n - 1 + dv)
      quad.append(cell_vertex[tuple(index)])
    keep = cross & (quad[0] >= 0) & (quad[1] >= 0) & (quad[2] >= 0) & (quad[3] >= 0)
    where = keep.reshape(-1).nonzero().reshape(-1)                       # a host read
    q = torch.stack([c.reshape(-1)[where] for c in quad], 1)
    flip = ~(lower.reshape(-1)[where] < 0)
    q = torch.where(flip[:, None], q.flip(1), q)
    faces.append(torch.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3))
  return vertices, colours, torch.cat(faces)


def integrate_kernel(volume, depths, images, on_host):
  """The native integration's one launch alone, on a source table and host arrays built in advance: a function to time."""
  table = (_lib.GsrTsdfSource * VIEWS)(*[_lib.GsrTsdfSource(depth=d.data_ptr(), image=im.data_ptr(), H=H, W=W)
                                         for d, im in zip(depths, images)])
  params = np.ascontiguousarray(np.stack([np.concatenate([c.pose.reshape(12), c.intrinsics]) for c in on_host]))
  tsdf = np.array([on_host[0].near, volume.trunc, 1.0 / volume.trunc], np.float64)
  state, dims, grid = volume.state, volume.dims, volume.grid

  def run():
    _lib.call("gsr_tsdf_integrate", state.data_ptr(), *dims, grid.ctypes.data, table, params.ctypes.data, VIEWS,
              tsdf.ctypes.data, _lib.current_stream_ptr())
  return run


def extract_kernels(volume, V, F):
  """The native extraction's launches alone, on buffers sized in advance: a function to time."""
  state, dims, grid = volume.state, volume.dims, volume.grid
  cells, nodes, block = volume.num_cells, volume.num_nodes, fusion.COMPACT_BLOCK
  active = torch.empty(cells, dtype=torch.uint8, device="cuda")
  keep = torch.empty(3 * nodes, dtype=torch.uint8, device="cuda")
  cell_vertex = torch.empty(cells, dtype=torch.int32, device="cuda")
  offsets_v = torch.empty((cells + block - 1) // block, dtype=torch.int32, device="cuda")
  offsets_f = torch.empty((3 * nodes + block - 1) // block, dtype=torch.int32, device="cuda")
  total = torch.empty(2, dtype=torch.int32, device="cuda")
  ws = _lib.workspace(int(_lib.load().gsr_compact_workspace_bytes(3 * nodes)), "cuda")
  vertices = torch.empty((V, 3), dtype=torch.float32, device="cuda")
  colours = torch.empty((V, 3), dtype=torch.uint8, device="cuda")
  faces = torch.empty((F, 3), dtype=torch.int32, device="cuda")

  def run():
    s = _lib.current_stream_ptr()
    head = (state.data_ptr(), *dims)
    _lib.call("gsr_mesh_vertex_mask", *head, 1, active.data_ptr(), s)
    _lib.call("gsr_compact_offsets", active.data_ptr(), cells, offsets_v.data_ptr(), total.data_ptr(), _lib.ptr(ws), ws.numel(), s)
    _lib.call("gsr_mesh_vertex_emit", *head, grid.ctypes.data, 1, offsets_v.data_ptr(), V, cell_vertex.data_ptr(),
              vertices.data_ptr(), colours.data_ptr(), s)
    _lib.call("gsr_mesh_face_mask", *head, 1, cell_vertex.data_ptr(), keep.data_ptr(), s)
    _lib.call("gsr_compact_offsets", keep.data_ptr(), 3 * nodes, offsets_f.data_ptr(), total[1:].data_ptr(), _lib.ptr(ws), ws.numel(), s)
    _lib.call("gsr_mesh_face_emit", *head, 1, cell_vertex.data_ptr(), offsets_f.data_ptr(), F, faces.data_ptr(), s)
  return run, (vertices, colours, faces)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--json", default=None)
  ap.add_argument("--grid", type=int, default=None, help="nodes a side, for a rehearsal (default 256)")
  ap.add_argument("--size", default=None, help="WxH of the depth maps, for a rehearsal (default 1920x1080)")
  args = ap.parse_args()
  global W, H, GRID
  if args.size:
    W, H = (int(v) for v in args.size.split("x"))
  if args.grid:
    GRID = args.grid
  if not torch.cuda.is_available():
    raise SystemExit("mesh_bench needs a GPU: nothing here is a measurement without one")
  torch.cuda.set_device(0)
  depths, images, cameras = views()
  on_host = fusion.read_cameras(cameras)
  volume, scratch = new_volume(), new_volume()
  nodes = volume.num_nodes

  # ---- integrate: the volume that the timed calls add to is a scratch one; `volume` takes the views once
  volume.integrate(depths, images, on_host)
  reference = torch_integrate(torch.zeros_like(volume.state), volume, depths, images, on_host)
  differing = int((reference != volume.state).sum())
  del reference

  def native_integrate():
    scratch.views = 0
    scratch.integrate(depths, images, on_host)
  forms = (("native", native_integrate), ("torch", lambda: torch_integrate(scratch.state, scratch, depths, images, on_host)))
  ms = repetitions(forms, REPS, warmup=2, warmup_form="per_form", calls=3, clock=HostClock())
  row = comparison_row(f"integrate {VIEWS} views of {W}x{H} into {GRID}^3", ms["native"], ms["torch"])
  raw = integrate_kernel(scratch, depths, images, on_host)
  before = scratch.state.clone()
  raw()
  kernel_agrees = bool((scratch.state - before == volume.state).all())   # the raw call adds what integrate added
  del before
  device_ms = repetitions((("kernel", raw),), REPS, warmup=2, calls=3)["kernel"]
  estimate = 48.0 * nodes
  rows = [dict(row, kernel_ms=round(lower_median(device_ms), 4), kernel_range=[round(t, 4) for t in spread(device_ms)],
               estimate_gb=round(estimate / 1e9, 3), gb_per_s=round(estimate / 1e9 / (lower_median(device_ms) / 1e3), 1),
               touched_nodes=int((volume.state[1] > 0).sum()), differing=differing, kernel_agrees=kernel_agrees)]
  del scratch

  # ---- extract
  mesh = volume.extract()
  V, F = mesh.num_vertices, mesh.num_faces
  t_vertices, t_colours, t_faces = torch_extract(volume.state, volume)
  same_counts = (int(t_vertices.shape[0]), int(t_faces.shape[0])) == (V, F)
  largest = float((t_vertices.double() - mesh.vertices.double()).abs().max()) if same_counts and V else None
  same_colours = bool((t_colours == mesh.colors).all()) if same_counts else None
  del t_vertices, t_colours, t_faces
  forms = (("native", volume.extract), ("torch", lambda: torch_extract(volume.state, volume)))
  ms = repetitions(forms, REPS, warmup=2, warmup_form="per_form", calls=3, clock=HostClock())
  row = comparison_row(f"extract {GRID}^3", ms["native"], ms["torch"])
  run, out = extract_kernels(volume, V, F)
  run()
  torch.cuda.synchronize()
  kernels_agree = bool((out[0] == mesh.vertices).all() and (out[2] == mesh.faces).all())
  kernel_ms = repetitions((("kernels", run),), REPS, warmup=2, calls=3)["kernels"]
  rows.append(dict(row, kernels_ms=round(lower_median(kernel_ms), 4), kernels_range=[round(t, 4) for t in spread(kernel_ms)],
                   vertices=V, faces=F, same_counts=same_counts, max_abs_vertex_difference=largest, same_colours=same_colours,
                   kernels_agree=kernels_agree))
  for r in rows:
    print(json.dumps(r), flush=True)
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
