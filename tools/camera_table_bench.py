"""Times ``table(idx)`` of a camera rig, forward + backward, on the native pose kernels (splat_trainer_amd.camera_table)
against the reference's chain restated in torch on the device (``F.normalize`` -> quaternion to matrix -> ``join_rt`` for
each table, a 4 x 4 matmul, and autograd's backward through all of it), in the same process on the same GPU.

    python tools/camera_table_bench.py [--json out.json]

Rig form (2 cameras, 64 frames), B = 1 and B = 8 images, both tables trainable.  Two figures per form and size:

wall_us     host clock around one forward + backward that ends in a device synchronise: what a training step pays, host
            work and launches included.  The two forms are alternated call by call after a warm-up; median and
            [min, max] over the repetitions.
device_us   device events around CALLS forward + backward calls enqueued back to back, divided by CALLS.  The work is
            launch-bound, so this is the rate at which the host can feed the queue, not kernel time.

The loop is tools/timing.py's: 50 warm-up calls per form, then REPS repetitions of one call on the host clock, then 7
repetitions of CALLS calls on a fresh event pair per window, without a second warm-up; fixed order, lower median.

The kernels' own times are a rocprofv3 --kernel-trace run's business; the trace of this tool under it lists
pose_forward_kernel and pose_backward_kernel.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import splat_trainer_amd as sta  # noqa: E402
from timing import HostClock, repetitions  # noqa: E402

CALLS = 200
REPS = 300


def torch_rotmat(q):
  x, y, z, w = q.unbind(-1)
  tx, ty, tz = 2 * x, 2 * y, 2 * z
  twx, twy, twz = tx * w, ty * w, tz * w
  txx, txy, txz = tx * x, ty * x, tz * x
  tyy, tyz, tzz = ty * y, tz * y, tz * z
  return torch.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx,
                      txz - twy, tyz + twx, 1 - (txx + tyy)], dim=-1).reshape(q.shape[:-1] + (3, 3))


def torch_pose(q, t, idx):
  """PoseTable.forward of the reference (pose_table.py:68-80) with its bounds assertion (a host wait) left out."""
  return sta.camera_table.join_rt(torch_rotmat(F.normalize(q[idx], dim=-1)), t[idx])


def stats(times):
  times = sorted(times)
  return dict(median=round(times[len(times) // 2], 2), range=[round(times[0], 2), round(times[-1], 2)])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--json", default=None)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  g = torch.Generator().manual_seed(0)
  table = sta.RigPoseTable(rig_t_world=torch.eye(4).repeat(64, 1, 1), camera_t_rig=torch.eye(4).repeat(2, 1, 1)).cuda()
  for p in table.parameters():
    p.data.add_(0.3 * torch.randn(p.shape, generator=g).cuda())
    p.requires_grad_(True)
  params = list(table.parameters())
  rows = []
  for B in (1, 8):
    image_idx = torch.randint(0, 128, (B,), generator=g).cuda()
    frame_idx, camera_idx = image_idx // 2, image_idx % 2
    G = torch.randn(B, 4, 4, generator=g).cuda()

    def native():
      return torch.autograd.grad(table(frame_idx, camera_idx), params, G)

    def reference():
      T = torch_pose(table.camera_t_rig.q, table.camera_t_rig.t, camera_idx) @ torch_pose(table.rig_t_world.q, table.rig_t_world.t, frame_idx)
      return torch.autograd.grad(T, params, G)

    for a, b in zip(native(), reference()):
      assert torch.allclose(a, b, rtol=1e-3, atol=1e-4), "the two forms disagree"
    forms = (("native", native), ("torch", reference))
    wall = repetitions(forms, REPS, warmup=50, warmup_form="per_form", clock=HostClock())
    device = repetitions(forms, 7, warmup=0, calls=CALLS, fresh_events=True)
    r = dict(case=f"rig forward+backward B={B}")
    for name, _ in forms:
      r[f"{name}_wall_us"] = stats([t * 1e3 for t in wall[name]])
      r[f"{name}_device_us"] = stats([t * 1e3 for t in device[name]])
    r["wall_speedup"] = round(r["torch_wall_us"]["median"] / r["native_wall_us"]["median"], 2)
    r["native_no_slower"] = r["native_wall_us"]["median"] <= r["torch_wall_us"]["median"]
    rows.append(r)
  sta.check_indices()
  for r in rows:
    print(json.dumps(r))
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
