"""Oracles for splat_trainer_amd.camera_table's pose kernels (csrc/camera_table.hip, maths in csrc/gsr_camera_table.h).

* ``forward_fp64``: the reference's chain restated in fp64 torch -- ``F.normalize(q[idx])`` (pose_table.py:75, eps
  1e-12), roma's ``unitquat_to_rotmat`` for XYZW quaternions (pose_table.py:79), ``join_rt`` (util/transforms.py:16-27)
  and, for a rig, ``camera_t_rig @ rig_t_world`` (pose_table.py:44-48); its gradient by torch autograd;
* ``backward_fp64``: the analytic formulas the kernels implement, in fp64, which must agree with autograd to fp64
  rounding;
* the inputs the checks use (``tables``, ``upstream``, ``measurement_inputs``), the error measures and the wrappers of the host shim.

Error measures.  Inputs: ``|q|`` in [0.1, 10], ``|t_i|`` <= 100, ``|G_ij|`` <= 1.  A forward entry is compared on
``1 + tmax``, ``tmax`` the largest ``|t_i|`` over the tables (a rig's translation is ``Rc tw + tc``).  A gradient entry of a
row is linear in G, in the other table's translation, in ``1 / |q|`` of its own row (``d_q`` only, through the
normalisation) and a sum over the ``n`` images that selected it, so it is compared on ``(1 + tmax) max(n, 1)`` and, for
``d_q``, ``max(1, 1 / |q|)`` on top.

MEASURED_* (one figure per form, single table and rig) are the largest errors of the host shim (g++, no contraction,
every fma written out: a function of the inputs alone) against fp64 on ``measurement_inputs()``: 4096-row tables, 8192
images.  The device may round differently where its compiler is free to (the fmaf order is written out, but sqrtf and
the division are the device's own), so the bound the device is held to is MARGIN times that, as
tests/filter3d_oracle.py does.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-12
T_MAX = 100.0
MARGIN = 4.0
# (profiles/r21_camera_table.txt) forward: of 1 + tmax; backward: of (1 + tmax) max(n, 1) [max(1, 1 / |q|)].  A single
# table's translation is copied and its rotation entries are O(1), hence the two orders of magnitude between the forms.
MEASURED_FORWARD = {"single": 4.0e-9, "rig": 4.6e-7}
MEASURED_BACKWARD = {"single": 1.1e-8, "rig": 8.6e-7}
BOUND_FORWARD = {form: MARGIN * e for form, e in MEASURED_FORWARD.items()}
BOUND_BACKWARD = {form: MARGIN * e for form, e in MEASURED_BACKWARD.items()}


# ---- fp64 forward and autograd ---------------------------------------------------------------------------------------

def rotmat(q):
  """roma.unitquat_to_rotmat for (..., 4) XYZW unit quaternions, in the dtype of ``q``."""
  x, y, z, w = q.unbind(-1)
  tx, ty, tz = 2 * x, 2 * y, 2 * z
  twx, twy, twz = tx * w, ty * w, tz * w
  txx, txy, txz = tx * x, ty * x, tz * x
  tyy, tyz, tzz = ty * y, tz * y, tz * z
  return torch.stack([1 - (tyy + tzz), txy - twz, txz + twy,
                      txy + twz, 1 - (txx + tzz), tyz - twx,
                      txz - twy, tyz + twx, 1 - (txx + tyy)], dim=-1).reshape(q.shape[:-1] + (3, 3))


def pose(q, t):
  """PoseTable.forward on gathered rows: (B, 4), (B, 3) -> (B, 4, 4)."""
  T = torch.zeros(q.shape[:-1] + (4, 4), dtype=q.dtype)
  T[..., :3, :3] = rotmat(F.normalize(q, dim=-1, eps=EPS))
  T[..., :3, 3] = t
  T[..., 3, 3] = 1
  return T


def _t64(a, grad=False):
  return None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float64)).requires_grad_(grad)


def _idx(a):
  return None if a is None else torch.as_tensor(np.asarray(a, dtype=np.int64))


def forward_torch(ql, tl, il, qr=None, tr=None, ir=None):
  T = pose(ql[il], tl[il])
  return T if qr is None else T @ pose(qr[ir], tr[ir])


def forward_fp64(ql, tl, il, qr=None, tr=None, ir=None):
  with torch.no_grad():
    return forward_torch(_t64(ql), _t64(tl), _idx(il), _t64(qr), _t64(tr), _idx(ir)).numpy()


def autograd_fp64(ql, tl, il, qr, tr, ir, G):
  """(d_ql, d_tl, d_qr, d_tr) of sum(G * T) by autograd on the fp64 forward; the right pair is None without a rig."""
  leaves = [_t64(a, grad=True) for a in ((ql, tl) if qr is None else (ql, tl, qr, tr))]
  T = forward_torch(leaves[0], leaves[1], _idx(il), *((None, None, None) if qr is None else (leaves[2], leaves[3], _idx(ir))))
  grads = torch.autograd.grad((T * _t64(G)).sum(), leaves, allow_unused=True)
  grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
  out = [g.numpy() for g in grads]
  return tuple(out) if qr is not None else (out[0], out[1], None, None)


# ---- the analytic backward, fp64 -------------------------------------------------------------------------------------

def _row_backward(q, D):
  """d_q (A, 4) from the summed dL/dR (A, 3, 3) of each row, through R(q^) and the normalisation."""
  n = np.linalg.norm(q, axis=1)
  d = np.maximum(n, EPS)
  qh = q / d[:, None]
  x, y, z, w = qh.T
  S01, S02, S12 = D[:, 0, 1] + D[:, 1, 0], D[:, 0, 2] + D[:, 2, 0], D[:, 1, 2] + D[:, 2, 1]
  A21, A02, A10 = D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]
  dh = 2 * np.stack([y * S01 + z * S02 - 2 * x * (D[:, 1, 1] + D[:, 2, 2]) + w * A21,
                     x * S01 + z * S12 - 2 * y * (D[:, 0, 0] + D[:, 2, 2]) + w * A02,
                     x * S02 + y * S12 - 2 * z * (D[:, 0, 0] + D[:, 1, 1]) + w * A10,
                     x * A21 + y * A02 + z * A10], axis=1)
  projected = (dh - qh * (qh * dh).sum(axis=1, keepdims=True)) / d[:, None]
  return np.where((n >= EPS)[:, None], projected, dh / EPS)


def _rot64(q):
  return rotmat(F.normalize(_t64(q), dim=-1, eps=EPS)).numpy()


def backward_fp64(ql, tl, il, qr, tr, ir, G):
  """The formulas of csrc/gsr_camera_table.h in fp64: dRc = G_R Rw^T + g tw^T, dtc = g, dRw = Rc^T G_R, dtw = Rc^T g,
  summed per row, then through the rotation and (I - q^ q^T) / |q| (1 / eps below the clamp)."""
  ql, tl, G = (np.asarray(a, dtype=np.float64) for a in (ql, tl, G))
  il = np.asarray(il, dtype=np.int64)
  GR, g = G[:, :3, :3], G[:, :3, 3]
  DL, dtl = np.zeros((ql.shape[0], 3, 3)), np.zeros((ql.shape[0], 3))
  if qr is None:
    np.add.at(DL, il, GR)
    np.add.at(dtl, il, g)
    return _row_backward(ql, DL), dtl, None, None
  qr, tr = np.asarray(qr, dtype=np.float64), np.asarray(tr, dtype=np.float64)
  ir = np.asarray(ir, dtype=np.int64)
  Rc, Rw, tw = _rot64(ql)[il], _rot64(qr)[ir], tr[ir]
  np.add.at(DL, il, GR @ Rw.transpose(0, 2, 1) + g[:, :, None] * tw[:, None, :])
  np.add.at(dtl, il, g)
  DR, dtr = np.zeros((qr.shape[0], 3, 3)), np.zeros((qr.shape[0], 3))
  np.add.at(DR, ir, Rc.transpose(0, 2, 1) @ GR)
  np.add.at(dtr, ir, (Rc.transpose(0, 2, 1) @ g[:, :, None])[:, :, 0])
  return _row_backward(ql, DL), dtl, _row_backward(qr, DR), dtr


# ---- inputs ------------------------------------------------------------------------------------------------------------

def tables(A, seed, unit=False):
  """(q (A, 4), t (A, 3)) float32: random directions with |q| log-uniform in [0.1, 10] (1 when ``unit``), |t_i| <= 100."""
  rng = np.random.default_rng(seed)
  q = rng.standard_normal((A, 4))
  q /= np.linalg.norm(q, axis=1, keepdims=True)
  if not unit:
    q *= 10.0 ** rng.uniform(-1.0, 1.0, (A, 1))
  t = rng.uniform(-T_MAX, T_MAX, (A, 3))
  return q.astype(np.float32), t.astype(np.float32)


def upstream(B, seed):
  """G = dL/dT (B, 4, 4) float32 in [-1, 1]; row 3 is filled too (it must be ignored)."""
  return np.random.default_rng(seed).uniform(-1.0, 1.0, (B, 4, 4)).astype(np.float32)


def measurement_inputs():
  """The inputs MEASURED_* were taken on: (name, ql, tl, il, qr, tr, ir, G), single then rig, half the rows unit."""
  A, B = 4096, 8192
  rng = np.random.default_rng(7)
  out = []
  for name, rig in (("single", False), ("rig", True)):
    ql, tl = tables(A, 11 if rig else 10)
    ql[: A // 2] = tables(A // 2, 12, unit=True)[0]
    il = rng.integers(0, A, B)
    qr = tr = ir = None
    if rig:
      qr, tr = tables(A, 13)
      qr[: A // 2] = tables(A // 2, 14, unit=True)[0]
      ir = rng.integers(0, A, B)
    out.append((name, ql, tl, il, qr, tr, ir, upstream(B, 15)))
  return out


# ---- error measures ----------------------------------------------------------------------------------------------------

def _tmax(tl, tr):
  return max(float(np.abs(tl).max()), float(np.abs(tr).max()) if tr is not None else 0.0)


def forward_error(T, T64, tl, tr=None):
  """The largest |T - T64| over the entries, of 1 + tmax."""
  if T64.size == 0:
    return 0.0
  return float(np.abs(np.asarray(T, dtype=np.float64) - T64).max() / (1.0 + _tmax(tl, tr)))


def backward_error(got, want, ql, tl, il, qr=None, tr=None, ir=None):
  """The largest error over (d_ql, d_tl, d_qr, d_tr), each entry on the scale of the module docstring."""
  worst = 0.0
  span = 1.0 + _tmax(tl, tr)
  for (dq, dt, dq64, dt64), q, idx in (((got[0], got[1], want[0], want[1]), ql, il),
                                        ((got[2], got[3], want[2], want[3]), qr, ir)):
    if q is None or dq is None:
      continue
    n = np.maximum(np.bincount(np.asarray(idx, dtype=np.int64), minlength=q.shape[0]), 1).astype(np.float64)
    inv = np.maximum(1.0, 1.0 / np.maximum(np.linalg.norm(np.asarray(q, dtype=np.float64), axis=1), EPS))
    worst = max(worst, float((np.abs(dq.astype(np.float64) - dq64) / (span * n * inv)[:, None]).max()),
                float((np.abs(dt.astype(np.float64) - dt64) / (span * n)[:, None]).max()))
  return worst


# ---- the host shim -------------------------------------------------------------------------------------------------------

def _c(a, dtype):
  return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def shim_forward(shim, ql, tl, il, qr=None, tr=None, ir=None):
  """(T (B, 4, 4) float32, return code)."""
  il = _c(il, np.int64)
  T = np.empty((il.shape[0], 4, 4), dtype=np.float32)
  rc = shim.hm_pose_forward(_c(ql, np.float32), _c(tl, np.float32), ql.shape[0], il, _c(qr, np.float32),
                            _c(tr, np.float32), 0 if qr is None else qr.shape[0], _c(ir, np.int64), il.shape[0], T)
  return T, rc


def shim_backward(shim, ql, tl, il, qr, tr, ir, G):
  il = _c(il, np.int64)
  d_ql, d_tl = np.full_like(ql, np.nan), np.full_like(tl, np.nan)
  d_qr, d_tr = (None, None) if qr is None else (np.full_like(qr, np.nan), np.full_like(tr, np.nan))
  rc = shim.hm_pose_backward(_c(ql, np.float32), _c(tl, np.float32), ql.shape[0], il, _c(qr, np.float32),
                             _c(tr, np.float32), 0 if qr is None else qr.shape[0], _c(ir, np.int64), il.shape[0],
                             _c(G, np.float32), d_ql, d_tl, d_qr, d_tr)
  return (d_ql, d_tl, d_qr, d_tr), rc


if __name__ == "__main__":            # the measurement behind MEASURED_*: python tests/camera_table_oracle.py
  import os
  import sys
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import importlib
  import hostmath
  shim = hostmath.load(importlib.import_module("splat_trainer_amd.build").build_all())
  for name, ql, tl, il, qr, tr, ir, G in measurement_inputs():
    T, _ = shim_forward(shim, ql, tl, il, qr, tr, ir)
    got, _ = shim_backward(shim, ql, tl, il, qr, tr, ir, G)
    want = backward_fp64(ql, tl, il, qr, tr, ir, G)
    auto = autograd_fp64(ql, tl, il, qr, tr, ir, G)
    print(f"{name:7s} forward {forward_error(T, forward_fp64(ql, tl, il, qr, tr, ir), tl, tr):.3e}  "
          f"backward {backward_error(got, want, ql, tl, il, qr, tr, ir):.3e}  "
          f"analytic vs autograd {backward_error([None if a is None else a for a in want], auto, ql, tl, il, qr, tr, ir):.3e}")
