"""The normal-consistency contract (csrc/gsr_normals.h) restated in torch, without reading the header: splat normals,
depth normals and the depth-normal consistency loss, differentiable through autograd, in whatever dtype the inputs have
(fp64 is the reference; the same formulas in fp32 on the CPU give the error the GPU tests scale their bounds from).  The
input builders of tests/test_gpu_normals.py live here too, with the conditions they keep, so that
tests/test_normals_host.py can assert them without a GPU."""
import torch

from helpers import oracle


# ---- the contract ----------------------------------------------------------------------------------------------------
def thin_axis(log_scaling: torch.Tensor) -> torch.Tensor:
  """Index of the smallest entry of each row, the lowest index on ties (torch.argmin does not promise which)."""
  k = torch.zeros(log_scaling.shape[0], dtype=torch.int64)
  best = log_scaling[:, 0]
  for j in (1, 2):
    better = log_scaling[:, j] < best
    k = torch.where(better, torch.full_like(k, j), k)
    best = torch.where(better, log_scaling[:, j], best)
  return k


def splat_normals(rotation, log_scaling, position, indexes, T_camera_world) -> torch.Tensor:
  """(M, 3): R_cw R[:, k] of the rows ``indexes``, negated where it points away from the camera.  Differentiable in
  ``rotation`` alone: the axis and the flip are constants."""
  R = oracle.quat_to_rotmat_xyzw(rotation[indexes])
  k = thin_axis(log_scaling[indexes].detach())
  col = R[torch.arange(indexes.shape[0]), :, k]
  Rcw, t = T_camera_world[:3, :3].detach(), T_camera_world[:3, 3].detach()
  n = col @ Rcw.t()
  p = position[indexes].detach() @ Rcw.t() + t
  flip = (n.detach() * p).sum(1) > 0
  return torch.where(flip[:, None], -n, n)


def geometry_features(rotation, log_scaling, position, indexes, depth, T_camera_world) -> torch.Tensor:
  n = splat_normals(rotation, log_scaling, position, indexes, T_camera_world)
  return torch.cat([n, depth.reshape(-1, 1), torch.ones_like(depth.reshape(-1, 1))], 1)


def rays(H: int, W: int, projection: torch.Tensor) -> torch.Tensor:
  fx, fy, cx, cy = projection.unbind(0)
  u = (torch.arange(W, dtype=projection.dtype) + 0.5 - cx) / fx
  v = (torch.arange(H, dtype=projection.dtype) + 0.5 - cy) / fy
  return torch.stack([u[None, :].expand(H, W), v[:, None].expand(H, W), torch.ones(H, W, dtype=projection.dtype)], -1)


def depth_normals(depth: torch.Tensor, projection: torch.Tensor):
  """-> (normals (H, W, 3), valid (H, W) bool, |c| (H, W))."""
  H, W = depth.shape
  n = torch.zeros(H, W, 3, dtype=depth.dtype)
  valid = torch.zeros(H, W, dtype=torch.bool)
  length = torch.zeros(H, W, dtype=depth.dtype)
  if H < 3 or W < 3:
    return n, valid, length
  ok = torch.isfinite(depth) & (depth > 0)
  safe = torch.where(ok, depth, torch.ones_like(depth))            # keeps NaN out of the graph; masked below
  P = rays(H, W, projection.detach()) * safe[..., None]
  a = P[1:-1, 2:] - P[1:-1, :-2]
  b = P[2:, 1:-1] - P[:-2, 1:-1]
  c = torch.cross(b, a, dim=-1)
  ln = c.norm(dim=-1)
  inner = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1] & (ln > 0)
  unit = c / torch.where(inner, ln, torch.ones_like(ln))[..., None]
  n = torch.nn.functional.pad(torch.where(inner[..., None], unit, torch.zeros_like(unit)), (0, 0, 1, 1, 1, 1))
  valid[1:-1, 1:-1] = inner
  length[1:-1, 1:-1] = ln.detach()
  return n, valid, length


def expected_depth(G: torch.Tensor, alpha_min: float) -> torch.Tensor:
  D, A = G[..., 3], G[..., 4]
  seen = A >= alpha_min
  return torch.where(seen, D / torch.where(seen, A, torch.ones_like(A)), torch.zeros_like(D))


def normal_loss(G: torch.Tensor, projection: torch.Tensor, alpha_min: float):
  """-> (L, n_d, valid)."""
  H, W = G.shape[:2]
  n_d, valid, _ = depth_normals(expected_depth(G, alpha_min), projection)
  per_pixel = G[..., 4] - (G[..., :3] * n_d).sum(-1)
  L = torch.where(valid, per_pixel, torch.zeros_like(per_pixel)).sum() / (H * W)
  return L, n_d, valid


def touched(valid: torch.Tensor) -> torch.Tensor:
  """Pixels that are valid or a tap of a valid pixel: the only ones the loss gradient may reach."""
  t = valid.clone()
  t[:, 1:] |= valid[:, :-1]
  t[:, :-1] |= valid[:, 1:]
  t[1:, :] |= valid[:-1, :]
  t[:-1, :] |= valid[1:, :]
  return t


# ---- tolerance: the oracle's own fp32 error, never the kernel's --------------------------------------------------------------
def bound(fp32_result: torch.Tensor, fp64_result: torch.Tensor) -> float:
  """4 x the largest error of the oracle's formulas in fp32 on the CPU against fp64 (the factor
  tests/test_gpu_filter3d.py grants for contraction and another order of three-term sums), plus 2^-22 max|oracle|."""
  ref = fp64_result.detach().double()
  own = (fp32_result.detach().double() - ref).abs().max().item() if ref.numel() else 0.0
  scale = ref.abs().max().item() if ref.numel() else 0.0
  return 4.0 * own + 2.0 ** -22 * scale


# ---- input builders ------------------------------------------------------------------------------------------------------
SPLAT_N = (1, 63, 64, 65, 257, 1000)
DEPTH_SIZES = ((3, 3), (5, 1), (2, 7), (17, 5), (64, 3), (65, 33), (130, 67))       # (W, H)
LOSS_SIZES = ((17, 5), (65, 33), (130, 67))
SCALE_GAP, FACING_MIN = 1e-3, 1e-3


def camera_pose(seed: int) -> torch.Tensor:
  """A rigid T_camera_world (4, 4) float32 with a general rotation."""
  gen = torch.Generator().manual_seed(seed)
  q = torch.randn(4, generator=gen, dtype=torch.float64)
  T = torch.eye(4, dtype=torch.float64)
  T[:3, :3] = oracle.quat_to_rotmat_xyzw(q)
  T[:3, 3] = torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64)
  return T.float()


def splat_inputs(N: int, seed: int):
  """rotation (N, 4) not normalised, log_scaling (N, 3), position (N, 3), T (4, 4): float32, with the two smallest scales
  of a row at least SCALE_GAP apart and |n . p| / |p| >= FACING_MIN in fp64 (rows that miss either are redrawn)."""
  gen = torch.Generator().manual_seed(seed)
  T = camera_pose(seed + 1)
  rot = torch.randn(N, 4, generator=gen) * (0.5 + torch.rand(N, 1, generator=gen))
  ls = torch.randn(N, 3, generator=gen)
  pos = torch.randn(N, 3, generator=gen) * 2.0
  for _ in range(64):
    bad = ~splat_conditions(rot, ls, pos, T)
    if not bad.any():
      break
    k = int(bad.sum())
    rot[bad] = torch.randn(k, 4, generator=gen)
    ls[bad] = torch.randn(k, 3, generator=gen)
    pos[bad] = torch.randn(k, 3, generator=gen) * 2.0
  return rot, ls, pos, T


def splat_conditions(rot, ls, pos, T) -> torch.Tensor:
  """Per row: the builder's two conditions, evaluated in fp64."""
  two = ls.double().sort(dim=1).values
  idx = torch.arange(rot.shape[0])
  n = splat_normals(rot.double(), ls.double(), pos.double(), idx, T.double())
  p = pos.double() @ T.double()[:3, :3].t() + T.double()[:3, 3]
  facing = (n * p).sum(1).abs() / p.norm(dim=1)
  return (two[:, 1] - two[:, 0] >= SCALE_GAP) & (facing >= FACING_MIN) & (rot.double().norm(dim=1) > 0.05)


def pinhole(W: int, H: int) -> torch.Tensor:
  """fx fy cx cy float32: a 60 degree lens with the principal point off the centre."""
  f = 0.5 * max(W, H) / 0.57735
  return torch.tensor([f, 1.07 * f, 0.5 * W + 0.3, 0.5 * H - 0.2], dtype=torch.float32)


PLANE_N0 = (0.3, -0.2, -0.9327379053088815)         # unit, facing the camera
PLANE_C = -2.0                                      # n0 . X = c: the plane crosses the axis at z = 2.14


def plane_depth(W: int, H: int, projection: torch.Tensor, dtype=torch.float64):
  """(depth (H, W), n0 (3,)) of the analytic plane n0 . X = c seen through ``projection``: d = c / (n0 . ray)."""
  n0 = torch.tensor(PLANE_N0, dtype=dtype)
  d = PLANE_C / (rays(H, W, projection.to(dtype)) @ n0)
  return d, n0


def random_depth(W: int, H: int, seed: int) -> torch.Tensor:
  gen = torch.Generator().manual_seed(seed)
  return 1.0 + 2.0 * torch.rand(H, W, generator=gen)


PUNCHES = ((2, 2, 0.0), (5, 1, float("nan")), (9, 3, -1.0), (0, 0, 0.0), (16, 4, float("nan")))      # (x, y, value)


def punched(depth: torch.Tensor):
  """``depth`` with the PUNCHES that fit inside it, and the mask of the pixels that must lose their normal: the punched
  pixels and their four neighbours."""
  H, W = depth.shape
  out, lost = depth.clone(), torch.zeros(H, W, dtype=torch.bool)
  for x, y, v in PUNCHES:
    if x < W and y < H:
      out[y, x] = v
      for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        if 0 <= x + dx < W and 0 <= y + dy < H:
          lost[y + dy, x + dx] = True
  return out, lost


ALPHA_MIN = 0.5


def geometry_image(W: int, H: int, seed: int) -> torch.Tensor:
  """A random G (H, W, 5) float32: N^ in [-1, 1]^3, expected depth in [1, 3], A in [0.05, 0.45) for about a quarter of
  the pixels and in (0.55, 1] for the rest, D = depth A."""
  gen = torch.Generator().manual_seed(seed)
  N = 2.0 * torch.rand(H, W, 3, generator=gen) - 1.0
  depth = 1.0 + 2.0 * torch.rand(H, W, generator=gen)
  low = torch.rand(H, W, generator=gen) < 0.25
  r = torch.rand(H, W, generator=gen)
  A = torch.where(low, 0.05 + 0.399 * r, 0.551 + 0.449 * r)
  return torch.cat([N, (depth * A)[..., None], A[..., None]], -1)


def geometry_conditions(G: torch.Tensor) -> bool:
  A = G[..., 4]
  share = (A < ALPHA_MIN).double().mean().item()
  return bool(((A < 0.45) | (A > 0.55)).all()) and 0.15 <= share <= 0.35
