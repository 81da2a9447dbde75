"""fp64 statement of the evaluation pass's iterative colour fit (splat_trainer_amd.evaluation.fit_colors_batch,
csrc/gsr_eval.h), written from its contract, in numpy:

  design row of a pixel (r, g, b):  a = [r^2, rg, rb, g^2, gb, b^2, r, g, b, 1]
  iteration k, channel c:           w_c = argmin sum_p m_c(p) (a(p) . w - ref_c(p))^2,
                                    m_c = unclipped(x0_c) & unclipped(x_c) & unclipped(ref_c),  unclipped(z) = eps <= z <= 1 - eps
  next iterate:                     x <- clip(a W, 0, 1)

``form="lstsq"`` solves each system as the reference does (a least-squares solve on the masked rows: full rank only);
``form="pinv"`` is the project's rule for every rank: S = A^T A and t = A^T b scaled by s_i = 1 / sqrt(S_ii) (1 where
S_ii <= 0), symmetric eigendecomposition, eigenvalues <= 1e-9 lambda_max dropped (lambda_max <= 0: w = 0), w the
pseudo-inverse solution, unscaled.  Both report how close any mask decision came to its threshold and the smallest
kept-to-largest eigenvalue ratio, so that a test can show its inputs are far from either edge.
"""
import numpy as np

RANK_CUT = 1e-9
EXPONENTS = ((2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))


def monomial_tables():
  """mono[i][j] = index of the monomial a_i a_j among the 35 of degree <= 4, numbered by first appearance over (i, j)
  row-major (the numbering of the 35 sums in csrc/gsr_eval.h), and the exponent triple of each."""
  seen, mono = [], [[0] * 10 for _ in range(10)]
  for i in range(10):
    for j in range(10):
      e = tuple(a + b for a, b in zip(EXPONENTS[i], EXPONENTS[j]))
      if e not in seen:
        seen.append(e)
      mono[i][j] = seen.index(e)
  assert len(seen) == 35
  return mono, seen


def design(x):
  """(P, 3) -> (P, 10), in the dtype of x."""
  r, g, b = x[:, 0], x[:, 1], x[:, 2]
  return np.stack([r * r, r * g, r * b, g * g, g * b, b * b, r, g, b, np.ones_like(r)], axis=1)


def system_from_sums(sums):
  """45 sums (35 monomials, then a . ref) -> S (10, 10), t (10)."""
  mono, _ = monomial_tables()
  sums = np.asarray(sums, np.float64)
  S = np.array([[sums[mono[i][j]] for j in range(10)] for i in range(10)])
  return S, sums[35:45].copy()


def moments(x0, x, ref, eps=0.5 / 255):
  """The 3 x 45 sums of iterate x (fp64 arithmetic on the given values), as csrc/gsr_eval.h numbers them."""
  _, exps = monomial_tables()
  x0, x, ref = (np.asarray(v, np.float64).reshape(-1, 3) for v in (x0, x, ref))
  A = design(x)
  out = np.zeros((3, 45))
  for c in range(3):
    m = unclipped(x0[:, c], eps) & unclipped(x[:, c], eps) & unclipped(ref[:, c], eps)
    xm = x[m]
    for k, (p, q, s) in enumerate(exps):
      out[c, k] = np.sum(xm[:, 0] ** p * xm[:, 1] ** q * xm[:, 2] ** s)
    out[c, 35:] = A[m].T @ ref[m, c]
  return out


def unclipped(z, eps):
  return (z >= eps) & (z <= 1 - eps)


def solve_pinv(S, t, cut=RANK_CUT):
  """-> (w, kept-to-largest eigenvalue ratio or inf when nothing is kept, largest dropped-to-largest ratio or 0)."""
  d = np.diag(S)
  s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0)
  lam, V = np.linalg.eigh(S * s[:, None] * s[None, :])
  lmax = lam.max()
  if not lmax > 0:
    return np.zeros(10), np.inf, 0.0
  keep = lam > cut * lmax
  y = V[:, keep] @ ((V[:, keep].T @ (t * s)) / lam[keep])
  dropped = np.abs(lam[~keep]).max() / lmax if (~keep).any() else 0.0
  return s * y, lam[keep].min() / lmax, dropped


def fit(img, ref, num_iters=5, eps=0.5 / 255, form="pinv"):
  """-> (result of img's shape, fp64; info) with info = dict(threshold_distance, eig_ratio, iterates)."""
  shape = np.shape(img)
  x0 = np.asarray(img, np.float64).reshape(-1, 3)
  r = np.asarray(ref, np.float64).reshape(-1, 3)
  x = x0.copy()
  edge = lambda z: min(np.abs(z - eps).min(), np.abs(z - (1 - eps)).min())
  distance, ratio, iterates = min(edge(x0), edge(r)), np.inf, []
  for _ in range(num_iters):
    iterates.append(x.copy())
    distance = min(distance, edge(x))
    A = design(x)
    W = np.zeros((10, 3))
    for c in range(3):
      m = unclipped(x0[:, c], eps) & unclipped(x[:, c], eps) & unclipped(r[:, c], eps)
      Am, bm = A * m[:, None], r[:, c] * m
      w, kept, _ = solve_pinv(Am.T @ Am, Am.T @ bm)
      ratio = min(ratio, kept)
      W[:, c] = np.linalg.lstsq(Am, bm, rcond=-1)[0] if form == "lstsq" else w
    x = np.clip(A @ W, 0.0, 1.0)
  return x.reshape(shape), dict(threshold_distance=float(distance), eig_ratio=float(ratio), iterates=iterates)


# ---- the golden fixtures (tests/golden/color_fit_ref.npz, written by tests/golden/make_golden_color_fit.py) ------------
def decode_images(img_u16, ref_u8):
  """The fixtures' fp32 images from their stored integers: k / 65535 and k / 255, IEEE float32 divisions."""
  return (img_u16.astype(np.float32) / np.float32(65535.0)), (ref_u8.astype(np.float32) / np.float32(255.0))


def load_golden(path):
  """-> list of dict(img, ref (fp32), out64 (the reference on the widened inputs), out32 (the reference in fp32),
  threshold_distance, eig_ratio)."""
  z = np.load(path)
  out = []
  for i in range(int(z["count"])):
    img, ref = decode_images(z[f"f{i}_img_u16"], z[f"f{i}_ref_u8"])
    out64 = z[f"f{i}_out64"]
    # the fp32 result is stored as its distance in float32 steps from the rounded fp64 result (small integers)
    out32 = (out64.astype(np.float32).view(np.int32) + z[f"f{i}_out32_steps"]).view(np.float32)
    out.append(dict(img=img, ref=ref, out64=out64, out32=out32, threshold_distance=float(z[f"f{i}_threshold_distance"]),
                    eig_ratio=float(z[f"f{i}_eig_ratio"])))
  return out


def golden_tolerance(fixtures):
  """4 x the largest deviation of the reference's own fp32 run from its fp64 run over the fixtures: the fp32 form is
  what the reference's users get, and the factor covers a different order of operations in applying the warp."""
  return 4.0 * max(float(np.abs(f["out32"].astype(np.float64) - f["out64"]).max()) for f in fixtures)
