"""The stage contract of K4 tile binning and of the deterministic per-splat reductions (csrc/binning.hip, the tile
maths of csrc/gsr_math.h): an fp64 reference with derived rounding bands, the cases, a comparator that returns the list
of violations, and a bit-exact numpy fp32 model of the reductions.  numpy on the CPU only; no kernel is involved here.

BINNING.  Input: the packed fp32 rows [M, 16] (u v A B | C opacity ...), taken exactly into fp64, W, H and the raster
parameters.  Per splat qmax = min(q_max * 1.00001, 2 ln(op / thr) * 1.0001 + 1e-4) (gsr_splat_extent's constants in
fp64); no tiles when op < thr or det = A C - B B <= 0.  Per tile half (tx, ty, h) -- upper half rows 0-7, lower half rows
8-15 -- the rectangle of its pixel centres relative to the mean, NOT clipped to the image (gsr_tile_half_mask does not
clip either), and on each of its four edges the closed-form minimum of q = Kf df^2 + 2 B df d + Kv d^2 (gsr_edge_min_q)
with S = |Kf| df^2 + 2 |B df d| + |Kv| d^2 at the minimiser.  With u = 2^-24:

  q band per edge   8u S + 8u max(qmax, 1): the fp32 evaluation of the quadratic is off by at most 4u S, one rounding in
                    each of the two offsets (16 tx + .5 is exact) moves it by at most 2u S, the rest is slack; the second
                    term covers logf and the arithmetic of qmax.
  extent band       rho = 2u (|A C| + B^2) / det bounds the relative error of the fp32 det, rel = rho + 8u that of the
                    half-width (which only inherits rho / 2), pad = 8u (|u| + hx64 + 16) the roundings of u -+ hx - .5.
                    A tile column is firmly inside the extent when it is inside for the half-width hx64 (1 - rel) - pad and
                    firmly outside when it is outside for hx64 (1 + rel) + pad + 1.01e-3 (the device adds 1e-3); rows alike.
  firm hit          (mean inside the rectangle, or some edge has q + band <= qmax) and the tile firmly inside the extent
  firm miss         (mean outside and every edge has q - band > qmax) or the tile firmly outside the extent
  undecided         everything else: either answer is accepted; a family may leave at most UNDECIDED_CAP of its
                    firm-hit-or-undecided halves undecided, so the bands cannot hide a defect.

NEED is the brute-force cross-check: the halves that hold an in-image pixel centre with q64 <= min(q_max, 2 ln(op / thr)),
no inflation.  NEED must lie inside firm hit + undecided, and a binning must emit all of it.

REDUCTIONS.  The slots of rank k are [offsets[k], offsets[k] + count[k]).  Read off reduce_vis_kernel, reduce_grad_kernel,
reduce_grad_wide_kernel and gsr_wave_sum_to_lane63:

  count <= 64       acc = fl(acc + x_j) from +0 in slot order.  A gradient column skips slots with vis <= 0 (their
                    `partial` is never read); skipping equals adding +0, which leaves an accumulator that started at +0
                    unchanged.  The visibility column adds every slot.  Slots at or beyond `limit` (visibility only)
                    are absent.
  count > 64        groups of 64 slots counted from the rank's first slot; missing slots, slots with vis <= 0 (gradient
                    columns) and slots at or beyond `limit` enter as +0; each group is summed by the wave tree; the group
                    sums are added from +0 in group order.
  the tree          row_shr:1, 2, 4, 8 (bound_ctrl: a lane without a source adds 0): after them lane 15 of each row of 16
                    holds ((((x15+x14)+(x13+x12)) + ((x11+x10)+(x9+x8))) + (((x7+x6)+(x5+x4)) + ((x3+x2)+(x1+x0)))), every
                    operand of lane 15 having a source at each step (15 - 1, 13 - 2, 11 - 4, 7 - 8 + ... >= 0).
                    row_bcast:15 with row mask 0xa adds lane 15 of row 0 into row 1 and of row 2 into row 3: lane 31 =
                    r1 + r0, lane 63 = r3 + r2.  row_bcast:31 with row mask 0xc adds lane 31 into rows 2 and 3: lane 63 =
                    (r3 + r2) + (r1 + r0).  fp32 addition is commutative, so this is the balanced pairwise tree over the
                    64 lanes: x = x[0::2] + x[1::2] applied six times.
"""
import functools

import numpy as np

U = 2.0 ** -24
PARAMS = dict(alpha_threshold=1.0 / 255.0, clamp_max_alpha=0.99, T_eps=1e-4, q_max=9.0, blur=0.3, antialias=0,
              tile_size=16, margin_px=48.0)
THR = float(np.float32(PARAMS["alpha_threshold"]))          # the parameters travel as fp32
Q_MAX = float(np.float32(PARAMS["q_max"]))
UNDECIDED_CAP = 0.01
CANARY = 0xCDCDCDCD
MAP_TILES = 32                                               # binning.hip: extents up to this use the 64-bit map
SERIAL = 64                                                  # binning.hip: GSR_REDUCE_SERIAL
CHUNK = 256                                                  # reduce_grad_kernel: slots per LDS chunk, ranks per block


def tiles(W, H):
  return (W + 15) // 16, (H + 15) // 16


# ---------------------------------------------------------------------------------------------------- binning reference
class Reference:
  """firm_hit / firm_miss [M, tiles_y, tiles_x, 2] (last axis: upper, lower half), rho [M], valid [M]."""

  def __init__(self, firm_hit, firm_miss, rho, valid):
    self.firm_hit, self.firm_miss, self.rho, self.valid = firm_hit, firm_miss, rho, valid
    self.undecided = ~firm_hit & ~firm_miss

  def stats(self):
    hit, und = int(self.firm_hit.sum()), int(self.undecided.sum())
    return dict(firm_hit=hit, undecided=und, share=und / max(hit + und, 1),
                max_rho=float(self.rho[self.valid].max()) if self.valid.any() else 0.0)


def _edge(Kf, Bc, Kv, df, lo, hi):
  d = np.clip(-Bc * df / Kv, lo, hi)
  q = Kf * df * df + 2.0 * Bc * df * d + Kv * d * d
  S = np.abs(Kf) * df * df + 2.0 * np.abs(Bc * df * d) + np.abs(Kv) * d * d
  return q, S


def _inside(c, h, idx, n):
  lo = np.clip(np.floor((c - h - 0.5) / 16.0), 0, n)
  hi = np.clip(np.floor((c + h - 0.5) / 16.0) + 1.0, 0, n)
  return (idx >= lo) & (idx < hi)


def reference(rows, W, H):
  nx, ny = tiles(W, H)
  g = np.asarray(rows, np.float32)[:, :6].astype(np.float64)
  u, v, A, B, C, op = (g[:, i][:, None, None] for i in range(6))
  with np.errstate(all="ignore"):
    qmax = np.minimum(Q_MAX * 1.00001, 2.0 * np.log(op / THR) * 1.0001 + 1e-4)
    det = A * C - B * B
    valid = (op >= THR) & (det > 0.0)
  A, C, det = np.where(valid, A, 1.0), np.where(valid, C, 1.0), np.where(valid, det, 1.0)
  B, qmax = np.where(valid, B, 0.0), np.where(valid, qmax, 0.0)
  rho = 2.0 * U * (np.abs(A * C) + B * B) / det
  rel = rho + 8.0 * U
  txs, tys = np.arange(nx)[None, None, :], np.arange(ny)[None, :, None]
  inside, outside = valid, ~valid
  for c, K, idx, n in ((u, C, txs, nx), (v, A, tys, ny)):
    h = np.sqrt(qmax * K / det)
    pad = 8.0 * U * (np.abs(c) + h + 16.0)
    h_in = h * (1.0 - rel) - pad
    inside = inside & (h_in >= 0.0) & _inside(c, h_in, idx, n)
    outside = outside | ~_inside(c, h * (1.0 + rel) + pad + 1.01e-3, idx, n)
  rx0 = 16.0 * txs + 0.5 - u
  rx1 = rx0 + 15.0
  band0 = 8.0 * U * np.maximum(qmax, 1.0)
  firm_hit = np.zeros((g.shape[0], ny, nx, 2), bool)
  firm_miss = np.zeros_like(firm_hit)
  for half in (0, 1):
    ry0 = 16.0 * tys + 0.5 - v + 8.0 * half
    ry1 = ry0 + 7.0
    mean_in = (rx0 <= 0.0) & (rx1 >= 0.0) & (ry0 <= 0.0) & (ry1 >= 0.0)
    some_hit, all_miss = np.zeros(mean_in.shape, bool), np.ones(mean_in.shape, bool)
    for q, S in (_edge(A, B, C, rx0, ry0, ry1), _edge(A, B, C, rx1, ry0, ry1),
                 _edge(C, B, A, ry0, rx0, rx1), _edge(C, B, A, ry1, rx0, rx1)):
      band = 8.0 * U * S + band0
      some_hit |= q + band <= qmax
      all_miss &= q - band > qmax
    firm_hit[..., half] = inside & (mean_in | some_hit)
    firm_miss[..., half] = outside | (all_miss & ~mean_in)
  return Reference(firm_hit, firm_miss, rho[:, 0, 0], valid[:, 0, 0])


def need(rows, W, H):
  """[M, tiles_y, tiles_x, 2]: the half holds an in-image pixel centre with q64 <= min(q_max, 2 ln(op / thr))."""
  nx, ny = tiles(W, H)
  g = np.asarray(rows, np.float32)[:, :6].astype(np.float64)
  out = np.zeros((g.shape[0], ny, nx, 2), bool)
  px, py = np.arange(W) + 0.5, np.arange(H) + 0.5
  for m, (u, v, A, B, C, op) in enumerate(g):
    if not op >= THR:
      continue
    dx, dy = (px - u)[None, :], (py - v)[:, None]
    ok = np.zeros((ny * 16, nx * 16), bool)
    ok[:H, :W] = A * dx * dx + 2.0 * B * dx * dy + C * dy * dy <= min(Q_MAX, 2.0 * np.log(op / THR))
    out[m] = ok.reshape(ny, 2, 8, nx, 16).any(axis=(2, 4)).transpose(0, 2, 1)
  return out


# ---------------------------------------------------------------------------------------------------------------- cases
def conic_rows(u, v, s1, s2, theta, op):
  """Packed rows [M, 16] fp32 of splats with standard deviations s1 (along theta) and s2."""
  c, s = np.cos(theta), np.sin(theta)
  rows = np.zeros((len(u), 16), np.float32)
  rows[:, 0], rows[:, 1] = u, v
  rows[:, 2] = c * c / s1 ** 2 + s * s / s2 ** 2
  rows[:, 3] = c * s * (1.0 / s1 ** 2 - 1.0 / s2 ** 2)
  rows[:, 4] = s * s / s1 ** 2 + c * c / s2 ** 2
  rows[:, 5] = op
  return rows


def _log_uniform(rng, lo, hi, n):
  return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _special_opacities(op):
  thr = np.float32(PARAMS["alpha_threshold"])
  special = [thr * np.float32(0.5), np.nextafter(thr, np.float32(0)), thr, thr * np.float32(1.0 + 1e-3),
             np.float32(0.02), np.float32(1.0)]
  op = op.astype(np.float32)
  for i in range(min(len(op), 4 * len(special))):
    op[i] = special[i % len(special)]
  return op


def _scatter(rng, M, W, H, margin, s_lo, s_hi, special=True):
  op = rng.uniform(0.5 * THR, 1.0, M)
  return conic_rows(rng.uniform(-margin, W + margin, M), rng.uniform(-margin, H + margin, M),
                    _log_uniform(rng, s_lo, s_hi, M), _log_uniform(rng, s_lo, s_hi, M), rng.uniform(0, np.pi, M),
                    _special_opacities(op) if special else op)


class Case:
  def __init__(self, name, family, W, H, rows, order):
    self.name, self.family, self.W, self.H = name, family, W, H
    self.rows, self.order = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(order, np.uint32)
    self.M = len(order)
    self.tiles_x, self.tiles_y = tiles(W, H)
    self.num_tiles = self.tiles_x * self.tiles_y

  @functools.cached_property
  def ref(self):
    return reference(self.rows, self.W, self.H)

  @functools.cached_property
  def need(self):
    return need(self.rows, self.W, self.H)


def _place(nx, ny, x0, y0):
  """Axis-aligned splat at full opacity whose extent is exactly nx x ny tiles from tile (x0, y0): the box ends 4 px
  inside its first and last tile (h = 3.000015 sigma at q_max 9), far from any undecided column."""
  hx, hy = 8.0 * nx - 4.0, 8.0 * ny - 4.0
  return (16.0 * x0 + 8.0 * nx + 0.5, 16.0 * y0 + 8.0 * ny + 0.5, hx / 3.0, hy / 3.0)


MAP_EDGE_WIDE = [(32, 1, 4, 10), (8, 4, 1, 1), (4, 8, 12, 2), (16, 2, 20, 14), (33, 1, 3, 20), (11, 3, 25, 3), (3, 11, 36, 9)]
MAP_EDGE_TALL = [(1, 32, 1, 4), (1, 33, 2, 5), (2, 16, 0, 20)]


def _map_edge(name, W, H, placed, seed):
  u, v, sx, sy = (np.array(c) for c in zip(*(_place(*p) for p in placed)))
  rows = conic_rows(u, v, sx, sy, np.zeros(len(u)), np.ones(len(u)))
  return Case(name, "map edge", W, H, rows, np.random.default_rng(seed).permutation(len(u)))


@functools.lru_cache(maxsize=None)
def binning_cases():
  cases = []
  rng = np.random.default_rng(3101)
  cases.append(Case("grid", "grid", 200, 120, _scatter(rng, 300, 200, 120, 50.0, 0.55, 40.0), rng.permutation(300)))

  rng = np.random.default_rng(3102)
  M, W, H = 200, 640, 360
  theta = rng.uniform(0, np.pi, M)
  theta[:8] = [0.0, np.pi / 2, np.pi / 4, 3 * np.pi / 4, np.pi / 6, np.pi / 3, 1e-3, np.pi / 2 - 1e-3]
  rows = conic_rows(rng.uniform(-40, W + 40, M), rng.uniform(-40, H + 40, M), _log_uniform(rng, 5.0, 150.0, M),
                    _log_uniform(rng, 0.55, 8.0, M), theta, rng.uniform(0.05, 1.0, M))
  cases.append(Case("needles", "needles", W, H, rows, rng.permutation(M)))

  # 64 giants fill wave 0 (lanes 0 and 63 among them: the large-extent loop runs 64 times there), a 65th is alone in
  # wave 1, whose other lanes lie behind M
  rng = np.random.default_rng(3103)
  M = 65
  rows = conic_rows(rng.uniform(0, W, M), rng.uniform(0, H, M), _log_uniform(rng, 40.0, 400.0, M),
                    _log_uniform(rng, 40.0, 400.0, M), rng.uniform(0, np.pi, M), rng.uniform(0.3, 1.0, M))
  cases.append(Case("giants", "giants", W, H, rows, rng.permutation(M)))

  cases.append(_map_edge("map edge wide", 640, 360, MAP_EDGE_WIDE, 3104))
  cases.append(_map_edge("map edge tall", 64, 640, MAP_EDGE_TALL, 3105))

  for i, (W, H) in enumerate(((24, 8), (16, 16), (8, 8))):
    rng = np.random.default_rng(3110 + i)
    cases.append(Case(f"tiny {W}x{H}", "tiny", W, H, _scatter(rng, 100, W, H, 10.0, 0.55, 20.0), rng.permutation(100)))

  for M in (1, 63, 64, 65, 257):
    rng = np.random.default_rng(3120 + M)
    cases.append(Case(f"counts M={M}", "counts", 200, 120, _scatter(rng, M, 200, 120, 50.0, 0.55, 40.0, special=M > 1),
                      rng.permutation(M)))
  return tuple(cases)


def binning_case(name):
  return next(c for c in binning_cases() if c.name == name)


def m_dev_values(M):
  return sorted({0, 1, M // 2, M - 1, M})


def family_stats(cases):
  """family -> dict(firm_hit, undecided, share, max_rho) over the family's cases."""
  out = {}
  for c in cases:
    s, t = c.ref.stats(), out.setdefault(c.family, dict(firm_hit=0, undecided=0, max_rho=0.0))
    t["firm_hit"] += s["firm_hit"]
    t["undecided"] += s["undecided"]
    t["max_rho"] = max(t["max_rho"], s["max_rho"])
  for t in out.values():
    t["share"] = t["undecided"] / max(t["firm_hit"] + t["undecided"], 1)
  return out


def shim_masks(shim, params, case):
  """Half masks [M, num_tiles] of the project's tile maths compiled for the host (hostmath_shim: hm_tile_half_masks)."""
  masks = np.zeros((case.M, case.num_tiles), np.uint8)
  shim.hm_tile_half_masks(params, case.M, np.ascontiguousarray(case.rows[:, :6]), case.tiles_x, case.tiles_y, masks)
  return masks


def shim_extents(shim, params, case):
  """(extent [M, 4] = x0 x1 y0 y1, qmax [M]) of gsr_splat_extent compiled for the host (hm_splat_extent)."""
  ext, qmax = np.zeros((case.M, 4), np.int32), np.zeros(case.M, np.float32)
  shim.hm_splat_extent(params, case.M, np.ascontiguousarray(case.rows[:, :6]), case.tiles_x, case.tiles_y, ext, qmax)
  return ext, qmax


# ----------------------------------------------------------------------------------------------------------- comparator
def emit(masks, order, live, capacity=None):
  """What a sequential walk emits for per-splat half masks [M, num_tiles] (0: tile not hit): a dict in the layout of the
  device's outputs -- count, offsets, total, keys, inst, capacity -- with CANARY in the slots it does not write."""
  M = len(order)
  count = np.zeros(M, np.uint32)
  keys, inst = [], []
  for k in range(min(live, M)):
    s = int(order[k])
    idx = np.flatnonzero(masks[s])
    count[k] = len(idx)
    keys.append(idx.astype(np.uint32))
    inst.append(np.uint32(s) | (masks[s][idx].astype(np.uint32) << np.uint32(30)))
  offsets = (np.cumsum(count, dtype=np.uint64) - count).astype(np.uint32)
  total = int(count.sum())
  cap = total if capacity is None else capacity
  k_out, i_out = np.full(max(total, cap) + 8, CANARY, np.uint32), np.full(max(total, cap) + 8, CANARY, np.uint32)
  if total:
    k_out[:total], i_out[:total] = np.concatenate(keys), np.concatenate(inst)
  k_out[cap:], i_out[cap:] = CANARY, CANARY
  return dict(count=count, offsets=offsets, total=total, keys=k_out, inst=i_out, capacity=capacity)


def decode(order, live, out, num_tiles):
  """Half masks [M, num_tiles] by splat id from an emission (slots below the capacity; malformed entries are left out)."""
  masks = np.zeros((len(order), num_tiles), np.uint8)
  cap = len(out["keys"]) if out["capacity"] is None else min(out["capacity"], len(out["keys"]))
  for k in range(min(live, len(order))):
    b = int(out["offsets"][k])
    e = min(b + int(out["count"][k]), cap)
    if e > b:
      key, val = out["keys"][b:e], out["inst"][b:e]
      ok = key < num_tiles
      masks[int(order[k]), key[ok]] = (val[ok] >> np.uint32(30)).astype(np.uint8)
  return masks


def compare(ref, order, live, out, num_tiles, limit=20):
  """The violations of the contract in one emission `out` (see emit), as a list of strings; empty when it conforms."""
  bad = []
  M = len(order)
  count, offsets = out["count"].astype(np.int64), out["offsets"].astype(np.int64)
  keys, inst = out["keys"], out["inst"]
  capacity = len(keys) if out["capacity"] is None else out["capacity"]
  for k in np.flatnonzero(count[live:])[:3]:
    bad.append(f"rank {live + k} lies behind the device count {live} but has count {count[live + k]}")
  scan = np.cumsum(count) - count
  for k in np.flatnonzero(offsets != scan % 2 ** 32)[:3]:
    bad.append(f"offsets[{k}] = {offsets[k]} is not the exclusive scan of count ({scan[k]})")
  if out["total"] != int(count.sum()):
    bad.append(f"total {out['total']} is not the sum of the counts {int(count.sum())}")
  written = min(capacity, int(count.sum()))
  for name, a in (("keys", keys), ("inst2splat", inst)):
    for i in np.flatnonzero(a[written:] != CANARY)[:3]:
      bad.append(f"{name}[{written + i}] was written: capacity {capacity}, total {int(count.sum())}")
  fh = ref.firm_hit.reshape(len(ref.firm_hit), num_tiles, 2)
  fm = ref.firm_miss.reshape(len(ref.firm_miss), num_tiles, 2)
  for k in range(min(live, M)):
    if len(bad) >= limit:
      break
    s, b, n = int(order[k]), int(scan[k]), int(count[k])
    e = min(b + n, capacity)
    if e > len(keys):
      bad.append(f"rank {k}: slots [{b}, {b + n}) exceed the buffers ({len(keys)})")
      continue
    key, val = keys[b:e].astype(np.int64), inst[b:e]
    sid, mask = val & np.uint32(0x3FFFFFFF), (val >> np.uint32(30)).astype(np.uint8)
    if (sid != s).any():
      bad.append(f"rank {k}: slot {b + int(np.flatnonzero(sid != s)[0])} carries splat id {sid[sid != s][0]}, not {s}")
    if (mask == 0).any():
      bad.append(f"rank {k}: slot {b + int(np.flatnonzero(mask == 0)[0])} has an empty half mask")
    if (key >= num_tiles).any():
      bad.append(f"rank {k}: key {key.max()} is outside the {num_tiles} tiles")
      continue
    if (np.diff(key) <= 0).any():
      bad.append(f"rank {k}: keys are not in ascending row-major order at slot {b + int(np.flatnonzero(np.diff(key) <= 0)[0]) + 1}")
    got = np.zeros((num_tiles, 2), bool)
    got[key, 0], got[key, 1] = (mask & 1) != 0, (mask & 2) != 0
    for t, h in np.argwhere(got & fm[s])[:2]:
      bad.append(f"rank {k} (splat {s}): tile {t} half {h} is a firm miss but was emitted")
    if b + n <= capacity:
      for t, h in np.argwhere(fh[s] & ~got)[:2]:
        bad.append(f"rank {k} (splat {s}): tile {t} half {h} is a firm hit but was not emitted")
  return bad[:limit]


# ------------------------------------------------------------------------------------------------------ reduction model
def tree64(x):
  """gsr_wave_sum_to_lane63 over the last axis (64 lanes) in fp32: the balanced pairwise tree (module docstring)."""
  x = np.asarray(x, np.float32)
  for _ in range(6):
    x = x[..., 0::2] + x[..., 1::2]
  return x[..., 0]


def model_sum(x):
  """The device's sum of the slots x [n, columns] of one rank (fp32, masked slots already zero): [columns]."""
  x = np.asarray(x, np.float32)
  n = x.shape[0]
  acc = np.zeros(x.shape[1], np.float32)
  if n > SERIAL:
    groups = -(-n // 64)
    padded = np.zeros((groups * 64, x.shape[1]), np.float32)
    padded[:n] = x
    x = tree64(padded.reshape(groups, 64, -1).transpose(0, 2, 1))
  for row in x:
    acc = acc + row
  return acc


def model_reduce(values, vis, offsets, count, gate, limit=None):
  """Per rank [M, columns]: the modelled sums of values [O, columns]; gate: skip slots with vis <= 0 (gradient columns);
  limit: slots at or beyond it are absent."""
  values = np.asarray(values, np.float32)
  keep = np.ones(len(values), bool)
  if gate:
    keep &= vis > 0
  if limit is not None:
    keep[limit:] = False
  x = np.where(keep[:, None], values, np.float32(0))
  return np.stack([model_sum(x[b:b + n]) for b, n in zip(offsets.astype(np.int64), count.astype(np.int64))])


def fp64_distance(values, vis, offsets, count, gate, modelled):
  """Largest |model - fp64 sum| / ((n - 1) u sum |x_j|) over ranks and columns (0 where the bound is 0 and met)."""
  worst = 0.0
  for k, (b, n) in enumerate(zip(offsets.astype(np.int64), count.astype(np.int64))):
    x = values[b:b + n].astype(np.float64)
    if gate:
      x = np.where((vis[b:b + n] > 0)[:, None], x, 0.0)
    err = np.abs(modelled[k].astype(np.float64) - x.sum(axis=0))
    bound = max(n - 1, 0) * U * np.abs(x).sum(axis=0)
    if (err > bound).any():
      return np.inf
    worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
  return worst


REDUCTION_M = (1, 255, 256, 257, 700)
REDUCTION_COUNTS = (0, 1, 2, 3, 17, 63, 64, 65, 128, 129, 300, 700)
WIDE_C = (4, 5, 8, 16)


def wide_cw(C):
  return 4 if C <= 4 else 8 if C <= 8 else 16


class ReductionCase:
  """count / offsets / order [M], vis [O] (about 30 % zeros), partial [O, 24] with NaN rows where vis == 0: the narrow
  form reads columns 0-10 as its 11 sums (its 12th float is padding), the wide forms columns 0-7 and 8 .. 8 + CW."""

  def __init__(self, M):
    rng = np.random.default_rng(3200 + M)
    weights = np.array([6, 8, 8, 8, 8, 6, 6, 4, 2, 2, 1, 0.5])
    count = rng.choice(REDUCTION_COUNTS, M, p=weights / weights.sum())
    forced = {1: {0: 700},
              255: {0: 0, 254: 300, 64: 65, 127: 129, 10: 128, 20: 65},
              256: {0: 300, 255: 0, 63: 700, 100: 64, 101: 65},
              257: {255: 0, 256: 129, 0: 63, 1: 64, 2: 64, 3: 64, 4: 17},
              700: {0: 0, 255: 0, 64: 300, 127: 65, 130: 128, 140: 700, 512: 0, 699: 0,
                    513: 63, 514: 64, 515: 64, 516: 64, 517: 17}}[M]
    if M == 700:
      count[256:512] = 0                                          # a block whose ranks all have count 0
    for k, n in forced.items():
      count[k] = n
    self.M, self.count = M, count.astype(np.uint32)
    self.offsets = (np.cumsum(count) - count).astype(np.uint32)
    self.O = O = int(count.sum())
    self.order = rng.permutation(M).astype(np.uint32)
    mag = lambda shape: (10.0 ** rng.uniform(-6, 3, shape)).astype(np.float32)
    self.vis = np.where(rng.random(O) < 0.3, np.float32(0), mag(O)).astype(np.float32)
    self.partial = (mag((O, 24)) * rng.choice(np.float32([-1, 1]), (O, 24))).astype(np.float32)
    self.partial[self.vis == 0] = np.nan

  def features(self):
    """Which of the placements the contract asks for occur in this case."""
    c, o, f = self.count.astype(np.int64), self.offsets.astype(np.int64), set()
    for b0 in range(0, self.M, CHUNK):
      blk, off = c[b0:b0 + CHUNK], o[b0:b0 + CHUNK]
      if len(blk) > 1 and not blk.any():
        f.add("empty block")
      if len(blk) > 1 and blk[0] == 0:
        f.add("zero at block start")
      if len(blk) > 1 and blk[-1] == 0:
        f.add("zero at block end")
      rel = off - off[0]                                         # chunks are counted from the block's first slot
      serial = (blk > 0) & (blk <= SERIAL)
      if (serial & (rel // CHUNK != (rel + blk - 1) // CHUNK)).any():
        f.add("serial rank across a chunk boundary")
    large = np.flatnonzero(c > SERIAL)
    if (large % 64 == 0).any():
      f.add("large rank in lane 0")
    if (large % 64 == 63).any():
      f.add("large rank in lane 63")
    if len(large) and np.bincount(large // 64).max() >= 2:
      f.add("two large ranks in one wave")
    return f


REDUCTION_FEATURES = {"empty block", "zero at block start", "zero at block end", "serial rank across a chunk boundary",
                      "large rank in lane 0", "large rank in lane 63", "two large ranks in one wave"}


@functools.lru_cache(maxsize=None)
def reduction_case(M):
  return ReductionCase(M)


@functools.lru_cache(maxsize=None)
def reduction_model(M, limit=None):
  """(visibility [M], sums [M, 24]) by rank: the visibility column adds every slot, the others are gated by it."""
  c = reduction_case(M)
  vis = model_reduce(c.vis[:, None], c.vis, c.offsets, c.count, gate=False, limit=limit)[:, 0]
  sums = None if limit is not None else model_reduce(c.partial, c.vis, c.offsets, c.count, gate=True)
  return vis, sums


def narrow_rows(M, order):
  """The [M, 16] rows gsr_reduce_gradients writes, at the rows `order` names (None: rank = row)."""
  vis, sums = reduction_model(M)
  rows = np.zeros((M, 16), np.float32)
  at = np.arange(M) if order is None else order.astype(np.int64)
  rows[at, :11], rows[at, 11] = sums[:, :11], vis
  return rows


def wide_rows(M, C, order):
  """(rows [M, 16], d_features [M, C]) of gsr_reduce_gradients_wide on partial[:, :8 + CW]."""
  vis, sums = reduction_model(M)
  rows, feat = np.zeros((M, 16), np.float32), np.zeros((M, C), np.float32)
  at = np.arange(M) if order is None else order.astype(np.int64)
  rows[at, :8], rows[at, 11], feat[at] = sums[:, :8], vis, sums[:, 8:8 + C]
  return rows, feat
