"""The argument contracts of gsr_fuse_check, gsr_fuse_mask, gsr_fuse_emit and gsr_voxel_downsample
(include/gsplat_hip.h), code by code and in the stated precedence.  Host only, as tests/test_abi_undistort_contract.py
(whose caller this uses): every case returns in the wrapper's own checks, so device pointers are stand-in addresses that
are never read; the host arrays are real.  The host shim runs the same checks from the same header and must agree."""
import ctypes as C

import numpy as np
import pytest

import hostmath
from splat_trainer_amd import _lib
from test_abi_argument_contract import INVALID, NAMES, OK, PTR, TOO_SMALL, UNSUPPORTED, _label, call, nulls

CHECK, MASK, EMIT, VOXEL = "gsr_fuse_check", "gsr_fuse_mask", "gsr_fuse_emit", "gsr_voxel_downsample"
NAN, INF = float("nan"), float("inf")
_KEEP = []


def host(values, **at):
  """The address of a host array of doubles: `values` with the entries `at` = {_index: value} replaced."""
  a = np.array(values, np.float64).reshape(-1)
  for k, v in at.items():
    a[int(k[1:])] = v
  _KEEP.append(a)
  return a.ctypes.data


def table(*sources):
  """GsrFuseSource[len(sources)] of (depth, H, W)."""
  t = (_lib.GsrFuseSource * len(sources))(*[_lib.GsrFuseSource(depth=d, H=h, W=w) for d, h, w in sources])
  _KEEP.append(t)
  return t


INTR = [0.1, 0.1, 6.5, 4.5]
PARAMS = np.concatenate([np.eye(3, 4).reshape(12), [10.0, 10.0, 5.5, 3.5]])
PARAMS2 = np.concatenate([PARAMS, PARAMS])
WORLD = np.eye(3, 4).reshape(12)
GRID = [0.5, 0.0, 1.0, -1.0]
TWO = table((PTR, 7, 11), (PTR, 5, 17))
DEFAULTS = {
    CHECK: dict(Hr=9, Wr=13, ref_intrinsics_host=host(INTR), sources_host=TWO, source_params_host=host(PARAMS2), S=2,
                tolerances_host=host([0.1, 0.01])),
    MASK: dict(Hr=9, Wr=13, min_agree=2, max_violate=0),
    EMIT: dict(Hr=9, Wr=13, ref_intrinsics_host=host(INTR), world_t_ref_host=host(WORLD), min_agree=2, max_violate=0,
               base=0, capacity=100),
    VOXEL: dict(N=8, grid_host=host(GRID)),
}
CHECK_DEVICE = dict(ref_depth=None, counts=None)
EMIT_DEVICE = {n: None for n in ("ref_depth", "counts", "image", "block_offsets", "points_out", "colors_out", "agree_out")}
VOXEL_DEVICE = {n: None for n in ("points", "colors", "points_out", "colors_out", "counts_out", "K_dev", "workspace")}

CASES = [
    # ---- gsr_fuse_check: a negative size
    (CHECK, dict(Hr=-1), INVALID), (CHECK, dict(Wr=-1), INVALID), (CHECK, dict(Wr=-1, Hr=40000), INVALID),
    # a side above 32768, before S and the host arrays are looked at
    (CHECK, dict(Hr=32769), UNSUPPORTED), (CHECK, dict(Wr=32769, S=0), UNSUPPORTED),
    (CHECK, dict(Wr=32769, ref_intrinsics_host=None), UNSUPPORTED),
    # S, the host arrays and their values
    (CHECK, dict(S=0), INVALID), (CHECK, dict(S=17), INVALID), (CHECK, dict(S=-1, sources_host=None), INVALID),
    (CHECK, dict(ref_intrinsics_host=None), INVALID), (CHECK, dict(sources_host=None), INVALID),
    (CHECK, dict(source_params_host=None), INVALID), (CHECK, dict(tolerances_host=None), INVALID),
    (CHECK, dict(ref_intrinsics_host=host(INTR, _0=NAN)), INVALID), (CHECK, dict(ref_intrinsics_host=host(INTR, _3=INF)), INVALID),
    (CHECK, dict(source_params_host=host(PARAMS2, _31=NAN)), INVALID), (CHECK, dict(source_params_host=host(PARAMS2, _3=-INF)), INVALID),
    (CHECK, dict(tolerances_host=host([NAN, 0.01])), INVALID), (CHECK, dict(tolerances_host=host([0.1, -0.01])), INVALID),
    (CHECK, dict(tolerances_host=host([0.1, INF])), INVALID),
    # a source's size: negative, then too large
    (CHECK, dict(sources_host=table((PTR, -1, 11), (PTR, 5, 40000))), INVALID),
    (CHECK, dict(sources_host=table((PTR, 7, 11), (PTR, 5, 32769))), UNSUPPORTED),
    (CHECK, dict(CHECK_DEVICE, Hr=0, sources_host=table((PTR, 7, 32769), (PTR, 5, 17))), UNSUPPORTED),   # ... before Hr == 0
    (CHECK, dict(CHECK_DEVICE, Hr=0, tolerances_host=host([0.1, NAN])), INVALID),
    # nothing to do
    (CHECK, dict(CHECK_DEVICE, Hr=0), OK), (CHECK, dict(CHECK_DEVICE, Wr=0), OK),
    (CHECK, dict(CHECK_DEVICE, Wr=0, sources_host=table((None, 7, 11), (None, 5, 17))), OK),
    # the device pointers, last; an empty source needs no depth
    (CHECK, dict(ref_depth=None), INVALID), (CHECK, dict(counts=None), INVALID),
    (CHECK, dict(sources_host=table((PTR, 7, 11), (None, 5, 17))), INVALID),
    (CHECK, dict(sources_host=table((None, 0, 11), (None, 5, 0)), counts=None), INVALID),
    (CHECK, dict(Hr=32768, Wr=32768, S=16, sources_host=table(*[(PTR, 32768, 32768)] * 16),
                 source_params_host=host(np.tile(PARAMS, 16)), counts=None), INVALID),    # the limits themselves pass
    # ---- gsr_fuse_mask
    (MASK, dict(Hr=-1, Wr=40000), INVALID), (MASK, dict(Wr=32769, min_agree=-1), UNSUPPORTED),
    (MASK, dict(min_agree=-1), INVALID), (MASK, dict(min_agree=256), INVALID), (MASK, dict(max_violate=-1), INVALID),
    (MASK, dict(max_violate=256), INVALID), (MASK, dict(nulls(MASK), Hr=0, max_violate=256), INVALID),
    (MASK, dict(nulls(MASK), Hr=0), OK), (MASK, dict(nulls(MASK), Wr=0, min_agree=255, max_violate=255), OK),
    (MASK, dict(ref_depth=None), INVALID), (MASK, dict(counts=None), INVALID), (MASK, dict(keep_out=None), INVALID),
    # ---- gsr_fuse_emit: a negative size, base or capacity
    (EMIT, dict(Hr=-1), INVALID), (EMIT, dict(Wr=-1), INVALID), (EMIT, dict(base=-1), INVALID), (EMIT, dict(capacity=-1), INVALID),
    (EMIT, dict(capacity=-1, Wr=40000), INVALID),
    (EMIT, dict(Hr=32769), UNSUPPORTED), (EMIT, dict(Wr=32769, min_agree=300), UNSUPPORTED),
    (EMIT, dict(min_agree=256), INVALID), (EMIT, dict(max_violate=-1), INVALID),
    (EMIT, dict(ref_intrinsics_host=None), INVALID), (EMIT, dict(world_t_ref_host=None), INVALID),
    (EMIT, dict(ref_intrinsics_host=host(INTR, _1=NAN)), INVALID), (EMIT, dict(world_t_ref_host=host(WORLD, _11=INF)), INVALID),
    (EMIT, dict(EMIT_DEVICE, Hr=0, world_t_ref_host=host(WORLD, _0=NAN)), INVALID),       # ... before Hr == 0 returns
    (EMIT, dict(EMIT_DEVICE, Hr=0), OK), (EMIT, dict(EMIT_DEVICE, Wr=0), OK), (EMIT, dict(EMIT_DEVICE, capacity=0), OK),
    (EMIT, dict(EMIT_DEVICE, base=100), OK), (EMIT, dict(EMIT_DEVICE, base=101, capacity=100), OK),
    (EMIT, dict(ref_depth=None), INVALID), (EMIT, dict(counts=None), INVALID), (EMIT, dict(block_offsets=None), INVALID),
    (EMIT, dict(points_out=None), INVALID), (EMIT, dict(colors_out=None), INVALID), (EMIT, dict(agree_out=None), INVALID),
    (EMIT, dict(base=99, agree_out=None), INVALID),
    # ---- gsr_voxel_downsample
    (VOXEL, dict(N=-1), INVALID), (VOXEL, dict(N=1 << 31), INVALID), (VOXEL, dict(N=-1, grid_host=None), INVALID),
    (VOXEL, dict(grid_host=None), INVALID), (VOXEL, dict(grid_host=host(GRID, _0=0.0)), INVALID),
    (VOXEL, dict(grid_host=host(GRID, _0=-0.5)), INVALID), (VOXEL, dict(grid_host=host(GRID, _0=NAN)), INVALID),
    (VOXEL, dict(grid_host=host(GRID, _0=INF)), INVALID), (VOXEL, dict(grid_host=host(GRID, _0=1e-320)), INVALID),
    (VOXEL, dict(grid_host=host(GRID, _2=NAN)), INVALID), (VOXEL, dict(grid_host=host(GRID, _3=-INF)), INVALID),
    (VOXEL, dict(VOXEL_DEVICE, N=0, grid_host=host(GRID, _1=INF)), INVALID),              # ... before N == 0 returns
    (VOXEL, dict(VOXEL_DEVICE, N=0, workspace_bytes=0), OK),                              # ... before any pointer
    (VOXEL, dict(points=None), INVALID), (VOXEL, dict(colors=None), INVALID), (VOXEL, dict(points_out=None), INVALID),
    (VOXEL, dict(colors_out=None), INVALID), (VOXEL, dict(counts_out=None), INVALID), (VOXEL, dict(K_dev=None), INVALID),
    (VOXEL, dict(K_dev=None, workspace_bytes=0), INVALID),                                # ... before the workspace
    (VOXEL, dict(workspace=None), TOO_SMALL), (VOXEL, dict(workspace_bytes=0), TOO_SMALL),
    (VOXEL, dict(workspace_bytes=4096), TOO_SMALL),
]
SHIM = {CHECK: "hm_fuse_check", MASK: "hm_fuse_mask", EMIT: "hm_fuse_emit", VOXEL: "hm_voxel_downsample"}
# what the shim's entry point does not take: the stream everywhere, the block offsets (it ranks in a plain walk), the
# workspace; K_dev is its K_out
SHIM_LEAVES_OUT = {"stream", "block_offsets", "workspace", "workspace_bytes"}


def _id(case):
  fn, over, _ = case
  shown = {k: ("host" if isinstance(v, (int, C.Array)) and k.endswith("_host") and v else v) for k, v in over.items()}
  return _label((fn, shown, None))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_returned_code(built_libs, case):
  fn, over, expected = case
  assert call(_lib.load(), fn, dict(DEFAULTS[fn], **over)) == expected


@pytest.mark.parametrize("case", [c for c in CASES if not SHIM_LEAVES_OUT & set(c[1])], ids=_id)
def test_host_shim_returns_the_same_code(built_libs, case):
  fn, over, expected = case
  assert callable(getattr(hostmath.load(built_libs), SHIM[fn]))
  lib = C.CDLL(built_libs[1])                                           # raw: the checked binding takes arrays, not addresses
  f = getattr(lib, SHIM[fn])
  f.restype, f.argtypes = hostmath.PROTOTYPES[SHIM[fn]]
  a = dict(DEFAULTS[fn], **over)
  args = []
  for name, ctype in zip(NAMES[fn], _lib.FUNCTIONS[fn][1]):
    if name in SHIM_LEAVES_OUT:
      continue
    v = a[name] if name in a else PTR if ctype.endswith("*") else 1
    args.append(C.addressof(v) if isinstance(v, C.Array) else v)
  assert f(*args) == expected


def test_the_entry_points_are_declared_with_the_stated_signatures():
  assert _lib.ABI_VERSION == 38 and _lib.CONSTANTS["GSR_FUSE_MAX_SOURCES"] == 16
  assert _lib.STRUCTS["GsrFuseSource"] == [("depth", "const float*", 0), ("H", "int32_t", 0), ("W", "int32_t", 0)]
  assert C.sizeof(_lib.GsrFuseSource) == 16
  for fn in (CHECK, MASK, EMIT, VOXEL):
    ret, args = _lib.FUNCTIONS[fn]
    kept = [(n, t) for n, t in zip(NAMES[fn], args) if n not in SHIM_LEAVES_OUT]
    kept = ["const void*" if t == "const GsrFuseSource*" else "int64_t*" if n == "K_dev" else t for n, t in kept]
    assert ret == "int" and hostmath.FUNCTIONS[SHIM[fn]] == ("int", kept), fn
  assert _lib.FUNCTIONS["gsr_voxel_workspace_bytes"] == ("size_t", ["int64_t"])


def test_the_workspace_size_grows_with_n(built_libs):
  lib = _lib.load()
  sizes = [lib.gsr_voxel_workspace_bytes(n) for n in (-5, 0, 1, 1000, 1 << 20, (1 << 31) - 1)]
  assert sizes[0] == sizes[1] > 0 and sizes == sorted(sizes) and sizes[-1] > 16 * ((1 << 31) - 1)
