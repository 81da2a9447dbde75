"""The argument contracts of gsr_tsdf_integrate and the four extraction entry points (include/gsplat_hip.h), code by
code and in the stated precedence.  Host only, as tests/test_abi_fusion_contract.py (whose helpers and caller this
uses): every case returns in the wrapper's own checks, so device pointers are stand-in addresses that are never read;
the host arrays are real.  The host shim runs the same checks from the same header and must agree."""
import ctypes as C

import numpy as np
import pytest

import hostmath
from splat_trainer_amd import _lib
from test_abi_argument_contract import INVALID, NAMES, OK, PTR, UNSUPPORTED, _label, call, nulls
from test_abi_fusion_contract import INF, NAN, PARAMS, PARAMS2, _KEEP, host

INTEGRATE, VMASK, VEMIT, FMASK, FEMIT = ("gsr_tsdf_integrate", "gsr_mesh_vertex_mask", "gsr_mesh_vertex_emit",
                                         "gsr_mesh_face_mask", "gsr_mesh_face_emit")


def table(*sources):
  """GsrTsdfSource[len(sources)] of (depth, image, H, W)."""
  t = (_lib.GsrTsdfSource * len(sources))(*[_lib.GsrTsdfSource(depth=d, image=i, H=h, W=w) for d, i, h, w in sources])
  _KEEP.append(t)
  return t


GRID = [0.5, 0.0, 1.0, -1.0]
TSDF = [0.1, 2.0, 0.5]
TWO = table((PTR, PTR, 7, 11), (PTR, None, 5, 17))
LATTICE = dict(nx=13, ny=9, nz=7)
DEFAULTS = {
    INTEGRATE: dict(LATTICE, grid_host=host(GRID), sources_host=TWO, source_params_host=host(PARAMS2), S=2, tsdf_host=host(TSDF)),
    VMASK: dict(LATTICE, min_weight=1),
    VEMIT: dict(LATTICE, grid_host=host(GRID), min_weight=1, capacity=100),
    FMASK: dict(LATTICE, min_weight=1),
    FEMIT: dict(LATTICE, min_weight=1, capacity=100),
}
NO_STATE = dict(state=None)
VEMIT_DEVICE = {n: None for n in ("state", "block_offsets", "cell_vertex_out", "vertices_out", "colors_out")}
FEMIT_DEVICE = {n: None for n in ("state", "cell_vertex", "block_offsets", "faces_out")}

CASES = [
    # ---- gsr_tsdf_integrate: a negative size, before everything
    (INTEGRATE, dict(nx=-1), INVALID), (INTEGRATE, dict(ny=-1), INVALID), (INTEGRATE, dict(nz=-1), INVALID),
    (INTEGRATE, dict(nz=-1, nx=1 << 30), INVALID),
    # more than 2^29 nodes, before S and the host arrays are looked at
    (INTEGRATE, dict(nx=1024, ny=1024, nz=513), UNSUPPORTED), (INTEGRATE, dict(nx=(1 << 29) + 1, ny=1, nz=1), UNSUPPORTED),
    (INTEGRATE, dict(nx=1 << 30, ny=1 << 30, nz=1 << 30), UNSUPPORTED), (INTEGRATE, dict(nx=1 << 20, ny=1 << 20, nz=1, S=0), UNSUPPORTED),
    (INTEGRATE, dict(nx=1024, ny=1024, nz=513, grid_host=None), UNSUPPORTED),
    (INTEGRATE, dict(NO_STATE, nx=1 << 30, ny=0), UNSUPPORTED),                                # a side alone, though there is no node
    # S, the host arrays and their values
    (INTEGRATE, dict(S=0), INVALID), (INTEGRATE, dict(S=17), INVALID), (INTEGRATE, dict(S=-1, sources_host=None), INVALID),
    (INTEGRATE, dict(grid_host=None), INVALID), (INTEGRATE, dict(sources_host=None), INVALID),
    (INTEGRATE, dict(source_params_host=None), INVALID), (INTEGRATE, dict(tsdf_host=None), INVALID),
    (INTEGRATE, dict(grid_host=host(GRID, _0=0.0)), INVALID), (INTEGRATE, dict(grid_host=host(GRID, _0=-0.5)), INVALID),
    (INTEGRATE, dict(grid_host=host(GRID, _0=NAN)), INVALID), (INTEGRATE, dict(grid_host=host(GRID, _0=1e-320)), INVALID),
    (INTEGRATE, dict(grid_host=host(GRID, _2=INF)), INVALID),
    (INTEGRATE, dict(source_params_host=host(PARAMS2, _31=NAN)), INVALID), (INTEGRATE, dict(source_params_host=host(PARAMS2, _3=-INF)), INVALID),
    (INTEGRATE, dict(tsdf_host=host(TSDF, _0=NAN)), INVALID), (INTEGRATE, dict(tsdf_host=host(TSDF, _1=0.0)), INVALID),
    (INTEGRATE, dict(tsdf_host=host(TSDF, _1=-2.0)), INVALID), (INTEGRATE, dict(tsdf_host=host(TSDF, _2=0.0)), INVALID),
    (INTEGRATE, dict(tsdf_host=host(TSDF, _2=INF)), INVALID),
    # a source's size: negative, then too large
    (INTEGRATE, dict(sources_host=table((PTR, PTR, -1, 11), (PTR, PTR, 5, 40000))), INVALID),
    (INTEGRATE, dict(sources_host=table((PTR, PTR, 7, 11), (PTR, PTR, 5, 32769))), UNSUPPORTED),
    (INTEGRATE, dict(NO_STATE, nz=0, sources_host=table((PTR, PTR, 7, 32769), (PTR, PTR, 5, 17))), UNSUPPORTED),      # ... before "no node"
    (INTEGRATE, dict(NO_STATE, nz=0, tsdf_host=host(TSDF, _1=NAN)), INVALID),
    # nothing to do
    (INTEGRATE, dict(NO_STATE, nx=0), OK), (INTEGRATE, dict(NO_STATE, ny=0, nx=1 << 29, nz=1 << 29), OK),
    (INTEGRATE, dict(NO_STATE, nz=0, sources_host=table((None, None, 7, 11), (None, None, 5, 17))), OK),
    # the device pointers, last; an image is optional, an empty source needs no depth
    (INTEGRATE, dict(state=None), INVALID), (INTEGRATE, dict(sources_host=table((PTR, None, 7, 11), (None, PTR, 5, 17))), INVALID),
    (INTEGRATE, dict(sources_host=table((None, None, 0, 11), (None, None, 5, 0)), state=None), INVALID),
    (INTEGRATE, dict(nx=1024, ny=1024, nz=512, S=16, sources_host=table(*[(PTR, None, 32768, 32768)] * 16),
                     source_params_host=host(np.tile(PARAMS, 16)), state=None), INVALID),      # the limits themselves pass
    # ---- gsr_mesh_vertex_mask
    (VMASK, dict(nx=-1, ny=1 << 30), INVALID), (VMASK, dict(nx=1024, ny=1024, nz=513, min_weight=0), UNSUPPORTED),
    (VMASK, dict(min_weight=0), INVALID), (VMASK, dict(min_weight=-3), INVALID),
    (VMASK, dict(nulls(VMASK), nz=1, min_weight=0), INVALID),                                  # ... before "no cell"
    (VMASK, dict(nulls(VMASK), nz=1), OK), (VMASK, dict(nulls(VMASK), nx=0), OK), (VMASK, dict(nulls(VMASK), nx=1, ny=1 << 20), OK),
    (VMASK, dict(state=None), INVALID), (VMASK, dict(active_out=None), INVALID),
    # ---- gsr_mesh_vertex_emit: a negative size or capacity
    (VEMIT, dict(ny=-1), INVALID), (VEMIT, dict(capacity=-1), INVALID), (VEMIT, dict(capacity=-1, nx=1024, ny=1024, nz=513), INVALID),
    (VEMIT, dict(nx=1024, ny=1024, nz=513, min_weight=0), UNSUPPORTED),
    (VEMIT, dict(min_weight=0), INVALID), (VEMIT, dict(grid_host=None), INVALID), (VEMIT, dict(grid_host=host(GRID, _0=0.0)), INVALID),
    (VEMIT, dict(grid_host=host(GRID, _3=NAN)), INVALID),
    (VEMIT, dict(VEMIT_DEVICE, ny=1, grid_host=host(GRID, _1=INF)), INVALID),                  # ... before "no cell"
    (VEMIT, dict(VEMIT_DEVICE, ny=1), OK), (VEMIT, dict(VEMIT_DEVICE, nz=0), OK),
    (VEMIT, dict(state=None), INVALID), (VEMIT, dict(block_offsets=None), INVALID), (VEMIT, dict(cell_vertex_out=None), INVALID),
    (VEMIT, dict(vertices_out=None), INVALID), (VEMIT, dict(colors_out=None), INVALID),
    (VEMIT, dict(capacity=0, vertices_out=None, colors_out=None, state=None), INVALID),        # the state all the same
    # ---- gsr_mesh_face_mask
    (FMASK, dict(nz=-1), INVALID), (FMASK, dict(nx=1024, ny=1024, nz=513), UNSUPPORTED), (FMASK, dict(min_weight=0), INVALID),
    (FMASK, dict(nulls(FMASK), nx=1), OK), (FMASK, dict(nulls(FMASK), nx=1, min_weight=0), INVALID),
    (FMASK, dict(state=None), INVALID), (FMASK, dict(cell_vertex=None), INVALID), (FMASK, dict(keep_out=None), INVALID),
    # ---- gsr_mesh_face_emit
    (FEMIT, dict(nx=-1), INVALID), (FEMIT, dict(capacity=-1), INVALID), (FEMIT, dict(nx=1024, ny=1024, nz=513), UNSUPPORTED),
    (FEMIT, dict(min_weight=0), INVALID), (FEMIT, dict(FEMIT_DEVICE, capacity=0, min_weight=0), INVALID),
    (FEMIT, dict(FEMIT_DEVICE, nx=1), OK), (FEMIT, dict(FEMIT_DEVICE, capacity=0), OK),
    (FEMIT, dict(state=None), INVALID), (FEMIT, dict(cell_vertex=None), INVALID), (FEMIT, dict(block_offsets=None), INVALID),
    (FEMIT, dict(faces_out=None), INVALID), (FEMIT, dict(capacity=1, faces_out=None), INVALID),
]
SHIM = {INTEGRATE: "hm_tsdf_integrate", VMASK: "hm_mesh_vertex_mask", VEMIT: "hm_mesh_vertex_emit", FMASK: "hm_mesh_face_mask",
        FEMIT: "hm_mesh_face_emit"}
# what the shim's entry points do not take: the stream, and the block offsets (they rank in a plain walk)
SHIM_LEAVES_OUT = {"stream", "block_offsets"}


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
  assert _lib.ABI_VERSION == 38 and _lib.CONSTANTS["GSR_FUSE_MAX_SOURCES"] == 16 and _lib.CONSTANTS["GSR_COMPACT_BLOCK"] == 256
  assert _lib.STRUCTS["GsrTsdfSource"] == [("depth", "const float*", 0), ("image", "const float*", 0), ("H", "int32_t", 0),
                                           ("W", "int32_t", 0)]
  assert C.sizeof(_lib.GsrTsdfSource) == 24
  lattice = ["int32_t", "int32_t", "int32_t"]
  assert _lib.FUNCTIONS[INTEGRATE] == ("int", ["int32_t*"] + lattice + ["const double*", "const GsrTsdfSource*", "const double*",
                                               "int32_t", "const double*", "void*"])
  assert _lib.FUNCTIONS[VMASK] == ("int", ["const int32_t*"] + lattice + ["int32_t", "uint8_t*", "void*"])
  assert _lib.FUNCTIONS[VEMIT] == ("int", ["const int32_t*"] + lattice + ["const double*", "int32_t", "const uint32_t*", "int64_t",
                                           "int32_t*", "float*", "uint8_t*", "void*"])
  assert _lib.FUNCTIONS[FMASK] == ("int", ["const int32_t*"] + lattice + ["int32_t", "const int32_t*", "uint8_t*", "void*"])
  assert _lib.FUNCTIONS[FEMIT] == ("int", ["const int32_t*"] + lattice + ["int32_t", "const int32_t*", "const uint32_t*", "int64_t",
                                           "int32_t*", "void*"])
  for fn in SHIM:                                                       # the twins: the same lists without what they leave out
    ret, args = _lib.FUNCTIONS[fn]
    kept = [t for n, t in zip(NAMES[fn], args) if n not in SHIM_LEAVES_OUT]
    kept = ["const void*" if t == "const GsrTsdfSource*" else t for t in kept]
    assert ret == "int" and hostmath.FUNCTIONS[SHIM[fn]] == ("int", kept), fn
