"""The argument contracts of gsr_weighted_draws, gsr_relocate_weights, gsr_relocate_rescale and gsr_relocate_rows
(include/gsplat_hip.h), code by code and in the stated precedence: a count or a domain out of range first; for the draw
then the pointers and their alignment, then the workspace's size, then its alignment; for the other three the empty
cases that return GSR_OK before any pointer is looked at, and the pointers (for the row move: every column) last.  Host
only, as tests/test_abi_undistort_contract.py (whose caller this uses): every case returns in the wrapper's own checks,
so device pointers are stand-in addresses that are never read; the column table is host memory and real.  The host
shim's entry points run the same checks from the same header and must agree.  (Left out: argument sets that enqueue
something -- every accepted draw does, it writes the total.)"""
import ctypes as C

import pytest

import hostmath
from splat_trainer_amd import _lib
from test_abi_argument_contract import INVALID, NAMES, ODD, OK, PTR, SCALARS, TOO_SMALL, _label, call, nulls

DRAWS, WEIGHTS, RESCALE, ROWS = "gsr_weighted_draws", "gsr_relocate_weights", "gsr_relocate_rescale", "gsr_relocate_rows"
SHIM = {DRAWS: "hm_weighted_draws", WEIGHTS: "hm_relocate_weights", RESCALE: "hm_relocate_rescale", ROWS: "hm_relocate_rows"}
MAX_N = _lib.NEIGHBOURS_MAX_N
NAN = float("nan")


def columns(*overrides):
  """A table of columns, one per dict of field overrides (default: one good column)."""
  rows = [dict(dict(data=PTR, width_dwords=3, zero=0), **o) for o in (overrides or ({},))]
  return (_lib.GsrRowColumnC * len(rows))(*[_lib.GsrRowColumnC(**r) for r in rows])


BASE = {DRAWS: dict(N=8, n=4, domain=1), WEIGHTS: dict(N=8), RESCALE: dict(N=8, o_floor=0.1),
        ROWS: dict(n=4, N=8, n_columns=1, columns_host=columns())}

CASES = [
    # ---- the draw: ranges, then pointers and their alignment, then the workspace's size, then its alignment ----
    (DRAWS, dict(N=-1), INVALID), (DRAWS, dict(n=-1), INVALID), (DRAWS, dict(N=MAX_N + 1), INVALID),
    (DRAWS, dict(n=MAX_N + 1), INVALID), (DRAWS, dict(domain=-1), INVALID), (DRAWS, dict(domain=256), INVALID),
    (DRAWS, dict(N=-1, workspace_bytes=0), INVALID),                          # ... before the workspace
    (DRAWS, dict(total_out=None), INVALID), (DRAWS, dict(weights=None), INVALID), (DRAWS, dict(counts_out=None), INVALID),
    (DRAWS, dict(sources_out=None), INVALID), (DRAWS, dict(weights=ODD), INVALID), (DRAWS, dict(counts_out=ODD), INVALID),
    (DRAWS, dict(total_out=None, workspace_bytes=0), INVALID),                # a pointer before the workspace
    (DRAWS, dict(weights=ODD, workspace=None), INVALID),
    (DRAWS, dict(N=0, total_out=None, weights=None, counts_out=None), INVALID),             # total_out is always written
    (DRAWS, dict(workspace_bytes=0), TOO_SMALL), (DRAWS, dict(workspace=None), TOO_SMALL),
    (DRAWS, dict(N=257, workspace_bytes=15), TOO_SMALL),                      # two blocks of 256 rows: 16 bytes
    (DRAWS, dict(N=0, weights=None, counts_out=None, workspace_bytes=7), TOO_SMALL),        # N == 0 needs neither array
    (DRAWS, dict(n=0, sources_out=None, workspace_bytes=7), TOO_SMALL),                     # n == 0 needs no sources
    (DRAWS, dict(workspace=ODD, workspace_bytes=0), TOO_SMALL),               # the size before the alignment
    (DRAWS, dict(workspace=ODD), INVALID), (DRAWS, dict(N=257, workspace=ODD, workspace_bytes=16), INVALID),
    # ---- the weights ----
    (WEIGHTS, dict(N=-1), INVALID), (WEIGHTS, dict(N=MAX_N + 1), INVALID),
    (WEIGHTS, dict(nulls(WEIGHTS), N=-1), INVALID),
    (WEIGHTS, dict(nulls(WEIGHTS), N=0), OK),                                 # before any pointer is looked at
    (WEIGHTS, dict(alpha_logit=None), INVALID), (WEIGHTS, dict(weights_out=None), INVALID),
    (WEIGHTS, dict(alive=None, weights_out=None), INVALID),
    # ---- the rescale: N and o_floor, then N == 0, then the pointers ----
    (RESCALE, dict(N=-1), INVALID), (RESCALE, dict(N=MAX_N + 1), INVALID), (RESCALE, dict(o_floor=0.0), INVALID),
    (RESCALE, dict(o_floor=1.0), INVALID), (RESCALE, dict(o_floor=-0.1), INVALID), (RESCALE, dict(o_floor=NAN), INVALID),
    (RESCALE, dict(nulls(RESCALE), N=0, o_floor=0.0), INVALID),               # ... before N == 0 returns
    (RESCALE, dict(nulls(RESCALE), N=0), OK),
    (RESCALE, dict(alpha_logit=None), INVALID), (RESCALE, dict(log_scaling=None), INVALID), (RESCALE, dict(counts=None), INVALID),
    # ---- the row move: ranges, then the empty cases, then the pointers and every column ----
    (ROWS, dict(n=-1), INVALID), (ROWS, dict(N=-1), INVALID), (ROWS, dict(n=MAX_N + 1), INVALID), (ROWS, dict(N=MAX_N + 1), INVALID),
    (ROWS, dict(n_columns=-1), INVALID), (ROWS, dict(n_columns=_lib.MAX_COLUMNS + 1), INVALID),
    (ROWS, dict(nulls(ROWS), n=0, n_columns=_lib.MAX_COLUMNS + 1), INVALID),  # ... before n == 0 returns
    (ROWS, dict(nulls(ROWS), n=0), OK), (ROWS, dict(nulls(ROWS), N=0), OK), (ROWS, dict(nulls(ROWS), n_columns=0), OK),
    (ROWS, dict(nulls(ROWS), n=0, N=0, n_columns=0), OK),
    (ROWS, dict(dst_rows=None), INVALID), (ROWS, dict(src_rows=None), INVALID), (ROWS, dict(columns_host=None), INVALID),
    (ROWS, dict(columns_host=columns(dict(data=None))), INVALID), (ROWS, dict(columns_host=columns(dict(width_dwords=0))), INVALID),
    (ROWS, dict(columns_host=columns(dict(width_dwords=-3))), INVALID),
    (ROWS, dict(columns_host=columns(dict(width_dwords=(1 << 20) + 1))), INVALID),
    (ROWS, dict(columns_host=columns(dict(data=PTR + 2))), INVALID),          # 4-byte words
    (ROWS, dict(n_columns=3, columns_host=columns({}, dict(zero=1), dict(data=None))), INVALID),      # every column is looked at
]


def _arguments(fn, over):
  return dict(BASE[fn], **over)


@pytest.mark.parametrize("case", CASES, ids=_label)
def test_returned_code(built_libs, case):
  fn, over, expected = case
  assert call(_lib.load(), fn, _arguments(fn, over)) == expected


@pytest.mark.parametrize("case", CASES, ids=_label)
def test_host_shim_returns_the_same_code(built_libs, case):
  fn, over, expected = case
  assert callable(getattr(hostmath.load(built_libs), SHIM[fn]))
  lib = C.CDLL(built_libs[1])                                           # raw: the checked binding takes arrays, not addresses
  f = getattr(lib, SHIM[fn])
  f.restype, f.argtypes = hostmath.PROTOTYPES[SHIM[fn]]
  a, args = _arguments(fn, over), []
  for name, ctype in zip(NAMES[fn][:-1], _lib.FUNCTIONS[fn][1]):        # the same arguments less the stream
    v = a[name] if name in a else PTR if ctype.endswith("*") else SCALARS.get(name, 1)
    args.append(C.cast(v, C.c_void_p) if isinstance(v, C.Array) else v)
  assert f(*args) == expected


def test_the_entry_points_are_declared_once_with_the_stated_signatures():
  assert _lib.ABI_VERSION == 38                                          # additive: no signature changed
  assert _lib.STRUCTS["GsrRowColumnC"] == [("data", "void*", 0), ("width_dwords", "int32_t", 0), ("zero", "int32_t", 0)]
  assert C.sizeof(_lib.GsrRowColumnC) == 16
  want = {DRAWS: ["const uint32_t*", "int64_t", "int64_t", "uint64_t", "uint64_t", "int32_t", "int32_t*", "int32_t*",
                  "uint64_t*", "void*", "size_t", "void*"],
          WEIGHTS: ["const float*", "const uint8_t*", "int64_t", "uint32_t*", "void*"],
          RESCALE: ["float*", "float*", "const int32_t*", "int64_t", "float", "void*"],
          ROWS: ["const int32_t*", "const int32_t*", "int64_t", "int64_t", "const GsrRowColumnC*", "int32_t", "void*"]}
  for fn, args in want.items():
    assert _lib.FUNCTIONS[fn] == ("int", args), fn
    shim_args = ["const void*" if a == "const GsrRowColumnC*" else a for a in args[:-1]]      # the same less the stream
    assert hostmath.FUNCTIONS[SHIM[fn]] == ("int", shim_args), fn
  assert _lib.FUNCTIONS["gsr_weighted_draws_workspace_bytes"] == ("size_t", ["int64_t"])


def test_workspace_size_is_one_word_per_256_rows(built_libs):
  size = _lib.load().gsr_weighted_draws_workspace_bytes
  assert [size(n) for n in (0, 1, 256, 257, 4099, MAX_N)] == [8, 8, 8, 16, 8 * 17, 8 * 2 ** 23]
