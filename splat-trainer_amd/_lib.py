"""ctypes binding of the C ABI in include/gsplat_hip.h.

There is no CPU fallback: if ``libgsplat_hip.so`` is missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

import torch

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libgsplat_hip.so")
HEADER_PATH = os.path.join(PKG_DIR, "..", "include", "gsplat_hip.h")


class GsplatHipError(RuntimeError):
  pass


# ---- the binding is derived from the header: include/gsplat_hip.h is the one place the ABI is written down ----------
# C types travel as normalised spellings ("int64_t", "const float*"); the rule that turns one into a ctypes type:
# scalars map to their ctypes scalar, a struct held by value is its mirror, a function argument pointing to one of the
# ABI's structs is POINTER(mirror), a `const char*` return is c_char_p and every other pointer -- every pointer field of
# a struct included -- is c_void_p (ctypes then takes a plain int address, no wrapper object per argument).
SCALARS = {"float": C.c_float, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32,
           "uint64_t": C.c_uint64, "size_t": C.c_size_t}

_TYPE = r"\s*(const\s+)?(\w+)\s*(\*?)\s*"
_DECLARATOR = r"\w+(?:\[\d+\])?"
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;")
_FUNCTION = re.compile(_TYPE + r"(\w+)\s*\(([^(){};]*)\)\s*;")
_FIELD = re.compile(_TYPE + rf"({_DECLARATOR}(?:\s*,\s*{_DECLARATOR})*)\s*")      # `T a;`, `T a, b, c;`, `T a[7];`
_ARGUMENT = re.compile(_TYPE + r"\w*\s*")
_DEFINE = re.compile(r"#\s*define\s+(\w+)(\([^)]*\))?\s*(.*)")                     # group 2: a function-like macro
_SPACE = re.compile(r"\s*")


def parse_header(text: str, prefix: str = "gsr_", filename: str = "gsplat_hip.h"):
  """The ABI a header text declares, in declaration order: (constants, structs, functions) with constants name -> int
  (the object-like macros that have a value), structs name -> [(field, C type, array length or 0)] and functions
  name -> (return C type, [argument C types]).  Function-like macros, #include, #ifndef / #endif guards and
  `extern "C"` carry no ABI; anything else it cannot read -- any other directive (#if, #else, #pragma: they could change
  what the compiler sees), a name declared twice, a function whose name lacks `prefix` and `void` held by value anywhere
  but as a function's return type included -- raises GsplatHipError naming `filename` and the line."""
  constants, structs, functions = {}, {}, {}

  def fail(pos):
    line = text.count("\n", 0, pos) + 1
    raise GsplatHipError(f"{filename}:{line}: cannot parse {text.splitlines()[line - 1].strip()!r}")

  def ctype(m, pos, returned=False):
    const, base, star = m.group(1, 2, 3)
    if not star and base not in SCALARS and base not in structs and not (returned and base == "void" and not const):
      fail(pos)                                                       # held by value: a scalar or an earlier struct
    return ("const " if const else "") + base + star

  def declare(table, name, value, pos):
    if name in table:
      fail(pos)
    table[name] = value

  def directive(m):
    d = _DEFINE.fullmatch(m.group().strip())
    if d is None:
      re.match(r"#\s*(include|ifndef|endif)\b", m.group().strip()) or fail(m.start())
    elif not d.group(2) and d.group(3):
      try:
        declare(constants, d.group(1), int(d.group(3), 0), m.start())
      except ValueError:
        fail(m.start())
    return ""

  blank = lambda m: "\n" * m.group().count("\n")                      # line numbers survive
  text = re.sub(r"/\*.*?\*/", blank, text, flags=re.S)
  text = re.sub(r"^#ifdef __cplusplus$.*?^#endif$", blank, text, flags=re.S | re.M)
  text = re.sub(r"^[ \t]*#.*$", directive, text, flags=re.M)

  pos = _SPACE.match(text).end()
  while pos < len(text):
    m = _STRUCT.match(text, pos)
    if m:
      fields, at = [], m.start(2)
      for decl in m.group(2).split(";"):
        if decl.strip():
          at_decl = at + len(decl) - len(decl.lstrip())
          d = _FIELD.fullmatch(decl) or fail(at_decl)
          for declarator in d.group(4).split(","):
            name, _, count = declarator.strip().partition("[")
            fields.append((name, ctype(d, at_decl), int(count[:-1] or 0)))
        at += len(decl) + 1
      declare(structs, m.group(1), fields, pos)
    else:
      m = _FUNCTION.match(text, pos) or fail(pos)
      m.group(4).startswith(prefix) or fail(pos)
      arguments = [] if m.group(5).strip() == "void" else m.group(5).split(",")
      declare(functions, m.group(4),
              (ctype(m, pos, returned=True), [ctype(_ARGUMENT.fullmatch(a) or fail(pos), pos) for a in arguments]), pos)
    pos = _SPACE.match(text, m.end()).end()
  return constants, structs, functions


def make_mirrors(structs) -> dict:
  """One ctypes.Structure per parsed struct, under the header's typedef name."""
  mirrors = {}
  for name, fields in structs.items():
    members = []
    for field, ctype, count in fields:
      t = C.c_void_p if ctype.endswith("*") else SCALARS.get(ctype) or mirrors[ctype]
      members.append((field, t * count if count else t))
    mirrors[name] = type(name, (C.Structure,), {"_fields_": members})
  return mirrors


def make_prototypes(functions, mirrors) -> dict:
  """name -> (restype, argtypes) for every parsed function; a `void` return is restype None."""
  def argument(ctype):
    base = ctype.removeprefix("const ").rstrip("*")
    if ctype.endswith("*"):
      return C.POINTER(mirrors[base]) if base in mirrors else C.c_void_p
    return SCALARS.get(base) or mirrors[base]
  returns = {"const char*": C.c_char_p, "void": None}
  return {name: (returns[ret] if ret in returns else argument(ret), [argument(a) for a in args])
          for name, (ret, args) in functions.items()}


with open(HEADER_PATH) as _f:
  CONSTANTS, STRUCTS, FUNCTIONS = parse_header(_f.read())
MIRRORS = make_mirrors(STRUCTS)
# The mirrors are module attributes under the header's typedef names -- GsrRasterParamsC, GsrSegmentsC, GsrFrameC,
# GsrFramePlanC, GsrFrameResultC, GsrFrameBackwardC, GsrColumnC, GsrColorModel, GsrColorGrads, GsrReg -- injected here:
# no class statement in this file defines them.
globals().update(MIRRORS)
PROTOTYPES = make_prototypes(FUNCTIONS, MIRRORS)

ABI_VERSION = CONSTANTS["GSR_ABI_VERSION"]
PREFETCH_MIN_ROWS = CONSTANTS["GSR_PREFETCH_MIN_ROWS"]
MAX_FEATURES = CONSTANTS["GSR_MAX_FEATURES"]
WIDE_MIN_FEATURES = CONSTANTS["GSR_WIDE_MIN_FEATURES"]
BILAGRID_MAX_SIDE = CONSTANTS["GSR_BILAGRID_MAX_SIDE"]
KNN_MAX_K = CONSTANTS["GSR_KNN_MAX_K"]
NEIGHBOURS_MAX_N = CONSTANTS["GSR_NEIGHBOURS_MAX_N"]
VISIBILITY_MAX_CAMERAS = CONSTANTS["GSR_VISIBILITY_MAX_CAMERAS"]
MAX_COLUMNS = CONSTANTS["GSR_MAX_COLUMNS"]


def raster_params(config) -> "GsrRasterParamsC":
  blur = float(config.blur_cov) + (float(config.aa_blur) if config.antialias else 0.0)
  return GsrRasterParamsC(                                    # noqa: F821  (injected above)
      alpha_threshold=float(config.alpha_threshold), clamp_max_alpha=float(config.clamp_max_alpha),
      T_eps=float(config.transmittance_eps), q_max=float(config.gaussian_scale) ** 2, blur=blur,
      antialias=1 if config.antialias else 0, tile_size=int(config.tile_size),
      margin_px=float(config.margin_tiles * config.tile_size))


_lib = None
_lock = threading.Lock()


def ptr(t):
  """Device address of a tensor's data as a plain int (the prototypes declare c_void_p: ctypes takes the int, no wrapper
  object per argument), or None (NULL) for None and for an empty tensor.  A raw address -- an int: buffers of the frame
  arena that are only ever handed to kernels are kept as addresses, see renderer._run_frame -- passes through, 0 as None."""
  if t is None:
    return None
  if isinstance(t, int):
    return t or None
  if t.numel() == 0:
    return None
  return t.data_ptr()


def current_stream_ptr() -> int:
  """hipStream_t of torch's current stream on the current device.  (torch.cuda.current_stream() costs ~13 us per call
  on this stack -- device-availability probing -- and a step makes a dozen launches; the raw getter costs well under 1 us.)"""
  return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())    # (0 = the null stream; ctypes passes the int)


def current_stream() -> "torch.cuda.Stream":
  """torch.cuda.current_stream() of the current device without the availability probe (explicit device index)."""
  return torch.cuda.current_stream(torch._C._cuda_getDevice())


def load() -> C.CDLL:
  """Loads (once) and returns the HIP library; raises GsplatHipError when it is absent."""
  global _lib
  if _lib is not None:
    return _lib
  with _lock:
    if _lib is not None:
      return _lib
    if not os.path.exists(LIB_PATH):
      raise GsplatHipError(
          f"{LIB_PATH} not found: build it with `python splat-trainer_amd/build.py` "
          "(hipcc --offload-arch=gfx950). There is no CPU fallback for the rasterizer path.")
    try:
      lib = C.CDLL(LIB_PATH)
    except OSError as e:
      raise GsplatHipError(f"failed to load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in PROTOTYPES.items():
      fn = getattr(lib, name)
      fn.restype = restype
      fn.argtypes = argtypes
    if lib.gsr_abi_version() != ABI_VERSION:
      raise GsplatHipError(f"ABI mismatch: library {lib.gsr_abi_version()} != binding {ABI_VERSION}; rebuild")
    # the mirrors must have the layout the library was compiled with: a stale .so fails here, not in a kernel
    frame_structs = ("GsrRasterParamsC", "GsrSegmentsC", "GsrFrameC", "GsrFramePlanC", "GsrFrameResultC",
                     "GsrFrameBackwardC")
    sized = [(lib.gsr_struct_bytes(i), n) for i, n in enumerate(frame_structs)]
    sized += [(lib.gsr_color_struct_bytes(i), n) for i, n in enumerate(("GsrColorModel", "GsrColorGrads"))]
    sized += [(lib.gsr_reg_struct_bytes(), "GsrReg")]
    for library_bytes, name in sized:
      if library_bytes != C.sizeof(MIRRORS[name]):
        raise GsplatHipError(f"struct layout mismatch: {name} is {C.sizeof(MIRRORS[name])} bytes in the binding, "
                             f"{library_bytes} in the library; rebuild")
    _lib = lib
  return _lib


def check(code: int, what: str) -> int:
  if code < 0:
    msg = load().gsr_error_string(code).decode()
    raise GsplatHipError(f"{what} failed: {msg} ({code})")
  return code


def call(name: str, *args, note: str = "", lib=None) -> int:
  """Calls the status-returning entry point ``name`` and returns its non-negative code; a negative one raises through
  ``check`` under that same name, with ``note`` behind it (``"(depth)"``: which of a wrapper's several calls it was).
  ``lib``: the library that holds ``name`` when it is not this one (the host-maths shim).  Calls that return a size
  (``*_workspace_bytes``, ``gsr_camera_grad_partial_rows``) have no status: they go through ``load()`` directly."""
  return check(getattr(lib or load(), name)(*args), name + note)


def workspace(nbytes: int, device) -> torch.Tensor:
  """A scratch buffer of ``nbytes`` bytes, at least one: the native wrappers refuse a NULL workspace even where they
  need no byte of it (``!workspace`` comes before the size test), and ``ptr`` of an empty tensor is NULL.  Pass it as
  ``ptr(ws), ws.numel()``."""
  return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


class on_device(torch.cuda.device):
  """``with on_device(dev) as stream``: ``torch.cuda.device(dev)`` that hands out the raw handle of the stream current
  there.  For the entry points that may be called with another device current; the frame path does not scope."""

  def __enter__(self) -> int:
    super().__enter__()
    return current_stream_ptr()
