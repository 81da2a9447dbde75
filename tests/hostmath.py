"""The one loader of the host-maths shim (libgsr_hostmath.so): ``load(built_libs).hm_*``.

The binding is derived from csrc/hostmath_shim.h with the reader of the main library's header, so no test states a C
signature.  A pointer parameter takes a numpy array, checked against the declared type (dtype, C-contiguous, writeable
unless `const`), None for NULL or -- `void*` only -- a ctypes.Structure by reference; scalars are plain Python numbers.
"""
import ctypes as C
import os

import numpy as np

from splat_trainer_amd import _lib

HEADER = os.path.join(_lib.PKG_DIR, "csrc", "hostmath_shim.h")
with open(HEADER) as _f:
  FUNCTIONS = _lib.parse_header(_f.read(), prefix="hm_", filename="hostmath_shim.h")[2]
PROTOTYPES = _lib.make_prototypes(FUNCTIONS, {})
DTYPES = {"float": np.float32, "double": np.float64, "int32_t": np.int32, "int64_t": np.int64, "uint32_t": np.uint32,
          "uint64_t": np.uint64, "int16_t": np.int16, "uint8_t": np.uint8, "void": None}          # void: any dtype
_shims = {}


def _address(name, i, ctype, a):
  """What ctypes passes for argument i (declared `ctype`, a pointer) of the shim's function `name`."""
  const, base = ctype.startswith("const "), ctype.removeprefix("const ").rstrip("*")
  if a is None:
    return None
  if isinstance(a, C.Structure) and base == "void":
    return C.addressof(a)
  want = DTYPES[base]
  found = (type(a).__name__ if not isinstance(a, np.ndarray) else
           f"dtype {a.dtype.name}" if want is not None and a.dtype != want else
           f"a non-contiguous {a.dtype.name} array" if not a.flags.c_contiguous else
           f"a read-only {a.dtype.name} array" if not (const or a.flags.writeable) else None)
  if found:
    raise TypeError(f"{name}: argument {i} ({ctype}) expects a C-contiguous {'' if const else 'writeable '}"
                    f"{np.dtype(want).name if want else 'numpy'} array, got {found}")
  return a.ctypes.data


def _checked(name, fn, ctypes):
  def call(*args):
    if len(args) != len(ctypes):
      raise TypeError(f"{name}: takes {len(ctypes)} arguments, got {len(args)}")
    return fn(*[_address(name, i, t, a) if t.endswith("*") else a for i, (t, a) in enumerate(zip(ctypes, args))])
  call.__name__ = name
  return call


class _Shim:
  def __init__(self, path):
    lib = C.CDLL(path)
    for name, (_, ctypes) in FUNCTIONS.items():
      fn = getattr(lib, name)                     # a declared function the library lacks raises here
      fn.restype, fn.argtypes = PROTOTYPES[name]
      setattr(self, name, _checked(name, fn, ctypes))


def load(built_libs):
  """The shim of the `built_libs` fixture's value, loaded and bound once per process."""
  path = built_libs[1]
  if path not in _shims:
    _shims[path] = _Shim(path)
  return _shims[path]
