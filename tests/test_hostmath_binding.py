"""The binding of the host shim (tests/hostmath.py), derived from csrc/hostmath_shim.h: every declared function is in the
built library, an array of the wrong dtype, layout or writeability is refused before the call, a scalar wider than 32
bits arrives whole, and the header reader takes the `hm_` prefix and a `void` return -- and only those."""
import ctypes as C

import numpy as np
import pytest

import controller_oracle as co
import hostmath
from splat_trainer_amd import _lib


def test_every_declared_function_resolves(built_libs):
  shim = hostmath.load(built_libs)
  assert hostmath.load(built_libs) is shim                                  # loaded once per process
  assert hostmath.FUNCTIONS and all(name.startswith("hm_") for name in hostmath.FUNCTIONS)
  for name, (ret, args) in hostmath.FUNCTIONS.items():
    assert callable(getattr(shim, name)), name
    restype, argtypes = hostmath.PROTOTYPES[name]
    assert (restype is None) == (ret == "void") and len(argtypes) == len(args), name


def _sh_basis_arguments():
  return np.zeros((2, 3), np.float32), np.zeros((2, 4), np.float32)         # hm_sh_basis(K, M, const float* dirs, float* Y)


def test_checked_arrays_pass(built_libs):
  dirs, Y = _sh_basis_arguments()
  hostmath.load(built_libs).hm_sh_basis(4, 2, dirs, Y)
  assert np.all(Y[:, 0] != 0)


def test_float64_array_to_a_const_float_pointer_raises(built_libs):
  dirs, Y = _sh_basis_arguments()
  with pytest.raises(TypeError, match=r"hm_sh_basis: argument 2 \(const float\*\) expects .*float32.*got dtype float64"):
    hostmath.load(built_libs).hm_sh_basis(4, 2, dirs.astype(np.float64), Y)
  assert not Y.any()                                                        # refused before the call


def test_non_contiguous_slice_raises(built_libs):
  _, Y = _sh_basis_arguments()
  wide = np.zeros((2, 6), np.float32)
  with pytest.raises(TypeError, match=r"hm_sh_basis: argument 2 .*C-contiguous.*non-contiguous"):
    hostmath.load(built_libs).hm_sh_basis(4, 2, wide[:, :3], Y)


def test_read_only_array_to_a_non_const_pointer_raises(built_libs):
  dirs, Y = _sh_basis_arguments()
  dirs.setflags(write=False)
  Y.setflags(write=False)
  with pytest.raises(TypeError, match=r"hm_sh_basis: argument 3 \(float\*\) expects .*writeable.*read-only"):
    hostmath.load(built_libs).hm_sh_basis(4, 2, dirs, Y)                     # dirs is `const`: read-only is fine there


def test_int_above_32_bits_arrives_intact(built_libs):
  """Rows 2^40 and 2^40 + 1 of the noise stream: a `first` cut to 32 bits would give rows 0 and 1."""
  shim, first, seed, step = hostmath.load(built_libs), 2 ** 40, 2 ** 33 + 7, 2 ** 35 + 11
  got, _ = co.shim_draws(shim, first, 2, seed, step)
  assert np.array_equal(got, co.words(np.array([first, first + 1], dtype=np.uint64), seed, step))
  assert not np.array_equal(got, co.shim_draws(shim, 0, 2, seed, step)[0])
  assert not np.array_equal(got, co.shim_draws(shim, first, 2, seed % 2 ** 32, step % 2 ** 32)[0])


HEADER = """#ifndef H
#define H
#include <stdint.h>
%s
#endif
"""


def test_parser_takes_the_prefix_and_a_void_return():
  text = HEADER % "void hm_f(const void* p, uint8_t* q, int64_t n);\nint hm_g(void);"
  _, _, functions = _lib.parse_header(text, prefix="hm_")
  assert functions == {"hm_f": ("void", ["const void*", "uint8_t*", "int64_t"]), "hm_g": ("int", [])}
  restype, argtypes = _lib.make_prototypes(functions, {})["hm_f"]
  assert restype is None and argtypes == [C.c_void_p, C.c_void_p, C.c_int64]
  assert _lib.parse_header(HEADER % "void gsr_f(int n);")[2] == {"gsr_f": ("void", ["int"])}


@pytest.mark.parametrize("declaration", ["int hm_f(void v);", "int hm_f(int n, void v);", "const void hm_f(int n);",
                                         "typedef struct S { void v; } S;"],
                         ids=["argument", "second_argument", "const_return", "field"])
def test_parser_refuses_void_held_by_value(declaration):
  with pytest.raises(_lib.GsplatHipError, match=r"shim\.h:4: cannot parse"):
    _lib.parse_header(HEADER % declaration, prefix="hm_", filename="shim.h")


@pytest.mark.parametrize("prefix,declaration", [("hm_", "int gsr_f(int n);"), ("gsr_", "int hm_f(int n);"),
                                                ("hm_", "int f(int n);"), ("gsr_", "int f(int n);")],
                         ids=["hm_given_gsr", "gsr_given_hm", "hm_given_none", "gsr_given_none"])
def test_parser_refuses_a_function_without_the_prefix(prefix, declaration):
  with pytest.raises(_lib.GsplatHipError, match=r":4: cannot parse"):
    _lib.parse_header(HEADER % declaration, prefix=prefix)
