"""The argument contract of gsr_image_resize_area_u8 (include/gsplat_hip.h), code by code and in the stated precedence:
a negative size before an unsupported channel count or side, those before a size that is no downscale, that before the
empty cases that return GSR_OK, and the pointers last.  Host only, as tests/test_abi_argument_contract.py (whose caller
this uses): every case returns in the wrapper's own checks, so the pointers are stand-in addresses that are never read.
The host shim's entry point runs the same checks from the same header and must agree."""
import pytest

import hostmath
from splat_trainer_amd import _lib
from test_abi_argument_contract import INVALID, OK, PTR, UNSUPPORTED, _label, call, nulls

FN = "gsr_image_resize_area_u8"
SIZES = dict(B=2, Hs=48, Ws=64, C=3, Hd=24, Wd=32)
NULLS = nulls(FN)

CASES = [
    # any negative size
    (FN, dict(B=-1), INVALID), (FN, dict(Hs=-1), INVALID), (FN, dict(Ws=-1), INVALID), (FN, dict(C=-1), INVALID),
    (FN, dict(Hd=-1), INVALID), (FN, dict(Wd=-1), INVALID),
    (FN, dict(Wd=-1, C=2), INVALID),                       # ... before the channel count
    (FN, dict(B=-1, Ws=40000), INVALID),                   # ... before the side limit
    (FN, dict(NULLS, B=0, Hd=-1), INVALID),                # ... before B == 0 returns
    # C outside {1, 3}
    (FN, dict(C=0), UNSUPPORTED), (FN, dict(C=2), UNSUPPORTED), (FN, dict(C=4), UNSUPPORTED),
    (FN, dict(C=2, Wd=65), UNSUPPORTED),                   # ... before upscaling is refused
    (FN, dict(NULLS, C=4, B=0), UNSUPPORTED),              # ... before B == 0 returns
    # a side above 32768
    (FN, dict(Ws=32769, Wd=32), UNSUPPORTED), (FN, dict(Hs=32769), UNSUPPORTED),
    (FN, dict(Ws=32769, Wd=40000), UNSUPPORTED),           # ... before upscaling is refused
    (FN, dict(NULLS, Hs=40000, B=0), UNSUPPORTED),
    # upscaling, and an empty destination of a non-empty source
    (FN, dict(Wd=65), INVALID), (FN, dict(Hd=49), INVALID), (FN, dict(Wd=0), INVALID), (FN, dict(Hd=0), INVALID),
    (FN, dict(NULLS, B=0, Wd=65), INVALID),                # ... before B == 0 returns
    (FN, dict(Ws=0, Wd=1), INVALID),                       # wider than an empty source
    # nothing to do: GSR_OK before any pointer is looked at
    (FN, dict(NULLS, B=0), OK), (FN, dict(NULLS, Ws=0, Wd=0), OK), (FN, dict(NULLS, Hs=0, Hd=0), OK),
    (FN, dict(NULLS, Hs=0, Hd=0, Ws=0, Wd=0), OK), (FN, dict(NULLS, Ws=0, Wd=0, Hd=0), OK),
    # the pointers, last
    (FN, dict(src=None), INVALID), (FN, dict(dst=None), INVALID), (FN, NULLS, INVALID),
    (FN, dict(C=1, src=None), INVALID),
    # the limits themselves pass the checks: equal sizes, and the largest side (stopped here by a NULL)
    (FN, dict(Ws=32768, Wd=32768, Hs=1, Hd=1, dst=None), INVALID),
]


@pytest.mark.parametrize("case", CASES, ids=_label)
def test_returned_code(built_libs, case):
  fn, over, expected = case
  assert call(_lib.load(), fn, dict(SIZES, **over)) == expected


@pytest.mark.parametrize("case", CASES, ids=_label)
def test_host_shim_returns_the_same_code(built_libs, case):
  _, over, expected = case
  a = {**SIZES, "src": PTR, "dst": PTR, **over}
  shim = hostmath.load(built_libs)
  import ctypes as C
  fn = C.CDLL(built_libs[1]).hm_image_resize_area_u8                 # raw: the checked binding takes arrays, not addresses
  fn.restype, fn.argtypes = hostmath.PROTOTYPES["hm_image_resize_area_u8"]
  assert callable(shim.hm_image_resize_area_u8)
  assert fn(a["src"], a["B"], a["Hs"], a["Ws"], a["C"], a["dst"], a["Hd"], a["Wd"]) == expected


def test_the_entry_point_is_declared_once_with_the_stated_signature():
  ret, args = _lib.FUNCTIONS[FN]
  assert ret == "int" and args == ["const uint8_t*", "int32_t", "int32_t", "int32_t", "int32_t", "uint8_t*", "int32_t",
                                   "int32_t", "void*"]
  ret_h, args_h = hostmath.FUNCTIONS["hm_image_resize_area_u8"]
  assert ret_h == "int" and args_h == args[:-1]                      # the same less the stream
