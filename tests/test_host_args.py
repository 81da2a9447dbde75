"""The rules the Python wrappers share, each tested where it is written: ``_args.f32`` / ``require`` / ``on_one_device``
and ``_lib.ptr`` / ``call`` / ``workspace``.  Host only: CPU tensors, and native calls that return before any HIP call
(argument sets of test_abi_argument_contract.py)."""
import pytest
import torch

import splat_trainer_amd as sta
from splat_trainer_amd import _args, _lib

INVALID = _lib.CONSTANTS["GSR_ERR_INVALID_ARGUMENT"]
# gsr_point_basis(log_scaling, rotation, indexes, M, eps, basis_out, stream): M < 0 is refused and M == 0 returns, both
# before a pointer is looked at
BASIS_REFUSED = (None, None, None, -1, 1e-4, None, None)
BASIS_NOTHING = (None, None, None, 0, 1e-4, None, None)


# ---- f32 ------------------------------------------------------------------------------------------------------------
def test_f32_returns_a_qualifying_tensor_itself():
  t = torch.rand(5, 3)
  assert _args.f32(t) is t and _args.f32(t, detach=False) is t
  p = torch.rand(5, 3, requires_grad=True)
  d = _args.f32(p)
  assert d.data_ptr() == p.data_ptr() and not d.requires_grad and d.grad_fn is None      # same storage, no graph
  row = torch.rand(4, 6)[1]                                           # a contiguous view: still no copy
  assert _args.f32(row).data_ptr() == row.data_ptr()


@pytest.mark.parametrize("make", [lambda: torch.rand(5, 3).half(), lambda: torch.rand(5, 3).double(),
                                  lambda: torch.rand(3, 5).t(), lambda: torch.rand(5, 6)[:, ::2],
                                  lambda: torch.arange(15).reshape(5, 3)], ids=["f16", "f64", "transposed", "strided", "i64"])
def test_f32_converts_what_does_not_qualify(make):
  t = make()
  out = _args.f32(t)
  assert out.dtype is torch.float32 and out.is_contiguous() and out.shape == t.shape and not out.requires_grad
  assert torch.equal(out, t.to(torch.float32))
  assert out.data_ptr() != t.data_ptr()


def test_f32_align16():
  buffer = torch.rand(64)
  assert buffer.data_ptr() % 16 == 0
  off = buffer[1:21].view(5, 4)                                       # starts 4 bytes into the buffer
  assert off.data_ptr() % 16 == 4 and off.is_contiguous()
  assert _args.f32(off) is off                                        # without the option the start does not matter
  copy = _args.f32(off, align16=True)
  assert copy.data_ptr() % 16 == 0 and copy.data_ptr() != off.data_ptr() and torch.equal(copy, off)
  aligned = buffer[4:24].view(5, 4)
  assert aligned.data_ptr() % 16 == 0 and _args.f32(aligned, align16=True) is aligned
  both = _args.f32(off.double(), align16=True)                        # converted and aligned
  assert both.dtype is torch.float32 and both.data_ptr() % 16 == 0 and torch.equal(both, off)


def test_f32_without_detach_keeps_the_graph():
  leaf = torch.rand(4, 4, dtype=torch.float64, requires_grad=True)
  out = _args.f32(leaf, detach=False)
  assert out.dtype is torch.float32 and out.requires_grad and out.grad_fn is not None
  out.sum().backward()
  assert torch.equal(leaf.grad, torch.ones(4, 4, dtype=torch.float64))             # back through the cast, in its dtype
  plain = torch.rand(4, 4, requires_grad=True)
  assert _args.f32(plain, detach=False) is plain
  assert not _args.f32(leaf).requires_grad


# ---- ptr ------------------------------------------------------------------------------------------------------------
def test_ptr():
  t = torch.rand(6, 3)
  assert _lib.ptr(None) is None and _lib.ptr(0) is None
  assert _lib.ptr(torch.empty(0)) is None and _lib.ptr(torch.empty(0, 3)) is None
  view = t[:0]
  assert view.numel() == 0 and view.storage_offset() == 0 and view.untyped_storage().data_ptr() == t.data_ptr() != 0
  assert _lib.ptr(view) is None and _lib.ptr(t[6:]) is None      # (whatever address torch reports for a view of no rows)
  assert _lib.ptr(0x10000) == 0x10000
  assert _lib.ptr(t) == t.data_ptr() and _lib.ptr(t[2:]) == t.data_ptr() + 24


# ---- call, workspace ------------------------------------------------------------------------------------------------
def test_call_raises_under_the_functions_name():
  message = _lib.load().gsr_error_string(INVALID).decode()
  with pytest.raises(sta.GsplatHipError) as raised:
    _lib.call("gsr_point_basis", *BASIS_REFUSED)
  assert str(raised.value) == f"gsr_point_basis failed: {message} ({INVALID})"
  with pytest.raises(sta.GsplatHipError) as raised:
    _lib.call("gsr_point_basis", *BASIS_REFUSED, note="(the rows)")
  assert str(raised.value) == f"gsr_point_basis(the rows) failed: {message} ({INVALID})"
  with pytest.raises(sta.GsplatHipError) as raised:                     # check is where the text is made
    _lib.check(INVALID, "gsr_point_basis")
  assert str(raised.value) == f"gsr_point_basis failed: {message} ({INVALID})"


def test_call_returns_the_code():
  assert _lib.call("gsr_point_basis", *BASIS_NOTHING) == 0
  assert _lib.call("gsr_point_basis", *BASIS_NOTHING, note="(nothing)") == 0
  with pytest.raises(AttributeError):
    _lib.call("gsr_no_such_entry_point")


def test_workspace_is_never_empty():
  for nbytes in (0, 1, 257):
    ws = _lib.workspace(nbytes, "cpu")
    assert ws.dtype is torch.uint8 and ws.numel() == max(nbytes, 1) and _lib.ptr(ws) is not None


# ---- require, on_one_device -----------------------------------------------------------------------------------------
def test_require_passes_and_returns_the_tensor():
  t = torch.zeros(5, 3)
  assert _args.require("rows", t) is t
  assert _args.require("rows", t, shape=(5, 3), dtype=torch.float32) is t
  assert _args.require("rows", t, shape=("N", 3)) is t
  assert _args.require("rows", t, shape=[(5,), (5, 3)]) is t
  assert _args.require("rows", torch.zeros(0, 3), shape=("N", 3)) is not None


@pytest.mark.parametrize("kwargs, error, words", [
    (dict(t=[1.0]), ValueError, ("rows must be a torch.Tensor", "list")),
    (dict(t=None, what="the test step"), ValueError, ("rows must be a torch.Tensor", "NoneType")),
    (dict(shape=(5, 4)), ValueError, ("rows must be (5, 4)", "got shape (5, 3)")),
    (dict(shape=(5,)), ValueError, ("rows must be (5,)", "got shape (5, 3)")),
    (dict(shape=("N", 4)), ValueError, ("rows must be (N, 4)", "got shape (5, 3)")),
    (dict(shape=("N", 3, 1)), ValueError, ("rows must be (N, 3, 1)", "shape")),
    (dict(shape=[(5, 1), (5,)]), ValueError, ("rows must be (5, 1) or (5,)", "got shape (5, 3)")),
    (dict(dtype=torch.float16), ValueError, ("rows must be torch.float16", "got torch.float32")),
    (dict(shape=(5, 4), dtype=torch.float16, what="the test step"), ValueError, ("rows must be (5, 4)",)),  # shape first
    (dict(dtype=torch.float16, what="the test step"), ValueError, ("rows must be torch.float16",)),      # dtype < device
    (dict(what="the test step"), sta.GsplatHipError,
     ("rows is on cpu", "the test step", "HIP device only", "no CPU fallback")),
    (dict(shape=(5, 3), dtype=torch.float32, what="the test step", device_error=ValueError), ValueError,
     ("rows is on cpu", "the test step", "HIP device only", "no CPU fallback")),
])
def test_require_refuses(kwargs, error, words):
  kwargs = dict(kwargs)
  t = kwargs.pop("t", torch.zeros(5, 3))
  with pytest.raises(error) as raised:
    _args.require("rows", t, **kwargs)
  assert type(raised.value) is error
  for word in words:
    assert word in str(raised.value), (word, str(raised.value))


def test_on_one_device():
  a, b = torch.zeros(3), torch.zeros(4)
  _args.on_one_device(dict(a=a, b=b, c=None))                           # no phrase: CPU tensors are nobody's business
  _args.on_one_device({})
  with pytest.raises(sta.GsplatHipError, match="a is on cpu: the test step runs on the HIP device only"):
    _args.on_one_device(dict(c=None, a=a, b=b), what="the test step")
  with pytest.raises(ValueError, match="b is on cpu: the test step") as raised:
    _args.on_one_device(dict(b=b), what="the test step", device_error=ValueError)
  assert type(raised.value) is ValueError
  meta = torch.zeros(3, device="meta")                                  # a second device that needs no hardware
  with pytest.raises(ValueError, match="inputs on different devices: a on cpu, m on meta"):
    _args.on_one_device(dict(a=a, m=meta, c=None))
