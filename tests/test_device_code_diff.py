"""tools/device_code_diff.py: how two tables of kernels are classified (no compiler involved).  identical: nothing is
reported; reordered: the same instructions in another order or on other registers, VGPRs and scratch not above, LDS
equal; everything else differs."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import device_code_diff as dcd  # noqa: E402

BODY = ["\tv_add_u32_e32 v0, v1, v2   ; a comment", ".LBB3_1:", "\tds_read_b32 v3, v0", "\ts_waitcnt lgkmcnt(0)",
        "\ts_cbranch_execz .LBB3_1", "\t.p2align 8", "\ts_endpgm"]


def kernel(body=BODY, vgpr=8, sgpr=16, scratch=0, lds=16):
  return dict(body=list(body), vgpr=vgpr, sgpr=sgpr, scratch=scratch, lds=lds)


def verdict(old, new):
  r = dcd.classify(dict(k=old), dict(k=new))
  assert r["compared"] == 1 and not r["appear"] and not r["vanish"]
  return "differ" if r["differ"] else ("reordered" if r["reordered"] else "identical")


def test_function_index_of_labels_and_comments_do_not_count():
  moved = [ln.replace(".LBB3_1", ".LBB7_1").replace("a comment", "another") for ln in BODY]
  assert verdict(kernel(), kernel(moved)) == "identical"


def test_mnemonics_leave_labels_and_directives_out():
  assert dcd.mnemonics(BODY) == {"v_add_u32_e32": 1, "ds_read_b32": 1, "s_waitcnt": 1, "s_cbranch_execz": 1, "s_endpgm": 1}


def test_another_order_or_other_registers_is_reordered():
  swapped = [BODY[2], BODY[1], BODY[0]] + BODY[3:]
  renamed = [ln.replace("v3", "v5") for ln in BODY]
  assert verdict(kernel(), kernel(swapped)) == "reordered"
  assert verdict(kernel(), kernel(renamed)) == "reordered"
  assert verdict(kernel(), kernel(swapped, vgpr=7, sgpr=20)) == "reordered"       # SGPRs are free to move


def test_anything_else_differs():
  one_more = BODY[:3] + ["\ts_waitcnt lgkmcnt(0)"] + BODY[3:]
  other_op = [ln.replace("v_add_u32_e32", "v_sub_u32_e32") for ln in BODY]
  swapped = [BODY[2], BODY[1], BODY[0]] + BODY[3:]
  assert verdict(kernel(), kernel(one_more)) == "differ"
  assert verdict(kernel(), kernel(other_op)) == "differ"
  assert verdict(kernel(), kernel(swapped, vgpr=9)) == "differ"
  assert verdict(kernel(), kernel(swapped, scratch=4)) == "differ"
  assert verdict(kernel(), kernel(swapped, lds=32)) == "differ"
  assert verdict(kernel(), kernel(swapped, lds=8)) == "differ"
  assert verdict(kernel(), kernel(sgpr=17, vgpr=9)) == "differ"                   # the same body, more registers


def test_appear_and_vanish():
  r = dcd.classify(dict(a=kernel(), b=kernel()), dict(b=kernel(), c=kernel()))
  assert r["compared"] == 1 and r["appear"] == ["c"] and r["vanish"] == ["a"] and not r["differ"] and not r["reordered"]
