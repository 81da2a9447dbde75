"""Static budget of the pose-table kernels (csrc/camera_table.hip) on gfx950 -- hipcc cross-compiles without a GPU: the
two kernels are there, with no scratch, no LDS and no more registers than the build they were measured in
(profiles/r21_camera_table.txt), and the code holds no float atomic."""
import re

import pytest

from isa import FLOAT_ATOMIC, compiled

VGPRS = {"pose_forward_kernel": 52, "pose_backward_kernel": 48}     # as built


@pytest.fixture(scope="module")
def isa():
  return compiled("camera_table.hip")


def test_every_pose_kernel_is_there_inside_its_budget(isa):
  _, meta = isa
  for needle, vgprs in VGPRS.items():
    names = [n for n in meta if re.search(rf"\d{needle}E", n)]
    assert len(names) == 1, (needle, names)
    k = meta[names[0]]
    print(f"{needle}: {k['vgpr']} VGPRs, {k['sgpr']} SGPRs, scratch {k['scratch']} B, LDS {k['lds']} B")
    assert k["scratch"] == 0 and not k["lds"] and k["vgpr"] <= vgprs, (names[0], k["vgpr"], k["scratch"], k["lds"])
  assert len(meta) == len(VGPRS), sorted(meta)


def test_no_float_atomics(isa):
  asm, _ = isa
  assert not FLOAT_ATOMIC.findall(asm)
