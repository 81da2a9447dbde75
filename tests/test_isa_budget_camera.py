"""Static budget of the camera-gradient kernels (geometry.hip) on gfx950 -- hipcc cross-compiles without a GPU: every
camera kernel is there with no scratch and at most 128 VGPRs, and the parameter-backward kernels keep the register counts
they had before the camera gradient existed (the camera terms are formed by kernels of their own, so that the parameter
gradients keep their bits)."""
import pytest

from isa import compiled

DEFAULT_VGPR = {"project_bwd_rows_kernelILi0E": 114, "project_bwd_rows_kernelILi1E": 102,
                "project_bwd_rows_kernelILi2E": 102, "project_bwd_kernelILb0E": 94, "project_bwd_kernelILb1E": 96}
CAMERA_KERNELS = ("project_bwd_camera_kernel", "project_bwd_rows_camera_kernel", "sh_camera_grad_kernel",
                  "cam_grad_finish_kernel")


@pytest.fixture(scope="module")
def geometry_kernels():
  return compiled("geometry.hip")[1]


def _one(meta, needle):
  names = [n for n in meta if needle in n]
  assert len(names) == 1, (needle, names)
  return meta[names[0]]


def test_every_camera_kernel_is_there_inside_its_budget(geometry_kernels):
  for needle in CAMERA_KERNELS:
    k = _one(geometry_kernels, needle)
    assert k["scratch"] == 0 and k["vgpr"] <= 128, (needle, k["vgpr"], k["scratch"])


def test_parameter_backward_kernels_keep_their_registers(geometry_kernels):
  for needle, vgpr in DEFAULT_VGPR.items():
    k = _one(geometry_kernels, needle)
    assert k["scratch"] == 0 and k["vgpr"] == vgpr, (needle, k["vgpr"])
