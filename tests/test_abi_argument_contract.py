"""The argument contract of the C ABI's entry points: which code each returns for arguments it rejects, or accepts
without work, BEFORE it touches the device.  Host only: every case below returns in the wrapper's own checks -- no HIP
call is reached, so pointers that are never read on the host are stand-in addresses.  (Left out on purpose: argument
sets that enqueue something, such as gsr_frustum_cull with N == 0, which clears the count word.)

The table pins the codes and, where two faults meet, their precedence: a negative count is reported before an
unsupported K or C, an unsupported configuration before a zero count returns GSR_OK, and a zero count returns before
any pointer is looked at.
"""
import ctypes as C
import re

import pytest

from splat_trainer_amd import _lib

OK = _lib.CONSTANTS["GSR_OK"]
INVALID = _lib.CONSTANTS["GSR_ERR_INVALID_ARGUMENT"]
TOO_SMALL = _lib.CONSTANTS["GSR_ERR_WORKSPACE_TOO_SMALL"]
UNSUPPORTED = _lib.CONSTANTS["GSR_ERR_UNSUPPORTED"]

PTR = 0x10000          # a stand-in device address (16-byte aligned): passes the null checks, is never read
ODD = PTR + 4          # ... one that fails an alignment check
BIG = 1 << 40          # a workspace size no check finds too small

# every integer argument not named here defaults to 1, every float to 1.0, every pointer to PTR
SCALARS = dict(N=8, M=4, K=4, C=3, W=32, H=32, B=1, V=1, P=64, O=16, n=4, D=3, mode=0, stages=3, crop=0, levels=1, k=1,
               rank=0, slot=0, seg_pairs_cfg=0, heavy_min_cfg=0, dense_stride=64, camera_stride=3, stride=64, begin_bit=0,
               end_bit=32, workspace_bytes=BIG, GH=4, GW=4, L=4, num_bins=16, kept_total=4, n_tail=0, n_columns=1,
               A_left=2, A_right=2, lo=0.0, hi=1.0, eps=0.1, ridge=1.0)


def _argument_names():
  text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
  names = {}
  for fn in _lib.FUNCTIONS:
    inside = re.search(rf"\b{fn}\s*\(([^)]*)\)\s*;", text).group(1).strip()
    names[fn] = [] if inside == "void" else [re.search(r"(\w+)\s*$", a).group(1) for a in inside.split(",")]
  return names


NAMES = _argument_names()


def params(**fields):
  return _lib.GsrRasterParamsC(**dict(dict(alpha_threshold=1 / 255, clamp_max_alpha=0.99, T_eps=1e-4, q_max=9.0, blur=0.3,
                                           antialias=0, tile_size=16, margin_px=16.0), **fields))


def segments(**fields):
  """A segment plan whose every table is present (its pointers are never read here)."""
  full = {name: PTR for name, ctype, _ in _lib.STRUCTS["GsrSegmentsC"] if ctype.endswith("*")}
  return _lib.GsrSegmentsC(**{**full, "capacity": 4, "heavy_capacity": 2, **fields})


def frame(**fields):
  """A projected-mode frame (position NULL) of 8 splats with 3 channels on a 32 x 32 image."""
  base = dict(gaussians2d=PTR, depth=PTR, features=PTR, N=8, K=4, C=3, W=32, H=32, pair_capacity=64, near_plane=0.1,
              far_plane=100.0, params=params())
  return _lib.GsrFrameC(**dict(base, **fields))


def scene_frame(**fields):
  """The same with the scene's own tensors (position set: culled, projected and shaded by the frame)."""
  scene = {k: PTR for k in ("position", "log_scaling", "rotation_xyzw", "alpha_logit", "sh_features", "T_camera_world",
                            "projection", "camera_pos")}
  return frame(**dict(scene, **fields))


def frame_backward(**fields):
  full = {name: PTR for name, ctype, _ in _lib.STRUCTS["GsrFrameBackwardC"] if ctype.endswith("*")}
  base = dict(full, N=8, M=4, O=16, W=32, H=32, C=3, K=4, mode=0, sh_mode=0, params=params(), segments=None)
  return _lib.GsrFrameBackwardC(**dict(base, **fields))


def color_model(**fields):
  arrays = dict(weight=(C.c_void_p * 7)(*[PTR] * 7), bias=(C.c_void_p * 7)(*[PTR] * 7))
  return _lib.GsrColorModel(**dict(dict(P=8, G=0, H=32, L=1, S=3, color_channels=3, **arrays), **fields))


def reg(**fields):
  full = {name: PTR for name, ctype, _ in _lib.STRUCTS["GsrReg"] if ctype.endswith("*")}
  return _lib.GsrReg(**{**full, "M": 4, "N": 8, **fields})


def column(**fields):
  return (_lib.GsrColumnC * 1)(_lib.GsrColumnC(**dict(dict(src=PTR, dst=PTR, tail=None, width_dwords=3), **fields)))


STRUCT_DEFAULTS = {"GsrRasterParamsC": params, "GsrSegmentsC": lambda: None, "GsrFrameC": frame,
                   "GsrFramePlanC": _lib.GsrFramePlanC, "GsrFrameResultC": _lib.GsrFrameResultC,
                   "GsrFrameBackwardC": frame_backward, "GsrColorModel": color_model, "GsrColorGrads": lambda: None,
                   "GsrReg": reg, "GsrColumnC": column}
# pointers the wrappers read or write on the host
HOST_ARRAYS = {"bias_out": C.c_uint32, "max_key_out": C.c_uint32, "seg_pairs_out": C.c_int32, "heavy_min_out": C.c_int32,
               "strides1_host": C.c_int64 * 4, "strides2_host": C.c_int64 * 4, "strides_out_host": C.c_int64 * 4}


def call(lib, fn, over):
  _, ctypes_ = _lib.FUNCTIONS[fn]
  unknown = set(over) - set(NAMES[fn])
  assert not unknown, f"{fn} has no argument {sorted(unknown)}"
  args, keep = [], []
  for name, ctype in zip(NAMES[fn], ctypes_):
    base = ctype.removeprefix("const ").rstrip("*")
    if name in over:
      v = over[name]
    elif base in STRUCT_DEFAULTS:
      v = STRUCT_DEFAULTS[base]()
    elif name in HOST_ARRAYS:
      v = HOST_ARRAYS[name]()
    elif ctype.endswith("*"):
      v = PTR
    else:
      v = SCALARS.get(name, 1.0 if base == "float" else 1)
    keep.append(v)
    args.append(C.byref(v) if isinstance(v, C.Structure) or isinstance(v, C._SimpleCData) else v)
  return getattr(lib, fn)(*args)


def nulls(fn, *keep):
  """Every pointer argument NULL except the named ones."""
  return {n: None for n, t in zip(NAMES[fn], _lib.FUNCTIONS[fn][1]) if t.endswith("*") and n not in keep}


SEG_MAX = _lib.CONSTANTS["GSR_TILE_COUNT_OFFSETS_MAX"]
CASES = [
    # ---- geometry.hip ----
    ("gsr_frustum_cull", dict(N=-1), INVALID),
    ("gsr_frustum_cull", dict(N=1 << 31), INVALID),
    ("gsr_frustum_cull", dict(count_dev=None), INVALID),
    ("gsr_frustum_cull", dict(position=None), INVALID),
    ("gsr_frustum_cull", dict(workspace=None), TOO_SMALL),
    ("gsr_frustum_cull", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_frustum_cull", dict(indexes_out=None, workspace_bytes=0), INVALID),
    ("gsr_project_forward", dict(M=-1), INVALID),
    ("gsr_project_forward", dict(params_host=None), INVALID),
    ("gsr_project_forward", dict(nulls("gsr_project_forward", "params_host"), M=0), OK),
    ("gsr_project_forward", dict(depth_out=None), INVALID),
    ("gsr_project_backward", dict(M=-1), INVALID),
    ("gsr_project_backward", dict(nulls("gsr_project_backward", "params_host"), M=0), OK),
    ("gsr_project_backward", dict(d_alpha_logit=None), INVALID),
    ("gsr_camera_grad_finish", dict(rows=-1), INVALID),
    ("gsr_camera_grad_finish", dict(d_camera=None), INVALID),
    ("gsr_camera_grad_finish", dict(rows=2, camera_partials=None), INVALID),
    ("gsr_project_backward_camera", dict(M=-1), INVALID),
    ("gsr_project_backward_camera", dict(d_camera=None), INVALID),
    ("gsr_project_backward_camera", dict(camera_partials=None), INVALID),
    ("gsr_sh_camera_position_grad", dict(M=-1), INVALID),
    ("gsr_sh_camera_position_grad", dict(d_camera_pos=None), INVALID),
    ("gsr_sh_camera_position_grad", dict(dL_dcolors=None), INVALID),
    ("gsr_project_sh_forward", dict(M=-1, K=5), INVALID),
    ("gsr_project_sh_forward", dict(params_host=None, K=5), INVALID),
    ("gsr_project_sh_forward", dict(K=5), UNSUPPORTED),
    ("gsr_project_sh_forward", dict(K=0), UNSUPPORTED),
    ("gsr_project_sh_forward", dict(M=0, K=25), UNSUPPORTED),
    ("gsr_project_sh_forward", dict(nulls("gsr_project_sh_forward", "params_host"), M=0, K=16), OK),
    ("gsr_project_sh_forward", dict(sh_features=None), INVALID),
    ("gsr_pack_rows", dict(M=-1, C=7), INVALID),
    ("gsr_pack_rows", dict(C=0), UNSUPPORTED),
    ("gsr_pack_rows", dict(C=4), UNSUPPORTED),
    ("gsr_pack_rows", dict(M=0, C=4), UNSUPPORTED),
    ("gsr_pack_rows", dict(nulls("gsr_pack_rows", "params_host"), M=0), OK),
    ("gsr_pack_rows", dict(rows_out=None), INVALID),
    ("gsr_pack_rows_wide", dict(M=-1, C=3), INVALID),
    ("gsr_pack_rows_wide", dict(C=3), UNSUPPORTED),
    ("gsr_pack_rows_wide", dict(C=17), UNSUPPORTED),
    ("gsr_pack_rows_wide", dict(nulls("gsr_pack_rows_wide", "params_host"), M=0, C=8), OK),
    ("gsr_pack_rows_wide", dict(C=16, feat_rows_out=None), INVALID),
    ("gsr_project_backward_rows", dict(mode=3), INVALID),
    ("gsr_project_backward_rows", dict(mode=-1), INVALID),
    ("gsr_project_backward_rows", dict(M=9), INVALID),
    ("gsr_project_backward_rows", dict(params_host=None), INVALID),
    ("gsr_project_backward_rows", dict(M=0), OK),
    ("gsr_project_backward_rows", dict(mode=2, M=0, N=0), OK),
    ("gsr_project_backward_rows", dict(mode=2, d_position=None), INVALID),
    ("gsr_project_backward_rows", dict(mode=2, inverse=None), INVALID),
    ("gsr_project_backward_rows", dict(grad_rows=None), INVALID),
    ("gsr_project_backward_rows", dict(d_rotation=None), INVALID),
    ("gsr_project_backward_rows_camera", dict(M=-1), INVALID),
    ("gsr_project_backward_rows_camera", dict(d_camera=None), INVALID),
    ("gsr_project_backward_rows_camera", dict(mode=3), INVALID),
    ("gsr_sh_forward", dict(M=-1, K=5), INVALID),
    ("gsr_sh_forward", dict(K=5), UNSUPPORTED),
    ("gsr_sh_forward", dict(M=0, K=5), UNSUPPORTED),
    ("gsr_sh_forward", dict(nulls("gsr_sh_forward"), M=0, K=1), OK),
    ("gsr_sh_forward", dict(colors_out=None), INVALID),
    ("gsr_sh_backward", dict(M=-1, K=5), INVALID),
    ("gsr_sh_backward", dict(K=2), UNSUPPORTED),
    ("gsr_sh_backward", dict(nulls("gsr_sh_backward"), M=0, K=9), OK),
    ("gsr_sh_backward", dict(d_sh_features=None), INVALID),
    ("gsr_inverse_map", dict(M=9), INVALID),
    ("gsr_inverse_map", dict(N=1 << 31), INVALID),
    ("gsr_inverse_map", dict(nulls("gsr_inverse_map"), M=0, N=0), OK),
    ("gsr_inverse_map", dict(inverse_out=None), INVALID),
    ("gsr_sh_backward_dense", dict(M=9, K=5), INVALID),
    ("gsr_sh_backward_dense", dict(K=5), UNSUPPORTED),
    ("gsr_sh_backward_dense", dict(nulls("gsr_sh_backward_dense"), M=0, N=0), OK),
    ("gsr_sh_backward_dense", dict(inverse=None), INVALID),
    ("gsr_sh_backward_dense", dict(d_sh_features=None), INVALID),
    ("gsr_sh_backward_multi", dict(N=-1), INVALID),
    ("gsr_sh_backward_multi", dict(dense_stride=23), INVALID),
    ("gsr_sh_backward_multi", dict(camera_stride=2, K=5), INVALID),
    ("gsr_sh_backward_multi", dict(K=5), UNSUPPORTED),
    ("gsr_sh_backward_multi", dict(nulls("gsr_sh_backward_multi"), N=0), OK),
    ("gsr_sh_backward_multi", dict(nulls("gsr_sh_backward_multi"), num_cameras=0, accumulate=1), OK),
    ("gsr_sh_backward_multi", dict(sh_features=None), INVALID),
    # ---- binning.hip ----
    ("gsr_depth_key_range", dict(bias_out=None), INVALID),
    ("gsr_depth_key_range", dict(near_plane=0.1, far_plane=100.0), OK),
    ("gsr_depth_keys", dict(M=-1), INVALID),
    ("gsr_depth_keys", dict(nulls("gsr_depth_keys"), M=0), OK),
    ("gsr_depth_keys", dict(keys_out=None), INVALID),
    ("gsr_tile_count", dict(M=-1, params_host=params(tile_size=8)), INVALID),
    ("gsr_tile_count", dict(M=1 << 30), INVALID),
    ("gsr_tile_count", dict(W=0), INVALID),
    ("gsr_tile_count", dict(params_host=params(tile_size=8)), UNSUPPORTED),
    ("gsr_tile_count", dict(nulls("gsr_tile_count", "params_host"), M=0), OK),
    ("gsr_tile_count", dict(count_out=None), INVALID),
    ("gsr_tile_count", dict(W=16 * 0x10000), UNSUPPORTED),
    ("gsr_tile_count_offsets", dict(M=SEG_MAX + 1), INVALID),
    ("gsr_tile_count_offsets", dict(params_host=params(tile_size=32)), UNSUPPORTED),
    ("gsr_tile_count_offsets", dict(total_dev=None), INVALID),
    ("gsr_tile_count_offsets", dict(offsets_out=None, workspace_bytes=0), INVALID),
    ("gsr_tile_count_offsets", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_tile_count_offsets", dict(H=16 * 0x10000), UNSUPPORTED),
    ("gsr_tile_emit", dict(capacity=-1), INVALID),
    ("gsr_tile_emit", dict(capacity=1 << 31, params_host=params(tile_size=8)), INVALID),
    ("gsr_tile_emit", dict(params_host=params(tile_size=8)), UNSUPPORTED),
    ("gsr_tile_emit", dict(nulls("gsr_tile_emit", "params_host"), M=0), OK),
    ("gsr_tile_emit", dict(keys_out=None), INVALID),
    ("gsr_tile_ranges", dict(O=-1), INVALID),
    ("gsr_tile_ranges", dict(num_tiles=0), INVALID),
    ("gsr_tile_ranges", dict(nulls("gsr_tile_ranges"), O=0), OK),
    ("gsr_tile_ranges", dict(tile_range=None), INVALID),
    ("gsr_reduce_visibility", dict(M=-1), INVALID),
    ("gsr_reduce_visibility", dict(capacity=1 << 31), INVALID),
    ("gsr_reduce_visibility", dict(nulls("gsr_reduce_visibility"), M=0), OK),
    ("gsr_reduce_visibility", dict(offsets=None), INVALID),
    ("gsr_reduce_gradients", dict(M=-1), INVALID),
    ("gsr_reduce_gradients", dict(nulls("gsr_reduce_gradients"), M=0), OK),
    ("gsr_reduce_gradients", dict(count=None), INVALID),
    ("gsr_reduce_gradients_wide", dict(M=-1, C=3), INVALID),
    ("gsr_reduce_gradients_wide", dict(C=3), UNSUPPORTED),
    ("gsr_reduce_gradients_wide", dict(M=0, C=17), UNSUPPORTED),
    ("gsr_reduce_gradients_wide", dict(nulls("gsr_reduce_gradients_wide"), M=0, C=4), OK),
    ("gsr_reduce_gradients_wide", dict(C=8, vis_partial=None), INVALID),
    ("gsr_unpack_grad_rows", dict(M=-1, C=4), INVALID),
    ("gsr_unpack_grad_rows", dict(C=4), UNSUPPORTED),
    ("gsr_unpack_grad_rows", dict(C=0), UNSUPPORTED),
    ("gsr_unpack_grad_rows", dict(C=17, d_features=None), UNSUPPORTED),
    ("gsr_unpack_grad_rows", dict(nulls("gsr_unpack_grad_rows"), M=0, C=16), OK),
    ("gsr_unpack_grad_rows", dict(rows=None), INVALID),
    # ---- composite.hip, composite_wide.inc ----
    ("gsr_segment_thresholds", dict(num_tiles=0), INVALID),
    ("gsr_segment_thresholds", dict(seg_pairs_out=None), INVALID),
    ("gsr_segment_thresholds", dict(num_tiles=4), OK),
    ("gsr_segment_thresholds_wide", dict(heavy_min_out=None), INVALID),
    ("gsr_segment_plan", dict(num_tiles=0), INVALID),
    ("gsr_segment_plan", dict(capacity=0), INVALID),
    ("gsr_segment_plan", dict(O=-1, O_dev=None), INVALID),
    ("gsr_segment_plan", dict(heavy_capacity=2), INVALID),
    ("gsr_segment_plan", dict(seg_pairs_cfg=128, heavy_min_cfg=64), INVALID),
    ("gsr_segment_plan", dict(tile_range=None), INVALID),
    ("gsr_segment_plan_wide", dict(capacity=1 << 31), INVALID),
    ("gsr_segment_plan_wide", dict(seg_desc_out=None), INVALID),
    ("gsr_composite_forward", dict(params_host=None), INVALID),
    ("gsr_composite_forward", dict(W=0, C=4), INVALID),
    ("gsr_composite_forward", dict(params_host=params(tile_size=8)), UNSUPPORTED),
    ("gsr_composite_forward", dict(C=0), UNSUPPORTED),
    ("gsr_composite_forward", dict(C=4, tile_range=None), UNSUPPORTED),
    ("gsr_composite_forward", dict(tile_range=None), INVALID),
    ("gsr_composite_forward", dict(pair_vis_out=None), INVALID),
    ("gsr_composite_forward", dict(segments_host=segments(seg_desc=None)), INVALID),
    ("gsr_composite_forward", dict(segments_host=segments(seg_median=None)), INVALID),
    ("gsr_composite_backward", dict(H=0), INVALID),
    ("gsr_composite_backward", dict(C=4), UNSUPPORTED),
    ("gsr_composite_backward", dict(dL_dimage=None), INVALID),
    ("gsr_composite_backward", dict(segments_host=segments(), image=None), INVALID),
    ("gsr_composite_backward", dict(segments_host=segments(seg_TC=None)), INVALID),
    ("gsr_composite_forward_wide_seg", dict(W=0, C=3), INVALID),
    ("gsr_composite_forward_wide_seg", dict(C=3), UNSUPPORTED),
    ("gsr_composite_forward_wide_seg", dict(C=17), UNSUPPORTED),
    ("gsr_composite_forward_wide_seg", dict(C=8, params_host=params(tile_size=8)), UNSUPPORTED),
    ("gsr_composite_forward_wide_seg", dict(C=8, last_out=None), INVALID),
    ("gsr_composite_forward_wide_seg", dict(C=8, pair_vis_out=None), INVALID),
    ("gsr_composite_forward_wide_seg", dict(C=8, segments_host=segments(seg_col=None)), INVALID),
    ("gsr_composite_forward_wide", dict(C=3), UNSUPPORTED),
    ("gsr_composite_forward_wide", dict(C=4, image_out=None), INVALID),
    ("gsr_composite_backward_wide_seg", dict(C=3), UNSUPPORTED),
    ("gsr_composite_backward_wide_seg", dict(C=16, pair_vis=None), INVALID),
    ("gsr_composite_backward_wide_seg", dict(C=16, segments_host=segments(), image=None), INVALID),
    ("gsr_composite_backward_wide", dict(C=17), UNSUPPORTED),
    ("gsr_composite_backward_wide", dict(C=5, final_T=None), INVALID),
    # ---- frame.hip ----
    ("gsr_frame_plan", dict(frame_host=None), INVALID),
    ("gsr_frame_plan", dict(plan_out_host=None), INVALID),
    ("gsr_frame_plan", dict(frame_host=scene_frame(N=-1, K=5)), INVALID),
    ("gsr_frame_plan", dict(frame_host=frame(W=0)), INVALID),
    ("gsr_frame_plan", dict(frame_host=frame(pair_capacity=1 << 31)), INVALID),
    ("gsr_frame_plan", dict(frame_host=scene_frame(K=5)), UNSUPPORTED),
    ("gsr_frame_plan", dict(frame_host=frame(K=5)), OK),                                  # K is not read in projected mode
    ("gsr_frame_plan", dict(frame_host=frame(C=0)), UNSUPPORTED),
    ("gsr_frame_plan", dict(frame_host=frame(C=17)), UNSUPPORTED),
    ("gsr_frame_plan", dict(frame_host=scene_frame(C=2)), UNSUPPORTED),
    ("gsr_frame_plan", dict(frame_host=frame(C=8)), UNSUPPORTED),                         # wide without a feature table
    ("gsr_frame_plan", dict(frame_host=frame(C=8, feature_table=1)), OK),
    ("gsr_frame_plan", dict(frame_host=frame(params=params(tile_size=8))), UNSUPPORTED),
    ("gsr_frame_plan", dict(frame_host=scene_frame()), OK),
    ("gsr_frame_forward", dict(frame_host=None), INVALID),
    ("gsr_frame_forward", dict(out_arena=None), INVALID),
    ("gsr_frame_forward", dict(result_out_host=None), INVALID),
    ("gsr_frame_forward", dict(frame_host=frame(N=0)), INVALID),
    ("gsr_frame_forward", dict(frame_host=frame(depth=None)), INVALID),
    ("gsr_frame_forward", dict(frame_host=scene_frame(camera_pos=None)), INVALID),
    ("gsr_frame_backward", dict(backward_host=None), INVALID),
    ("gsr_frame_backward_stages", dict(stages=0), INVALID),
    ("gsr_frame_backward_stages", dict(stages=4), INVALID),
    ("gsr_frame_backward_stages", dict(backward_host=None), INVALID),
    ("gsr_frame_backward_stages", dict(backward_host=frame_backward(M=9)), INVALID),
    ("gsr_frame_backward_stages", dict(backward_host=frame_backward(mode=3)), INVALID),
    ("gsr_frame_backward_stages", dict(backward_host=frame_backward(sh_mode=3)), INVALID),
    ("gsr_frame_backward_stages", dict(backward_host=frame_backward(grad_rows=None)), INVALID),
    ("gsr_frame_backward_stages", dict(backward_host=frame_backward(sh_mode=1, d_sh=None)), INVALID),
    ("gsr_frame_backward_stages", dict(backward_host=frame_backward(mode=2, inverse=None)), INVALID),
    ("gsr_frame_backward_stages", dict(backward_host=frame_backward(partial=None)), INVALID),
    # ---- prims.hip ----
    ("gsr_exclusive_scan_u32", dict(n=-1), INVALID),
    ("gsr_exclusive_scan_u32", dict(n=1 << 32), INVALID),
    ("gsr_exclusive_scan_u32", dict(out=None, workspace_bytes=0), INVALID),
    ("gsr_exclusive_scan_u32", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_exclusive_scan_u32", dict(n=1 << 20, workspace=None), TOO_SMALL),
    ("gsr_exclusive_scan_u32_checked", dict(overflow_dev=None), INVALID),
    ("gsr_exclusive_scan_u32_checked", dict(workspace_bytes=255), TOO_SMALL),
    ("gsr_sort_pairs_u32", dict(n=-1, workspace_bytes=0), INVALID),
    ("gsr_sort_pairs_u32", dict(end_bit=33), INVALID),
    ("gsr_sort_pairs_u32", dict(begin_bit=9, end_bit=8), INVALID),
    ("gsr_sort_pairs_u32", dict(keys_b=None), INVALID),
    ("gsr_sort_pairs_u32", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_sort_pairs_u32", dict(workspace=None), TOO_SMALL),
    ("gsr_sort_pairs_u32", dict(nulls("gsr_sort_pairs_u32", "workspace"), n=0), 0),
    ("gsr_sort_pairs2_u32", dict(vals2_a=None), INVALID),
    ("gsr_sort_pairs2_u32", dict(vals2_b=None), INVALID),
    ("gsr_sort_pairs2_u32", dict(n=0, workspace_bytes=0), TOO_SMALL),
    # ---- ssim.hip ----
    ("gsr_ssim_forward", dict(B=0), INVALID),
    ("gsr_ssim_forward", dict(crop=-1), INVALID),
    ("gsr_ssim_forward", dict(H=10, crop=5), INVALID),
    ("gsr_ssim_forward", dict(img2=None, workspace_bytes=0), INVALID),
    ("gsr_ssim_forward", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_ssim_backward", dict(W=0), INVALID),
    ("gsr_ssim_backward", dict(d_img1=None), INVALID),
    ("gsr_msloss_forward", dict(levels=0), INVALID),
    ("gsr_msloss_forward", dict(C=5), INVALID),
    ("gsr_msloss_forward", dict(levels=3), INVALID),                             # 32 >> 2 = 8 pixels: too few for the window
    ("gsr_msloss_forward", dict(lo=1.0, hi=0.0), INVALID),
    ("gsr_msloss_forward", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_msloss_backward", dict(d_image=None), INVALID),
    ("gsr_msloss_backward", dict(workspace=None), TOO_SMALL),
    ("gsr_pixel_loss_forward", dict(n=0), INVALID),
    ("gsr_pixel_loss_forward", dict(kind=2), INVALID),
    ("gsr_pixel_loss_forward", dict(lo=1.0, hi=0.0), INVALID),
    ("gsr_pixel_loss_forward", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_pixel_loss_forward", dict(image=ODD), INVALID),
    ("gsr_pixel_loss_forward", dict(image=ODD, workspace_bytes=0), TOO_SMALL),
    ("gsr_pixel_loss_backward", dict(kind=-1), INVALID),
    ("gsr_pixel_loss_backward", dict(n=0), INVALID),
    # ---- optim.hip ----
    ("gsr_opt_point_weights", dict(M=-1), INVALID),
    ("gsr_opt_point_weights", dict(nulls("gsr_opt_point_weights"), M=0), OK),
    ("gsr_opt_point_weights", dict(vis_avg=None), INVALID),
    ("gsr_opt_step", dict(D=0), INVALID),
    ("gsr_opt_step", dict(type=3, M=0), INVALID),
    ("gsr_opt_step", dict(algo=2), INVALID),
    ("gsr_opt_step", dict(type=2, D=4), INVALID),
    ("gsr_opt_step", dict(type=2, D=3, basis=None), INVALID),
    ("gsr_opt_step", dict(nulls("gsr_opt_step"), M=0, D=64, type=0), OK),
    ("gsr_opt_step", dict(exp_avg_sq=None), INVALID),
    ("gsr_point_basis", dict(M=-1), INVALID),
    ("gsr_point_basis", dict(nulls("gsr_point_basis"), M=0), OK),
    ("gsr_point_basis", dict(basis_out=None), INVALID),
    # ---- densify.hip ----
    ("gsr_point_state_add", dict(scale_cols=3), INVALID),
    ("gsr_point_state_add", dict(nulls("gsr_point_state_add"), M=0), OK),
    ("gsr_point_state_add", dict(state_max_scale_px=None), INVALID),
    ("gsr_dp_pack", dict(N=2, M=1), INVALID),
    ("gsr_dp_pack", dict(M=9), INVALID),
    ("gsr_dp_pack", dict(block_out=None), INVALID),
    ("gsr_dp_pack", dict(views_sum=None), INVALID),
    ("gsr_dp_replay", dict(stride=50), INVALID),
    ("gsr_dp_replay", dict(nulls("gsr_dp_replay"), N=0), OK),
    ("gsr_dp_replay", dict(nulls("gsr_dp_replay"), num_cameras=0), OK),
    ("gsr_dp_replay", dict(slots=None), INVALID),
    ("gsr_dp_pack_sharded", dict(slot=1), INVALID),
    ("gsr_dp_pack_sharded", dict(num_ranks=0), INVALID),
    ("gsr_dp_pack_sharded", dict(split_score=None), INVALID),
    ("gsr_dp_pack_factors_rows", dict(factors_out=None), INVALID),
    ("gsr_dp_pack_factors_rows", dict(grad_rows=None), INVALID),
    ("gsr_dp_replay_slice", dict(rank=1), INVALID),
    ("gsr_dp_replay_slice", dict(num_cameras=2), INVALID),
    ("gsr_dp_replay_slice", dict(nulls("gsr_dp_replay_slice"), N=0), OK),
    ("gsr_dp_replay_slice", dict(recv=None), INVALID),
    ("gsr_dp_finish", dict(num_ranks=0), INVALID),
    ("gsr_dp_finish", dict(nulls("gsr_dp_finish"), N=0), OK),
    ("gsr_dp_finish", dict(gathered=None), INVALID),
    ("gsr_dp_finish", dict(state_max_scale_px=None), INVALID),
    ("gsr_select_n", dict(N=-1), INVALID),
    ("gsr_select_n", dict(nulls("gsr_select_n"), N=0), OK),
    ("gsr_select_n", dict(mask_out=None), INVALID),
    ("gsr_select_n", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_compact_offsets", dict(kept_total_dev=None), INVALID),
    ("gsr_compact_offsets", dict(keep_mask=None), INVALID),
    ("gsr_compact_offsets", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_compact_columns", dict(n_columns=_lib.CONSTANTS["GSR_MAX_COLUMNS"] + 1), INVALID),
    ("gsr_compact_columns", dict(kept_total=9), INVALID),
    ("gsr_compact_columns", dict(nulls("gsr_compact_columns"), n_columns=0), OK),
    ("gsr_compact_columns", dict(columns_host=None), INVALID),
    ("gsr_compact_columns", dict(columns_host=column(width_dwords=0)), INVALID),
    ("gsr_compact_columns", dict(columns_host=column(dst=None)), INVALID),
    # ---- sh_fit.hip ----
    ("gsr_sh_fit_accumulate", dict(K=5), INVALID),
    ("gsr_sh_fit_accumulate", dict(M=9), INVALID),
    ("gsr_sh_fit_accumulate", dict(acc=None), INVALID),
    ("gsr_sh_fit_solve", dict(K=0), INVALID),
    ("gsr_sh_fit_solve", dict(ridge=0.0), INVALID),
    ("gsr_sh_fit_solve", dict(N=0), INVALID),
    # ---- neighbours.hip ----
    ("gsr_knn", dict(k=0), INVALID),
    ("gsr_knn", dict(k=_lib.KNN_MAX_K + 1, N=64), INVALID),
    ("gsr_knn", dict(k=8, N=8), INVALID),
    ("gsr_knn", dict(idx_out=None, workspace_bytes=0), INVALID),
    ("gsr_knn", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_assign_clusters", dict(K=0), INVALID),
    ("gsr_assign_clusters", dict(labels_out=None), INVALID),
    ("gsr_kmeans_iter", dict(iters=0), INVALID),
    ("gsr_kmeans_iter", dict(workspace_bytes=0), TOO_SMALL),
    # ---- color_model.hip ----
    ("gsr_color_supported", dict(model=None), UNSUPPORTED),
    ("gsr_color_supported", dict(model=color_model(S=6)), UNSUPPORTED),
    ("gsr_color_supported", dict(model=color_model(L=3)), UNSUPPORTED),
    ("gsr_color_supported", dict(model=color_model(P=40, G=40)), UNSUPPORTED),
    ("gsr_color_supported", dict(model=color_model(L=2, S=5, P=40, G=8)), OK),
    ("gsr_color_forward", dict(model=color_model(S=1), M=-1), UNSUPPORTED),
    ("gsr_color_forward", dict(M=-1), INVALID),
    ("gsr_color_forward", dict(cam_pos=None), INVALID),
    ("gsr_color_forward", dict(model=color_model(G=4), glo_feature=None), INVALID),
    ("gsr_color_forward", dict(positions=None), INVALID),
    ("gsr_color_backward", dict(model=color_model(L=0)), UNSUPPORTED),
    ("gsr_color_backward", dict(grads=None), INVALID),
    # ---- reg.hip ----
    ("gsr_reg_forward", dict(args=None), INVALID),
    ("gsr_reg_forward", dict(args=reg(M=-1)), INVALID),
    ("gsr_reg_forward", dict(args=reg(depths=None)), INVALID),
    ("gsr_reg_forward", dict(terms_out=None, workspace_bytes=0), INVALID),
    ("gsr_reg_forward", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_reg_backward", dict(d_loss=None), INVALID),
    ("gsr_reg_backward", dict(args=reg(M=0)), OK),
    ("gsr_scene_post_step", dict(N=-1), INVALID),
    ("gsr_scene_post_step", dict(nulls("gsr_scene_post_step"), N=0), OK),
    ("gsr_scene_post_step", dict(rotation_xyzw=ODD), INVALID),
    # ---- eval.hip ----
    ("gsr_color_fit", dict(P=0), INVALID),
    ("gsr_color_fit", dict(out=PTR, image=PTR, ref=PTR + 4096), INVALID),       # in place is not supported
    ("gsr_color_fit", dict(ref=PTR + 4096, out=PTR + 8192, eps=0.5), INVALID),
    ("gsr_color_fit", dict(ref=PTR + 4096, out=PTR + 8192, workspace_bytes=0), TOO_SMALL),
    ("gsr_color_fit", dict(ref=PTR + 4096, out=PTR + 8192, workspace=ODD), INVALID),
    ("gsr_image_metrics", dict(H=10), INVALID),
    ("gsr_image_metrics", dict(metrics_out=None), INVALID),
    ("gsr_image_metrics", dict(workspace_bytes=0), TOO_SMALL),
    # ---- bilagrid.hip ----
    ("gsr_bilagrid_slice_forward", dict(k=8), INVALID),
    ("gsr_bilagrid_slice_forward", dict(L=0), INVALID),
    ("gsr_bilagrid_slice_forward", dict(out=None), INVALID),
    ("gsr_bilagrid_slice_backward", dict(k=-1), INVALID),
    ("gsr_bilagrid_slice_backward", dict(d_rgb=None, d_grids=None), OK),
    ("gsr_bilagrid_slice_backward", dict(workspace_bytes=0), TOO_SMALL),
    ("gsr_bilagrid_tv", dict(N=0), INVALID),
    ("gsr_bilagrid_tv", dict(workspace=None), TOO_SMALL),
    # ---- visibility.hip, filter3d.hip, controller.hip, camera_table.hip, histogram.hip ----
    ("gsr_frustum_counts", dict(N=0), INVALID),
    ("gsr_frustum_counts", dict(V=_lib.VISIBILITY_MAX_CAMERAS + 1), INVALID),
    ("gsr_frustum_counts", dict(point_counts_out=None, camera_counts_out=None), INVALID),
    ("gsr_view_features", dict(M=-1), INVALID),
    ("gsr_view_features", dict(cluster_range=None), INVALID),
    ("gsr_sampling_rate", dict(N=0), INVALID),
    ("gsr_sampling_rate", dict(margin=-1.0), INVALID),
    ("gsr_filter3d_forward", dict(strength=-1.0), INVALID),
    ("gsr_filter3d_forward", dict(rate=ODD), INVALID),
    ("gsr_filter3d_backward", dict(d_alpha_logit=None), INVALID),
    ("gsr_filter3d_backward", dict(d_log_scaling=ODD), INVALID),
    ("gsr_mcmc_noise", dict(nulls("gsr_mcmc_noise"), N=0), OK),
    ("gsr_mcmc_noise", dict(N=-1), INVALID),
    ("gsr_mcmc_noise", dict(opacity_threshold=0.0), INVALID),
    ("gsr_mcmc_draws", dict(N=0), OK),
    ("gsr_mcmc_draws", dict(words_out=None, normals_out=None), OK),
    ("gsr_mcmc_draws", dict(N=-1), INVALID),
    ("gsr_mcmc_draws", dict(words_out=ODD), INVALID),
    ("gsr_pose_forward", dict(A_left=0), INVALID),
    ("gsr_pose_forward", dict(status=None), INVALID),
    ("gsr_pose_forward", dict(q_right=None), INVALID),                           # t_right and idx_right without q_right
    ("gsr_pose_forward", dict(nulls("gsr_pose_forward", "q_left", "t_left", "status"), B=0), OK),
    ("gsr_pose_forward", dict(T_out=ODD), INVALID),
    ("gsr_pose_backward", dict(d_T=None), INVALID),
    ("gsr_pose_backward", dict(d_t_left=None), INVALID),
    ("gsr_histogram", dict(counts=None), INVALID),
    ("gsr_histogram", dict(mode=3), INVALID),
    ("gsr_histogram", dict(num_bins=0), INVALID),
    ("gsr_histogram", dict(auto_range=0, lo=1.0, hi=0.0), INVALID),
    ("gsr_histogram", dict(values=None), INVALID),
    ("gsr_histogram", dict(workspace=ODD), INVALID),
    ("gsr_histogram", dict(workspace_bytes=0), TOO_SMALL),
]


def _label(case):
  fn, over, _ = case
  shown = {k: (type(v).__name__ if isinstance(v, (C.Structure, C.Array)) else v) for k, v in over.items()}
  return f"{fn}({', '.join(f'{k}={v}' for k, v in shown.items())})"


def test_every_source_file_is_covered():
  """The table reaches entry points of all nineteen sources (one name from each)."""
  reached = {fn for fn, _, _ in CASES}
  for fn in ("gsr_sort_pairs_u32", "gsr_sh_forward", "gsr_tile_count", "gsr_composite_forward", "gsr_frame_plan",
             "gsr_ssim_forward", "gsr_opt_step", "gsr_select_n", "gsr_bilagrid_tv", "gsr_knn", "gsr_color_forward",
             "gsr_reg_forward", "gsr_view_features", "gsr_color_fit", "gsr_filter3d_forward", "gsr_sh_fit_solve",
             "gsr_mcmc_noise", "gsr_pose_forward", "gsr_histogram", "gsr_composite_forward_wide_seg"):
    assert fn in reached


@pytest.mark.parametrize("case", CASES, ids=_label)
def test_returned_code(built_libs, case):
  fn, over, expected = case
  assert call(_lib.load(), fn, over) == expected
