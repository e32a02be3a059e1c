"""ctypes binding of libpfnl_hip.so (include/pfnl_hip.h).

There is NO CPU fallback: if the shared library is missing or no gfx950 device is visible, every
compute entry point raises.  torch is imported *before* the library is loaded so that both resolve
the same ``libamdhip64.so.7`` (torch bundles one with that soname) — a torch-ROCm tensor's
``data_ptr()`` and ``torch.cuda.current_stream().cuda_stream`` can then be handed straight to the
C-ABI.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PFNL_HIP_LIB", os.path.join(_HERE, "lib", "libpfnl_hip.so"))

K_NAMES = ("nl_pack", "nl_attn", "conv0", "conv3x3", "conv1x1", "merge1", "tail")


class PFNLHipError(RuntimeError):
    """A libpfnl_hip call returned a negative status."""


class PFNLHipMissing(ImportError):
    """libpfnl_hip.so has not been built (run `python -c "import __graft_entry__ as g; g.build()"`)."""


class pfnl_config(C.Structure):
    _fields_ = [("num_frames", C.c_int32), ("scale", C.c_int32), ("mf", C.c_int32),
                ("num_block", C.c_int32), ("device_id", C.c_int32), ("reserved", C.c_int32 * 3)]


class pfnl_surface(C.Structure):
    """A frame as plane pointers with a row pitch each (include/pfnl_hip.h SURFACES)."""
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3)]


class pfnl_rect(C.Structure):
    """A rectangle of a raster in pixels (include/pfnl_hip.h PLACEMENT)."""
    _fields_ = [("y", C.c_int32), ("x", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]


class pfnl_tiling(C.Structure):
    """Tile extents, the margin and the tiles per run of a tiled forward (include/pfnl_hip.h TILES; pfnl_amd/tiles.py)."""
    _fields_ = [("tile_h", C.c_int32), ("tile_w", C.c_int32), ("pad", C.c_int32), ("batch", C.c_int32)]


class pfnl_telecine_params(C.Structure):
    """The parameters of inverse telecine (include/pfnl_hip.h TELECINE; pfnl_amd/telecine.py); comb_limit < 0: the default."""
    _fields_ = [("threshold", C.c_int), ("post", C.c_int), ("comb_limit", C.c_longlong)]


class pfnl_colour(C.Structure):
    """The colour of one edge of a session (include/pfnl_hip.h COLOUR; pfnl_amd/colour.py): matrix 0 | 1, full_range 0 | 1, PFNL_PRIM_*."""
    _fields_ = [("matrix", C.c_int), ("full_range", C.c_int), ("primaries", C.c_int)]


# name -> (restype, argtypes); exactly the symbols include/pfnl_hip.h declares
_vp, _i, _fp = C.c_void_p, C.c_int, C.POINTER(C.c_float)
_i32p, _tp = C.POINTER(C.c_int32), C.POINTER(pfnl_tiling)
SIGNATURES = {
    "pfnl_last_error": (C.c_char_p, []),
    "pfnl_version": (_i, []),
    "pfnl_device_count": (_i, [C.POINTER(_i)]),
    "pfnl_create": (_i, [C.POINTER(pfnl_config), C.POINTER(_vp)]),
    "pfnl_destroy": (_i, [_vp]),
    "pfnl_set_weight": (_i, [_vp, C.c_char_p, _vp, C.POINTER(C.c_int64), _i]),
    "pfnl_missing_weights": (_i, [_vp, C.POINTER(_i)]),
    "pfnl_finalize_weights": (_i, [_vp]),
    "pfnl_set_option": (_i, [_vp, C.c_char_p, C.c_char_p]),
    "pfnl_forward": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_forward_ensemble": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "pfnl_stream_ensemble": (_i, [_vp, _i]),
    "pfnl_op_dihedral": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_float, _vp]),
    "pfnl_op_dihedral_accum": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_float, _vp]),
    "pfnl_tile_axis": (_i, [_i, _i, _i, C.POINTER(_i), _i32p, _i32p, _i32p]),
    "pfnl_forward_tiled": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _tp, _i, _vp]),
    "pfnl_op_tile_gather": (_i, [_vp, _vp, _i, _i, _i, _i, _tp, _i, _i, _vp]),
    "pfnl_op_tile_scatter": (_i, [_vp, _vp, _i, _i, _i, _i, _tp, _i, _i, _vp]),
    "pfnl_stream_tile": (_i, [_vp, _tp]),
    "pfnl_forward_strip": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "pfnl_workspace_bytes": (_i, [_vp, _i, _i, _i, C.POINTER(C.c_size_t)]),
    "pfnl_plan": (_i, [_vp, _i, _i, _i, C.c_char_p, C.c_size_t]),
    "pfnl_get_option": (_i, [_vp, C.c_char_p, C.c_char_p, C.c_size_t]),
    "pfnl_sync": (_i, [_vp]),
    "pfnl_range_reruns": (_i, [_vp, C.POINTER(C.c_longlong)]),
    "pfnl_range_flag": (_i, [_vp, C.POINTER(_i)]),
    "pfnl_host_alloc": (_i, [C.c_size_t, C.POINTER(_vp)]),
    "pfnl_host_free": (_i, [_vp]),
    "pfnl_profile_enable": (_i, [_vp, _i]),
    "pfnl_profile_reset": (_i, [_vp]),
    "pfnl_profile_read": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pfnl_debug_tap": (_i, [_vp, C.c_char_p, _vp, C.c_size_t]),
    "pfnl_op_conv2d": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv2_grouped": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_accum": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_accum_split16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1x1_split16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1x1_stream": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1x1_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_accum_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1_conv10_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_winograd": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_split16": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_split16_sf": (_i, [_i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv_small": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv_small_pf_block": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1x1_split16_sf": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_winograd_ws": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_nonlocal": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_nonlocal_split16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_nonlocal_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_bicubic": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_blur_decimate": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_selftest_mfma": (_i, [_i]),
    "pfnl_op_nonlocal_embedded": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1_conv10_split16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1_conv10_split16_sf0": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv2_chain_sf0": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv2_chain_ex": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1_conv10_split16_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1_conv10_split16_mfma": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_accum_split16_ex": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv3x3_bf16_ex": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv1_conv10_bf16_ex": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_nonlocal_block": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv0": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv0_ex": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_conv0_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "pfnl_op_tail": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_gather_windows": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "pfnl_op_quantise_u8": (_i, [_vp, _vp, C.c_size_t, _vp]),
    "pfnl_op_quantise_u10": (_i, [_vp, _vp, C.c_size_t, _vp]),
    "pfnl_op_quantise_colour_u8": (_i, [_vp, _vp, C.c_size_t, _i, _i, _vp]),
    "pfnl_op_quantise_colour_u10": (_i, [_vp, _vp, C.c_size_t, _i, _i, _vp]),
    "pfnl_stream_colour": (_i, [_vp, C.POINTER(pfnl_colour), C.POINTER(pfnl_colour)]),
    "pfnl_colour_matrix": (_i, [_i, _i, _i32p]),
    "pfnl_colour_tables": (_i, [_i, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]),
    "pfnl_op_gather_windows_u8": (_i, [_vp, _vp, _i, C.c_longlong, C.c_longlong, _i, _i, _i, _i, _vp]),
    "pfnl_stream_open": (_i, [_vp, _i, _i, _i, _vp, C.POINTER(_vp)]),
    "pfnl_stream_push": (_i, [_vp, _vp, _i]),
    "pfnl_stream_end": (_i, [_vp]),
    "pfnl_stream_ready": (_i, [_vp, C.POINTER(_i)]),
    "pfnl_stream_pop": (_i, [_vp, _vp, _i, C.POINTER(C.c_longlong), C.POINTER(_i)]),
    "pfnl_stream_reset": (_i, [_vp]),
    "pfnl_stream_close": (_i, [_vp]),
    "pfnl_stream_next_batch": (_i, [_i, _i, C.c_longlong, _i, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(_i)]),
    "pfnl_stream_scenes": (_i, [_vp, _i, C.c_double]),
    "pfnl_stream_mark_cut": (_i, [_vp]),
    "pfnl_stream_pop_info": (_i, [_vp, C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong)]),
    "pfnl_stream_format": (_i, [_vp, _i, _i, _i, _i]),
    "pfnl_yuv_coefficients": (_i, [_i, _i, C.POINTER(C.c_int32)]),
    "pfnl_op_yuv420_to_rgb_u8": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "pfnl_op_rgb_to_yuv420_u8": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "pfnl_yuv10_coefficients": (_i, [_i, _i, C.POINTER(C.c_int32)]),
    "pfnl_op_rgb_to_yuv420_u10": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "pfnl_stream_resize": (_i, [_vp, _i, _i]),
    "pfnl_stream_push_surface": (_i, [_vp, C.POINTER(pfnl_surface), _i]),
    "pfnl_stream_pop_surface": (_i, [_vp, C.POINTER(pfnl_surface), _i, C.POINTER(C.c_longlong), C.POINTER(_i)]),
    "pfnl_op_yuv420_to_rgb_u8_surface": (_i, [C.POINTER(pfnl_surface), _i, _i, _i, _i, _i, _vp, _vp]),
    "pfnl_stream_chroma_siting": (_i, [_vp, _i, _i]),
    "pfnl_op_yuv420_to_rgb_u8_sited": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "pfnl_op_yuv420_to_rgb_u8_surface_sited": (_i, [C.POINTER(pfnl_surface), _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "pfnl_op_rgb_to_yuv420_u8_sited": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "pfnl_op_rgb_to_yuv420_u10_sited": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "pfnl_resize_max_taps": (_i, [_i, _i, C.POINTER(_i)]),
    "pfnl_resize_taps": (_i, [_i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int16)]),
    "pfnl_op_resize_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "pfnl_op_resize_u10": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "pfnl_stream_place": (_i, [_vp, _i, _i, C.POINTER(pfnl_rect), C.POINTER(pfnl_rect), C.POINTER(C.c_uint8)]),
    "pfnl_op_resize_place_u8": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(pfnl_rect), C.POINTER(pfnl_rect), C.POINTER(C.c_uint8), _vp, _vp]),
    "pfnl_op_resize_place_u10": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(pfnl_rect), C.POINTER(pfnl_rect), C.POINTER(C.c_uint16), _vp, _vp]),
    "pfnl_op_scene_sad_u8": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pfnl_op_gather_windows_u8_scenes": (_i, [_vp, _vp, _vp, _i, C.c_longlong, C.c_longlong, _i, _i, _i, _i, _vp]),
    "pfnl_stream_input_depth": (_i, [_vp, _i]),
    "pfnl_yuv10_decode_coefficients": (_i, [_i, _i, C.POINTER(C.c_int32)]),
    "pfnl_op_yuv420_to_rgb_u10_sited": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "pfnl_op_yuv420_to_rgb_u10_surface_sited": (_i, [C.POINTER(pfnl_surface), _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "pfnl_stream_chroma_format": (_i, [_vp, _i, _i]),
    "pfnl_op_yuv_to_rgb_u8_chroma": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "pfnl_op_yuv_to_rgb_u10_chroma": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "pfnl_op_yuv_to_rgb_u8_surface_chroma": (_i, [C.POINTER(pfnl_surface), _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "pfnl_op_yuv_to_rgb_u10_surface_chroma": (_i, [C.POINTER(pfnl_surface), _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "pfnl_op_rgb_to_yuv_u8_chroma": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "pfnl_op_rgb_to_yuv_u10_chroma": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "pfnl_stream_packing": (_i, [_vp, _i, _i]),
    "pfnl_op_packed_to_rgb_u8": (_i, [_vp, C.c_size_t, _i, _i, _i, _i, _i, C.c_size_t, _i, _i, _vp, _vp]),
    "pfnl_op_packed_to_rgb_u10": (_i, [_vp, C.c_size_t, _i, _i, _i, _i, _i, C.c_size_t, _i, _i, _vp, _vp]),
    "pfnl_op_rgb_to_packed_u8": (_i, [_vp, C.c_size_t, _i, _i, _i, _i, _i, C.c_size_t, _i, _i, _vp, _vp]),
    "pfnl_op_rgb_to_packed_u10": (_i, [_vp, C.c_size_t, _i, _i, _i, _i, _i, C.c_size_t, _i, _i, _vp, _vp]),
    "pfnl_stream_interlace": (_i, [_vp, _i, _i]),
    "pfnl_op_deinterlace_u8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "pfnl_op_deinterlace_u10": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "pfnl_op_deinterlace_pair_u8": (_i, [C.POINTER(_vp), _i, _i, _i, _vp, _vp]),
    "pfnl_op_deinterlace_pair_u10": (_i, [C.POINTER(_vp), _i, _i, _i, _vp, _vp]),
    "pfnl_stream_telecine": (_i, [_vp, _i, _i, C.POINTER(pfnl_telecine_params)]),
    "pfnl_stream_telecine_stats": (_i, [_vp, C.POINTER(C.c_longlong)]),
    "pfnl_telecine_deliverable": (_i, [_i, C.c_longlong, _i, C.POINTER(C.c_longlong)]),
    "pfnl_op_fieldmatch_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pfnl_op_fieldmatch_u10": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pfnl_op_telecine_frame_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(pfnl_telecine_params), _vp, _vp, _vp]),
    "pfnl_op_telecine_frame_u10": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(pfnl_telecine_params), _vp, _vp, _vp]),
    "pfnl_op_gather_windows_u10": (_i, [_vp, _vp, _i, C.c_longlong, C.c_longlong, _i, _i, _i, _i, _vp]),
    "pfnl_op_gather_windows_u10_scenes": (_i, [_vp, _vp, _vp, _i, C.c_longlong, C.c_longlong, _i, _i, _i, _i, _vp]),
    "pfnl_op_scene_sad_u10": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pfnl_op_content_box_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pfnl_op_content_box_u10": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pfnl_stream_bars": (_i, [_vp, _i, _i]),
    "pfnl_stream_pop_box": (_i, [_vp, C.POINTER(C.c_int32)]),
    "pfnl_stream_content_box": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_longlong)]),
    "pfnl_op_score_scratch_bytes": (_i, [_i, _i, _i, C.POINTER(C.c_size_t)]),
    "pfnl_op_score_y": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pfnl_comm_get_unique_id": (_i, [_vp]),
    "pfnl_comm_init_rank": (_i, [_i, _i, _vp, _i, C.POINTER(_vp)]),
    "pfnl_comm_init_all": (_i, [_i, C.POINTER(_i), C.POINTER(_vp)]),
    "pfnl_comm_destroy": (_i, [_vp]),
    "pfnl_comm_rank": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "pfnl_comm_bcast_weights": (_i, [_vp, _vp, _i]),
    "pfnl_copy_weights": (_i, [_vp, _vp]),
    "pfnl_comm_bcast": (_i, [_vp, _vp, C.c_size_t, _i]),
    "pfnl_comm_allreduce_f64": (_i, [_vp, C.POINTER(C.c_double), _i, _i]),
    "pfnl_comm_barrier": (_i, [_vp]),
    "pfnl_comm_allgather": (_i, [_vp, _vp, _vp, C.c_size_t, _vp]),
}
PIXEL_FORMATS = {"rgb24": 0, "nv12": 1, "i420": 2, "rgb10": 3, "p010": 4, "i010": 5}   # PFNL_PIX_*
TEN_BIT_FORMATS = ("rgb10", "p010", "i010")                # uint16 samples; names of out_format (10-bit input: in_depth)
FORMATS_420 = ("nv12", "i420", "p010", "i010")             # H * W * 3 / 2 samples, even sizes
YUV_MATRICES = {"bt601": 0, "bt709": 1}                    # PFNL_MATRIX_*
CHROMA_FORMATS = {"420": 0, "422": 1, "444": 2}            # PFNL_CHROMA_* (pfnl_amd/yuv.py CHROMAS, in its order)
CHROMA_SITINGS = {"left": 0, "center": 1, "topleft": 2}    # PFNL_SITING_* (pfnl_amd/yuv.py SITINGS, in its order)
PACKINGS = {"none": 0, "bgr24": 1, "rgba": 2, "bgra": 3, "yuyv422": 4, "uyvy422": 5, "x2rgb10": 6, "x2bgr10": 7, "y210": 8,
            "v210": 9}                                     # PFNL_PACK_* (pfnl_amd/packed.py PACKINGS, in its order)
COMM_ID_BYTES = 128
COMM_SUM, COMM_MAX = 0, 1

_lib: Optional[C.CDLL] = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load (once) and type the library.  Raises PFNLHipMissing if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise PFNLHipMissing(f"{path} not found: build it with __graft_entry__.build() "
                             f"(make -C pfnl_amd/csrc); there is no CPU fallback")
    try:  # share torch's HIP runtime (same soname) when torch is present
        import torch  # noqa: F401
        # ... and, for pfnl_comm_*, torch's RCCL build (it is linked against that same runtime); comm.hip dlopens it lazily
        cand = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if os.path.exists(cand):
            os.environ.setdefault("PFNL_RCCL_LIB", cand)
    except Exception:  # pragma: no cover - torch is plumbing, not a requirement of the C-ABI
        pass
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the library does not export the symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def rect_arg(r):
    """A (y, x, h, w) tuple as the pointer argument of the placement calls; None stays NULL (the whole raster / canvas)."""
    return None if r is None else C.byref(pfnl_rect(*(int(v) for v in r)))


def check(status: int) -> None:
    if status != 0:
        msg = load_library().pfnl_last_error()
        raise PFNLHipError(f"libpfnl_hip status {status}: {msg.decode() if msg else '?'}")


def device_count() -> int:
    n = C.c_int(0)
    check(load_library().pfnl_device_count(C.byref(n)))
    return n.value
