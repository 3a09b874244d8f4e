"""ctypes loader for libmvs_hip.so (the C-ABI of include/mvs.h).

Fails loudly: a missing library is an ImportError-grade failure and a missing
GPU turns every compute call into MvsError(MVS_E_NO_DEVICE).  There is no CPU
fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmvs_hip.so")

MVS_OK = 0
STATUS = {0: "MVS_OK", -1: "MVS_E_INVALID_ARG", -2: "MVS_E_BAD_MESH", -3: "MVS_E_NONMANIFOLD",
          -4: "MVS_E_NO_DEVICE", -5: "MVS_E_HIP", -6: "MVS_E_OOM", -7: "MVS_E_SOLVER", -8: "MVS_E_STATE",
          -9: "MVS_E_DEGENERATE", -10: "MVS_E_IO", 1: "MVS_W_UNCONVERGED"}
MVS_W_UNCONVERGED = 1


class MvsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class CCamera(C.Structure):
    """struct mvs_camera (include/mvs.h) — R/Camera/Camera.h:44-49."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("w", C.c_int32), ("h", C.c_int32)]

    @classmethod
    def of(cls, cam):
        if isinstance(cam, cls):
            return cam
        c = cls()
        c.fx, c.fy, c.cx, c.cy, c.w, c.h = cam.fx, cam.fy, cam.cx, cam.cy, int(cam.w), int(cam.h)
        c.R[:] = list(np.asarray(cam.R, dtype=np.float64).reshape(9))
        c.t[:] = list(np.asarray(cam.t, dtype=np.float64).reshape(3))
        return c


class CParams(C.Structure):
    """struct mvs_deform_params."""
    _fields_ = [("proj_len_err", C.c_double), ("proj_dist_err", C.c_double), ("min_cos", C.c_double),
                ("max_result", C.c_int32), ("top_k", C.c_int32), ("graph_k", C.c_int32),
                ("smooth_sweeps", C.c_int32), ("arap_iters", C.c_int32),
                ("arap_tol", C.c_double), ("cg_tol", C.c_double),
                ("cg_max_iters", C.c_int32), ("update_normals", C.c_int32), ("solver", C.c_int32), ("reserved0", C.c_int32)]


class CMatchFilterParams(C.Structure):
    """struct mvs_match_filter_params."""
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("view_count", C.c_int32), ("ssd_win", C.c_int32), ("ssd_err", C.c_double),
                ("sample_interval", C.c_int32), ("reserved", C.c_int32)]


class CSiftMatchParams(C.Structure):
    """struct mvs_sift_match_params."""
    _fields_ = [("view_count", C.c_int32), ("max_sift", C.c_int32), ("distmax", C.c_double), ("ratiomax", C.c_double)]


class CSiftParams(C.Structure):
    """struct mvs_sift_params."""
    _fields_ = [("first_octave", C.c_int32), ("dog_levels", C.c_int32), ("max_orient", C.c_int32), ("max_features", C.c_int32),
                ("dog_threshold", C.c_float), ("edge_threshold", C.c_float), ("sigma0", C.c_float), ("sigma_in", C.c_float),
                ("hl", C.c_double), ("hr", C.c_double), ("vl", C.c_double), ("vr", C.c_double)]


class CPointSampleParams(C.Structure):
    """struct mvs_point_sample_params."""
    _fields_ = [("dsp_min", C.c_double), ("dsp_max", C.c_double), ("max_dsp_err", C.c_double), ("min_conf", C.c_double),
                ("edge_sz_thres", C.c_double), ("pt_samp_rds", C.c_int32), ("nbr_frm_num", C.c_int32), ("nbr_frm_step", C.c_int32),
                ("reserved", C.c_int32)]


class CDepthRefineParams(C.Structure):
    """struct mvs_depth_refine_params."""
    _fields_ = [("dsp_min", C.c_double), ("dsp_max", C.c_double), ("rel_range", C.c_double), ("ssd_err", C.c_double),
                ("ssd_win", C.c_int32), ("ref_frm_count", C.c_int32), ("steps", C.c_int32), ("flags", C.c_int32)]


class CDepthRecoverParams(C.Structure):
    """struct mvs_depth_recover_params."""
    _fields_ = [("dsp_min", C.c_double), ("dsp_max", C.c_double), ("ssd_err", C.c_double), ("peak", C.c_double),
                ("ssd_win", C.c_int32), ("ref_frm_count", C.c_int32), ("levels", C.c_int32), ("min_refs", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class CDepthAggregateParams(C.Structure):
    """struct mvs_depth_aggregate_params."""
    _fields_ = [(k, C.c_int32) for k in ("p1", "p2", "cost_cap", "paths", "max_volume_mb", "reserved")]


class CColourParams(C.Structure):
    """struct mvs_colour_params."""
    _fields_ = [("min_cos", C.c_double), ("occ_tol", C.c_double), ("flags", C.c_int32), ("fill", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class CSrtRefineParams(C.Structure):
    """struct mvs_srt_refine_params."""
    _fields_ = [("rel_dist", C.c_double), ("min_cos", C.c_double), ("damping", C.c_double), ("tol", C.c_double), ("iters", C.c_int32),
                ("stride", C.c_int32), ("fixed_seq", C.c_int32), ("min_pairs", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class CJpegInfo(C.Structure):
    """struct mvs_jpeg_info_t."""
    _fields_ = [(k, C.c_int32) for k in ("w", "h", "components", "h_samp", "v_samp", "restart_interval", "n_segments", "sof")]


class CJpegEncodeParams(C.Structure):
    """struct mvs_jpeg_encode_params."""
    _fields_ = [(k, C.c_int32) for k in ("quality", "sampling", "restart_interval", "reserved")]


class CDrawPrim(C.Structure):
    """struct mvs_draw_prim (24 bytes)."""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("kind", C.c_uint8), ("size", C.c_uint8),
                ("c", C.c_uint8 * 3), ("pad", C.c_uint8 * 3)]


DRAW_PRIM_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("kind", "u1"), ("size", "u1"), ("c", "u1", (3,)),
                            ("pad", "u1", (3,))])
DRAW_DISC, DRAW_RING, DRAW_SEGMENT = 0, 1, 2          # MVS_DRAW_DISC, MVS_DRAW_RING, MVS_DRAW_SEGMENT (include/mvs.h)


class CGrabCutParams(C.Structure):
    """struct mvs_grabcut_params."""
    _fields_ = [("hl", C.c_double), ("hr", C.c_double), ("vl", C.c_double), ("vr", C.c_double), ("gamma", C.c_double),
                ("iters", C.c_int32), ("max_rounds", C.c_int32), ("reserved", C.c_int64)]


class CPoissonParams(C.Structure):
    """struct mvs_poisson_params."""
    _fields_ = [("scale", C.c_double), ("samples_per_node", C.c_double), ("solve_tol", C.c_double), ("depth_max", C.c_int32),
                ("depth_min", C.c_int32), ("max_cycles", C.c_int32), ("reserved", C.c_int32)]


class CPoissonInfo(C.Structure):
    """struct mvs_poisson_info."""
    _fields_ = [("origin", C.c_double * 3), ("h", C.c_double), ("iso", C.c_double), ("rel_residual", C.c_double), ("n_used", C.c_int64),
                ("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("depth", C.c_int32), ("cycles", C.c_int32)]


class CPoissonDensityParams(C.Structure):
    """struct mvs_poisson_density_params."""
    _fields_ = [("max_gain", C.c_double), ("flags", C.c_int32), ("density_drop", C.c_int32)]


class CPoissonDensityInfo(C.Structure):
    """struct mvs_poisson_density_info."""
    _fields_ = [("mean_density", C.c_double), ("min_point_density", C.c_double), ("max_point_density", C.c_double),
                ("density_depth", C.c_int32), ("n_clamped", C.c_int32)]


class CPoissonScreenParams(C.Structure):
    """struct mvs_poisson_screen_params."""
    _fields_ = [("alpha", C.c_double), ("reserved", C.c_int64)]


class CPoissonBandParams(C.Structure):
    """struct mvs_poisson_band_params."""
    _fields_ = [("base_depth", C.c_int32), ("band", C.c_int32), ("reserved", C.c_int32 * 2)]


POISSON_BAND_MAX_DEPTH = 10                 # MVS_POISSON_BAND_MAX_DEPTH


class CPoissonBandInfo(C.Structure):
    """struct mvs_poisson_band_info: the arrays are indexed by the level."""
    _fields_ = [("n_active_blocks", C.c_int64 * (POISSON_BAND_MAX_DEPTH + 1)), ("n_free", C.c_int64 * (POISSON_BAND_MAX_DEPTH + 1)),
                ("rel_residual", C.c_double * (POISSON_BAND_MAX_DEPTH + 1)), ("bnorm", C.c_double * (POISSON_BAND_MAX_DEPTH + 1)),
                ("iterations", C.c_int32 * (POISSON_BAND_MAX_DEPTH + 1)), ("n_open_edges", C.c_int64), ("scratch_bytes", C.c_int64),
                ("base_depth", C.c_int32), ("failed_level", C.c_int32)]


class CPoissonScreenInfo(C.Structure):
    """struct mvs_poisson_screen_info."""
    _fields_ = [("target", C.c_double), ("lambda_", C.c_double), ("rel_residual", C.c_double), ("iso_unscreened", C.c_double),
                ("occupied", C.c_int64), ("active_nodes", C.c_int64), ("cycles", C.c_int32), ("reserved", C.c_int32)]


class CPoissonBandScreenInfo(C.Structure):
    """struct mvs_poisson_band_screen_info: the arrays are indexed by the level."""
    _fields_ = [("lambda_", C.c_double * (POISSON_BAND_MAX_DEPTH + 1)), ("target", C.c_double * (POISSON_BAND_MAX_DEPTH + 1)),
                ("occupied", C.c_int64 * (POISSON_BAND_MAX_DEPTH + 1)), ("active_nodes", C.c_int64 * (POISSON_BAND_MAX_DEPTH + 1))]


class CSeqPairParams(C.Structure):
    """struct mvs_seq_pair_params."""
    _fields_ = [("filter", CMatchFilterParams), ("min_dsp", C.c_double), ("max_dsp", C.c_double), ("min_match_count", C.c_int32),
                ("ransac_iters", C.c_int32), ("pixel_err", C.c_double), ("adapt_ratio", C.c_double)]


class CStats(C.Structure):
    """struct mvs_deform_stats."""
    _fields_ = [("outer_done", C.c_int32), ("arap_iters_run", C.c_int32), ("cg_iters", C.c_int32),
                ("n_valid", C.c_int32), ("energy", C.c_double * 8), ("cg_rel_residual", C.c_double),
                ("cg_launches", C.c_int32), ("cg_active", C.c_int32),
                ("worst_rel_residual_in_batch", C.c_double), ("solves_in_batch", C.c_int32),
                ("unconverged_solves", C.c_int32), ("escalated", C.c_int32), ("reserved1", C.c_int32)]


CAND_DTYPE = np.dtype([("proj_dist", "<f8"), ("proj_len", "<f8"), ("pos", "<f8", (3,)), ("index", "<i8")])

_lib = None

# name -> (restype, argtypes); pointers are passed as c_void_p (numpy .ctypes.data or raw device addresses)
_VP, _I64, _I32, _D, _U32 = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_uint32
_SIGS = {
    "mvs_last_error": (C.c_char_p, []),
    "mvs_abi_version": (C.c_int, []),
    "mvs_device_count": (C.c_int, []),
    "mvs_set_device": (C.c_int, [_I32]),
    "mvs_trim": (C.c_int, []),
    "mvs_device_name": (C.c_int, [C.c_char_p, _I32]),
    "mvs_set_trace": (C.c_int, [_VP, _VP]),
    "mvs_set_trace_roctx": (C.c_int, [_I32]),
    "mvs_depth_to_model": (C.c_int, [_VP, _VP, _D, _D, _D, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_depth_to_model_dev": (C.c_int, [_VP, _VP, _D, _D, _D, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_depth_unproject": (C.c_int, [_VP, _VP, _D, _D, _VP, _VP]),
    "mvs_match_filter": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_match_filter_pairs": (C.c_int, [_I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_match_filter_pairs_dev": (C.c_int, [_I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_sequence_pair_srt": (C.c_int, [_I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                        _VP, _VP, _VP, _VP, _VP]),
    "mvs_gen_new_views": (C.c_int, [_I32, _VP, _VP, _I32, _I32, _D, _VP, _VP]),
    "mvs_gen_new_views_dev": (C.c_int, [_I32, _VP, _VP, _I32, _I32, _D, _VP, _VP, _VP]),
    "mvs_keypoint_cull": (C.c_int, [_I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _D, _D, _VP, _VP, _VP, _VP, _VP]),
    "mvs_keypoint_cull_dev": (C.c_int, [_I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _D, _D, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_grid_mincut": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _I32, _VP, _VP]),
    "mvs_grid_mincut_dev": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _I32, _VP, _VP, _VP]),
    "mvs_grabcut_default_params": (None, [_VP]),
    "mvs_grabcut_masks": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    "mvs_grabcut_masks_dev": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    "mvs_sift_match": (C.c_int, [_I64, _VP, _I64, _VP, _VP, _VP, _VP]),
    "mvs_sift_match_lists": (C.c_int, [_I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "mvs_sift_match_lists_dev": (C.c_int, [_I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP]),
    "mvs_sift_default_params": (None, [_VP]),
    "mvs_sift_detect": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _I64]),
    "mvs_sift_detect_dev": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "mvs_point_sample_default_params": (None, [_VP]),
    "mvs_point_sample": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64]),
    "mvs_point_sample_dev": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "mvs_depth_refine_default_params": (None, [_VP]),
    "mvs_refine_depth_maps": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_refine_depth_maps_dev": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_depth_recover_default_params": (None, [_VP]),
    "mvs_recover_depth_maps": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_recover_depth_maps_dev": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_depth_aggregate_default_params": (None, [_VP]),
    "mvs_recover_depth_maps_aggregated": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_recover_depth_maps_aggregated_dev": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_colour_default_params": (None, [_VP]),
    "mvs_colour_vertices": (C.c_int, [_VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_colour_vertices_dev": (C.c_int, [_VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_jpeg_info": (C.c_int, [_VP, _I64, _VP]),
    "mvs_jpeg_decode": (C.c_int, [_I32, _VP, _VP, _U32, _VP]),
    "mvs_jpeg_decode_dev": (C.c_int, [_I32, _VP, _VP, _U32, _VP, _VP]),
    "mvs_poisson_default_params": (None, [_VP]),
    "mvs_poisson_reconstruct": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64]),
    "mvs_poisson_reconstruct_dev": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP]),
    "mvs_poisson_density_default_params": (None, [_VP]),
    "mvs_poisson_reconstruct_density": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64]),
    "mvs_poisson_reconstruct_density_dev": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP]),
    "mvs_poisson_screen_default_params": (None, [_VP]),
    "mvs_poisson_reconstruct_screened": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64]),
    "mvs_poisson_reconstruct_screened_dev": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP]),
    "mvs_poisson_band_default_params": (None, [_VP]),
    "mvs_poisson_reconstruct_band": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64]),
    "mvs_poisson_reconstruct_band_dev": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP]),
    "mvs_poisson_reconstruct_band_density": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64]),
    "mvs_poisson_reconstruct_band_density_dev": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP]),
    "mvs_poisson_reconstruct_band_screened": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP, _VP, _VP]),
    "mvs_poisson_reconstruct_band_screened_dev": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP]),
    "mvs_mesh_trim_by_value": (C.c_int, [_I64, _VP, _VP, _I64, _VP, _VP, _D, _VP, _VP, _VP, _VP, _VP]),
    "mvs_mesh_trim_by_value_dev": (C.c_int, [_I64, _VP, _VP, _I64, _VP, _VP, _D, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_render_depth": (C.c_int, [_VP, _I64, _VP, _I64, _VP, C.c_float, C.c_float, _VP]),
    "mvs_render_depth_dev": (C.c_int, [_VP, _I64, _VP, _I64, _VP, C.c_float, C.c_float, _VP, _VP]),
    "mvs_render_depth_views": (C.c_int, [_VP, _I64, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _VP]),
    "mvs_render_depth_views_dev": (C.c_int, [_VP, _I64, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _VP, C.c_float, C.c_float, _VP, _VP]),
    "mvs_check_consistency": (C.c_int, [_VP, _VP, _I32, _VP, _VP, _D, _D, _I32, _VP]),
    "mvs_check_consistency_seq": (C.c_int, [_I32, _VP, _VP, _D, _D, _I32, _VP]),
    "mvs_check_consistency_seq_dev": (C.c_int, [_I32, _VP, _VP, _D, _D, _I32, _VP, _VP]),
    "mvs_srt_fit": (C.c_int, [_VP, _I64, _VP, _VP, _I32, _VP, _I32, _U32, _VP, _VP, _VP, _VP]),
    "mvs_srt_residual": (C.c_int, [_VP, _I64, _VP, _VP, _D, _VP, _VP, _VP, _VP]),
    "mvs_srt_remove_outliers": (C.c_int, [_VP, _I64, _VP, _VP, _I32, _D, _D, _VP, _VP, _VP, _VP]),
    "mvs_srt_make_triples": (C.c_int, [_I64, _I32, _VP, _VP]),
    "mvs_select_keyframe_pair": (C.c_int, [_I32, _I32, _VP, _VP, _VP, _VP, _I32, _I32, _D, _D, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_srt_compose": (C.c_int, [_D, _VP, _VP, _VP, _VP, _VP]),
    "mvs_srt_relative": (C.c_int, [_D, _VP, _VP, _D, _VP, _VP, _VP, _VP, _VP]),
    "mvs_srt_apply": (C.c_int, [_VP, _VP, _I64, _D, _VP, _VP, _I32, _VP, _VP]),
    "mvs_srt_apply_dev": (C.c_int, [_VP, _VP, _I64, _D, _VP, _VP, _I32, _VP, _VP, _VP]),
    "mvs_srt_refine_default_params": (None, [_VP]),
    "mvs_srt_refine": (C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_srt_refine_dev": (C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_visibility_cull": (C.c_int, [_VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP]),
    "mvs_visibility_cull_dev": (C.c_int, [_VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP]),
    "mvs_mesh_vertex_normals": (C.c_int, [_I64, _VP, _I64, _VP, _VP]),
    "mvs_mesh_vertex_normals_dev": (C.c_int, [_I64, _VP, _I64, _VP, _VP, _VP]),
    "mvs_pca": (C.c_int, [_VP, _I64, _VP, _U32, _VP, _VP, _VP, _VP]),
    "mvs_retain_connect_region": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "mvs_retain_connect_region_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "mvs_remove_ground": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _D, _VP]),
    "mvs_remove_ground_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _D, _VP]),
    "mvs_init_alignment": (C.c_int, [_VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP]),
    "mvs_init_alignment_sharded": (C.c_int, [_VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_comm_reduce": (C.c_int, [_VP, _VP, _I32, _I32]),
    "mvs_remove_ground_sharded": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _D, _VP, _VP, _I32, _VP]),
    "mvs_local_alignment_core_sharded": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _I64, _U32, _I32, _VP, _VP, _I32, _VP, _VP, _VP]),
    "mvs_part_recog": (C.c_int, [_VP, _VP, _I64, _VP, _I64, _VP]),
    "mvs_part_recog_dev": (C.c_int, [_VP, _VP, _I64, _VP, _I64, _VP]),
    "mvs_local_alignment_core": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _I64, _U32, _I32, _VP, _VP, _VP]),
    "mvs_align": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _D, _VP, _VP]),
    "mvs_align_dev": (C.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _D, _VP, _VP]),
    "mvs_deform_default_params": (None, [_VP]),
    "mvs_deform_create": (C.c_int, [_I64, _VP, _VP, _I64, _VP, _VP]),
    "mvs_deform_destroy": (C.c_int, [_VP]),
    "mvs_deform_sample_nodes": (C.c_int, [_VP, _I32, _VP]),
    "mvs_deform_set_nodes": (C.c_int, [_VP, _VP, _I64]),
    "mvs_deform_get_nodes": (C.c_int, [_VP, _VP]),
    "mvs_deform_sizes": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "mvs_deform_set_target": (C.c_int, [_VP, _I64, _VP, _VP, _I64]),
    "mvs_deform_set_target_dev": (C.c_int, [_VP, _I64, _VP, _VP, _I64]),
    "mvs_deform_iterate": (C.c_int, [_VP, _VP, _I32, _VP]),
    "mvs_deform_collect": (C.c_int, [_VP, _VP, _VP]),
    "mvs_deform_assoc_dmin": (C.c_int, [_VP, _VP, _VP]),
    "mvs_deform_assoc_select": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "mvs_deform_assoc_merge": (C.c_int, [_VP, _VP, _VP, _VP, _I32]),
    "mvs_deform_assoc_merge_packed": (C.c_int, [_VP, _VP, _VP, _I32]),
    "mvs_deform_assoc_merge_block": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I64, _I64, _I64, _VP]),
    "mvs_deform_set_node_targets_dev": (C.c_int, [_VP, _VP, _I32, _I64, _I64]),
    "mvs_deform_set_vertices": (C.c_int, [_VP, _VP, _VP]),
    "mvs_deform_solve": (C.c_int, [_VP, _VP, _VP]),
    "mvs_comm_unique_id": (C.c_int, [_VP]),
    "mvs_comm_init": (C.c_int, [_I32, _I32, _VP, _VP]),
    "mvs_comm_destroy": (C.c_int, [_VP]),
    "mvs_comm_info": (C.c_int, [_VP, _VP, _VP]),
    "mvs_comm_set_exchange": (C.c_int, [_VP, _I32]),
    "mvs_deform_iterate_sharded": (C.c_int, [_VP, _VP, _VP, _I32, _VP]),
    "mvs_deform_group_create": (C.c_int, [_VP, _I32, _VP]),
    "mvs_deform_group_iterate": (C.c_int, [_VP, _VP, _I32, _VP]),
    "mvs_deform_group_destroy": (C.c_int, [_VP]),
    "mvs_deform_sync": (C.c_int, [_VP]),
    "mvs_deform_stream": (C.c_void_p, [_VP]),
    "mvs_deform_set_stream": (C.c_int, [_VP, _VP]),
    "mvs_deform_get_vertices": (C.c_int, [_VP, _VP]),
    "mvs_deform_get_normals": (C.c_int, [_VP, _VP]),
    "mvs_deform_get_rotations": (C.c_int, [_VP, _VP]),
    "mvs_deform_get_node_targets": (C.c_int, [_VP, _I32, _VP, _VP, _VP, _VP, _VP]),
    "mvs_deform_get_node_graph": (C.c_int, [_VP, _VP]),
    "mvs_deform_compute_normals": (C.c_int, [_VP, _VP]),
    "mvs_deform_solver_info": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_knn_points": (C.c_int, [_VP, _I64, _I32, _VP]),
    "mvs_deform_arap": (C.c_int, [_VP, _VP, _VP, _VP]),
    "mvs_deform_kernel_time": (C.c_int, [_VP, C.c_char_p, _VP, _VP]),
    "mvs_deform_enable_timing": (C.c_int, [_VP, _I32]),
    # include/mvs_io.h
    "mvs_obj_read": (C.c_int, [C.c_char_p, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_obj_write": (C.c_int, [C.c_char_p, _I64, _VP, _VP, _I64, _VP]),
    "mvs_obj_write_coloured": (C.c_int, [C.c_char_p, _I64, _VP, _VP, _VP, _U32, _I64, _VP]),
    "mvs_obj_read_colours": (C.c_int, [C.c_char_p, _I64, _VP, _U32]),
    "mvs_npts_read": (C.c_int, [C.c_char_p, _VP, _VP, _VP]),
    "mvs_npts_write": (C.c_int, [C.c_char_p, _I64, _VP, _VP]),
    "mvs_srt_txt_read": (C.c_int, [C.c_char_p, _I64, _VP, _VP, _VP]),
    "mvs_srt_txt_write": (C.c_int, [C.c_char_p, _I64, _VP, _VP, _VP]),
    "mvs_jpeg_encode_default_params": (None, [_VP]),
    "mvs_jpeg_encode_bound": (C.c_int64, [_I32, _I32, _U32, _VP]),
    "mvs_jpeg_encode": (C.c_int, [_I32, _I32, _I32, _VP, _U32, _VP, _VP, _VP, _I64]),
    "mvs_jpeg_encode_dev": (C.c_int, [_I32, _I32, _I32, _VP, _U32, _VP, _VP, _VP, _I64, _VP]),
    "mvs_jpeg_roundtrip": (C.c_int, [_I32, _I32, _I32, _VP, _U32, _VP, _VP]),
    "mvs_jpeg_roundtrip_dev": (C.c_int, [_I32, _I32, _I32, _VP, _U32, _VP, _VP, _VP]),
    "mvs_depth_preview": (C.c_int, [_I32, _I32, _I32, _VP, _VP]),
    "mvs_depth_preview_dev": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP]),
    "mvs_draw_overlays": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    "mvs_draw_overlays_dev": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    "mvs_cv_rng_colours": (None, [_VP, _I64, _VP]),
    "mvs_match_overlays": (C.c_int, [_I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_match_overlays_dev": (C.c_int, [_I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_sift_overlays": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    "mvs_sift_overlays_dev": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    "mvs_processor_match_overlays": (C.c_int, [C.c_char_p, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _U32, _VP, _VP]),
    "mvs_processor_sift_overlays": (C.c_int, [C.c_char_p, C.c_char_p, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _U32, _VP]),
    "mvs_processor_save_views": (C.c_int, [C.c_char_p, _I32, _I32, _I32, _I32, _VP, _U32, _VP]),
    "mvs_processor_depth_previews": (C.c_int, [C.c_char_p, C.c_char_p, _I32, _I32, _I32, _VP]),
    "mvs_depth_raw_read": (C.c_int, [C.c_char_p, _I32, _I32, _VP]),
    "mvs_depth_raw_write": (C.c_int, [C.c_char_p, _I64, _VP]),
    "mvs_parts_read": (C.c_int, [C.c_char_p, _I64, _VP]),
    "mvs_processor_deform": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, _VP, _D, _VP, C.c_char_p, _VP]),
    "mvs_processor_stitch_points": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _U32, C.c_char_p, _VP]),
    "mvs_processor_refine_srt": (C.c_int, [_I32, _VP, C.c_char_p, _VP, C.c_char_p, _VP, _VP]),
    "mvs_processor_cull_model": (C.c_int, [C.c_char_p, _I32, _VP, _VP, _VP, _VP, _VP, _I32, C.c_char_p, _VP, _VP]),
    "mvs_processor_render": (C.c_int, [C.c_char_p, C.c_char_p, _I32, _VP, _VP, C.c_char_p, _VP, C.c_float, C.c_float, _VP]),
    "mvs_processor_refine_depths": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP]),
    "mvs_processor_load_images": (C.c_int, [_I32, _VP, _VP, _VP, _U32, _VP]),
    "mvs_processor_refine_depths_files": (C.c_int, [_I32, _VP, _VP, _VP, _VP]),
    "mvs_processor_recover_depths": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP]),
    "mvs_processor_recover_depths_files": (C.c_int, [_I32, _VP, _VP, _VP, _VP]),
    "mvs_processor_recover_depths_aggregated": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_processor_recover_depths_aggregated_files": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP]),
    "mvs_processor_colour_model": (C.c_int, [C.c_char_p, C.c_char_p, _I32, _VP, _VP, _VP, _VP, C.c_float, C.c_float, C.c_char_p, _VP]),
    "mvs_processor_point_sample": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_processor_poisson": (C.c_int, [C.c_char_p, _VP, C.c_char_p, _VP, _VP]),
    "mvs_processor_poisson_density": (C.c_int, [C.c_char_p, _VP, _VP, _D, C.c_char_p, _VP, _VP]),
    "mvs_processor_poisson_screened": (C.c_int, [C.c_char_p, _VP, _VP, _VP, _D, C.c_char_p, _VP, _VP]),
    "mvs_processor_poisson_band": (C.c_int, [C.c_char_p, _VP, _VP, C.c_char_p, _VP, _VP, _VP]),
    "mvs_processor_poisson_band_density": (C.c_int, [C.c_char_p, _VP, _VP, _VP, _D, C.c_char_p, _VP, _VP, _VP]),
    "mvs_processor_poisson_band_screened": (C.c_int, [C.c_char_p, _VP, _VP, _VP, _VP, _D, C.c_char_p, _VP, _VP, _VP]),
    # include/mvs_test.h (test hooks: per handle, not part of the drop-in ABI)
    "mvs_test_preload_wait": (C.c_int, []),
    "mvs_test_ctl": (C.c_int, [_VP, _VP, _I32]),
    "mvs_test_tail": (C.c_int, [_VP, _I32, _I32, _I32]),
    "mvs_test_group_leave": (C.c_int, [_VP, _I32]),
    "mvs_test_grid": (C.c_int, [_VP, _VP]),
    "mvs_test_sweep_steps": (C.c_int, [_VP, _I32, _VP]),
    "mvs_test_heavy_count": (C.c_int, [_VP, _VP, _VP]),
    "mvs_test_mesh_table": (C.c_int, [_VP, _I32, _VP, _VP]),
    "mvs_test_sift_scores": (C.c_int, [_I64, _VP, _I64, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_test_sift_level": (C.c_int, [_I32, _I32, _VP, _VP, _I32, _I32, _VP, _I64, _VP, _VP]),
    "mvs_test_sift_candidates": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _I64]),
    "mvs_test_point_sample_candidates": (C.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _I64]),
    "mvs_test_grabcut_trace": (C.c_int, [_I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_test_poisson_field": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _I64]),
    "mvs_test_poisson_density": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _I64]),
    "mvs_test_poisson_screened": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32]),
    "mvs_test_poisson_band_level": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _I64]),
    "mvs_test_poisson_band_density_level": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP,
                                                      _VP]),
    "mvs_test_poisson_band_screened_level": (C.c_int, [_I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP,
                                                       _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_test_jpeg_decode_timed": (C.c_int, [_I32, _VP, _VP, _U32, _VP, _VP, _VP]),
    "mvs_test_jpeg_encode_timed": (C.c_int, [_I32, _I32, _I32, _VP, _U32, _VP, _VP, _VP, _I64, _VP, _VP]),
    "mvs_test_jpeg_encode_coef": (C.c_int, [_I32, _I32, _I32, _VP, _U32, _VP, _VP, _VP, _I64]),
    "mvs_test_rotations": (C.c_int, [_I64, _VP, _I32, _VP, _VP, _VP]),
    "mvs_test_match_overlays_timed": (C.c_int, [_I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_test_srt_refine_sums": (C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mvs_test_srt_refine_timed": (C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _VP]),
}
EXPORTS = tuple(_SIGS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C multiviewstitch_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                "multiviewstitch_amd has no CPU fallback.")
        # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64, and whichever copy is mapped
        # first owns the devices (a later torch.cuda init on the other copy reports "No HIP GPUs are available"; the
        # stream handles exchanged in set_stream() are only meaningful within one runtime anyway).  Map torch's first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)          # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    """Negative statuses raise; positive ones (MVS_W_*: the call did its work, with a caveat) are returned."""
    if rc < 0:
        raise MvsError(rc, lib().mvs_last_error().decode(errors="replace"))
    return rc


CULL_SEQUENCES, CULL_ALL_SEQ = 0, 1          # enum mvs_cull_mode
STITCH_TRUNCATE = 1                         # MVS_STITCH_TRUNCATE (include/mvs_io.h)
JPEG_BGR, JPEG_RGB = 0, 1                   # MVS_JPEG_BGR, MVS_JPEG_RGB (include/mvs.h)
JPEG_GREY, JPEG_RESTART_ROW = 2, 65536      # MVS_JPEG_GREY, MVS_JPEG_RESTART_ROW
REFINE_SUBSTEP = 1                          # MVS_REFINE_SUBSTEP (include/mvs.h)
RECOVER_SUBSTEP = 1                         # MVS_RECOVER_SUBSTEP (include/mvs.h)
SGM_VOLUME_MB = 4096                        # MVS_SGM_VOLUME_MB (csrc/knobs.h): the budget behind max_volume_mb = 0; the host test pins it
SRT_REFINE_FIX_SCALE = 1                    # MVS_SRT_REFINE_FIX_SCALE (include/mvs.h)
SRT_REFINE_TERMS = 121                      # the int64 sums of one ordered pair (rule I6)
COLOUR_BEST = 1                             # MVS_COLOUR_BEST (include/mvs.h)


def cam_array(cameras):
    """``cameras`` as an mvs_camera array, at least one element long (the entries take a pointer, never an empty array)."""
    flat = [CCamera.of(c) for c in cameras]
    return (CCamera * max(1, len(flat)))(*flat)


def seq_cams(cameras):
    """cam_off int32 [n_seq + 1] and the mvs_camera array of all cameras, ``cameras[k]`` = sequence k's cameras."""
    off = np.zeros(len(cameras) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in cameras])
    return off, cam_array([c for seq in cameras for c in seq])


def seq_tables(scales, Rs, ts, cameras):
    """The SRT chain and the per-sequence camera lists of AlignmentSeq as C arrays:
    (n_seq, scales[n], R[n,3,3] row-major, t[n,3], cam_off int32[n+1], mvs_camera[]).  ``cameras[k]`` lists sequence k's cameras."""
    s = arr(scales, np.float64).reshape(-1)
    n = len(s)
    R = arr(Rs, np.float64).reshape(n, 3, 3)
    t = arr(ts, np.float64).reshape(n, 3)
    if len(cameras) != n:
        raise MvsError(-1, f"{len(cameras)} camera lists for {n} sequences")
    off, cams = seq_cams(cameras)
    return n, s, R, t, off, cams


def device_count():
    return lib().mvs_device_count()


def arr(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def ptr(a):
    """Host numpy array -> void*; None -> NULL; int -> raw (device) address; torch tensor -> its address."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(int(a) if isinstance(a, (int, np.integer)) else a.data_ptr())
