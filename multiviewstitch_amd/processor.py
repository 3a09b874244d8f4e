"""``Processor::Deform`` (R/Processor/Processor.cpp:1111-1138) on files, through ``mvs_processor_deform``; the tail of
``Processor::AlignmentSeq`` (:952-1105) through ``mvs_processor_stitch_points`` / ``mvs_processor_cull_model``;
``Processor::Render`` (:1140-1192) through ``mvs_processor_render`` and its batched render ``mvs_render_depth_views``."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from .deformation import _stats, default_params


def Deform(model_obj, template_obj, parts_path, cam_R, dist_thres: float, out_obj, params: L.CParams | None = None) -> dict:
    """./Result/Model.obj + ./Template/meanbody.obj + ./Template/part/parts -> ./Result/deform.obj.
    ``cam_R`` is the rotation of cameras[0][0]; the view ray is its third row (R^T.col(2))."""
    R = L.arr(cam_R, np.float64).reshape(9)
    prm = params if params is not None else default_params()
    st = L.CStats()
    rc = L.check(L.lib().mvs_processor_deform(os.fsencode(model_obj), os.fsencode(template_obj), os.fsencode(parts_path), L.ptr(R),
                                              float(dist_thres), C.byref(prm), os.fsencode(out_obj), C.byref(st)))
    return _stats(st, rc)


def StitchPointSets(npts_paths, scales, Rs, ts, cameras, out_dir, truncate: bool = False) -> np.ndarray:
    """The tail of Processor::AlignmentSeq before Poisson (R/Processor/Processor.cpp:952-1040): each sequence's ``.npts`` culled,
    compacted and mapped forward, written to ``out_dir``/PSR%d.obj and ``out_dir``/PSR.npts.  ``cameras[k]`` lists sequence k's
    cameras.  By default sequence k keeps the reference's P_k points (the kept ones, then the untouched tail); ``truncate`` writes
    the kept points only.  -> kept counts per sequence."""
    n, s, R, t, coff, cams = L.seq_tables(scales, Rs, ts, cameras)
    if len(npts_paths) != n:
        raise L.MvsError(-1, f"{len(npts_paths)} paths for {n} sequences")
    paths = (C.c_char_p * n)(*[os.fsencode(p) for p in npts_paths])
    nk = np.empty(n, np.int64)
    L.check(L.lib().mvs_processor_stitch_points(n, paths, L.ptr(s), L.ptr(R), L.ptr(t), L.ptr(coff), cams,
                                                L.STITCH_TRUNCATE if truncate else 0, os.fsencode(out_dir), L.ptr(nk)))
    return nk


def CullPoissonModel(model_obj, scales, Rs, ts, cameras, out_obj, all_seq_proj: bool = True):
    """The trim of the Poisson model (R/Processor/Processor.cpp:1057-1105): ReadObj (normals computed when the file has no `vn`),
    the AllSeqProj cull with its facet remap, RetainConnectRegion, WriteObj.  -> (V, F) written."""
    n, s, R, t, coff, cams = L.seq_tables(scales, Rs, ts, cameras)
    V, F = C.c_int64(), C.c_int64()
    L.check(L.lib().mvs_processor_cull_model(os.fsencode(model_obj), n, L.ptr(s), L.ptr(R), L.ptr(t), L.ptr(coff), cams,
                                             int(bool(all_seq_proj)), os.fsencode(out_obj), C.byref(V), C.byref(F)))
    return V.value, F.value


def _view_tables(cameras, scales, Rs, ts):
    """seq_tables for Render / RenderViews: the SRT may be absent (None for all three: the world frame, NULL pointers)."""
    n = len(cameras)
    if scales is None and Rs is None and ts is None:
        _, _, _, _, coff, cams = L.seq_tables(np.ones(n), np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3)), cameras)
        return n, None, None, None, coff, cams
    if scales is None or Rs is None or ts is None:
        raise L.MvsError(-1, "scales, Rs and ts must all be given or all be None")
    return L.seq_tables(scales, Rs, ts, cameras)


def Render(deform_obj, srt_txt, cameras, result_dir, seq_dirs, znear: float = 0.01, zfar: float = 2000.0) -> int:
    """The second half of `main -a 0` (R/Processor/Processor.cpp:1140-1192): SRT.txt and deform.obj read through float32, the mesh
    mapped into every sequence's frame and written to ``result_dir``/render%d.obj, then every camera i of sequence k rendered to
    ``seq_dirs[k]``DATA/Render/_depth<i>.raw (cameras[0][0]'s size for every raster).  ``cameras[k]`` lists sequence k's cameras.
    -> views rendered."""
    n, _, _, _, coff, cams = _view_tables(cameras, None, None, None)
    if len(seq_dirs) != n:
        raise L.MvsError(-1, f"{len(seq_dirs)} sequence dirs for {n} sequences")
    dirs = (C.c_char_p * n)(*[os.fsencode(d) for d in seq_dirs])
    nv = C.c_int64()
    L.check(L.lib().mvs_processor_render(os.fsencode(deform_obj), os.fsencode(srt_txt), n, L.ptr(coff), cams, os.fsencode(result_dir), dirs,
                                         float(znear), float(zfar), C.byref(nv)))
    return nv.value


def RenderViews(points, facets, cameras, scales=None, Rs=None, ts=None, znear: float = 0.01, zfar: float = 2000.0,
                out_dev: int | None = None, stream: int | None = None):
    """Model2Depth::SetInput + Run (R/Model2Depth/Model2Depth.cpp:58-190): every camera of every sequence in one call.  Sequence k
    renders the points mapped by its inverse SRT (1/s_k R_k^T (p - t_k)); without an SRT the points as given.  ``cameras[k]`` lists
    sequence k's cameras; cameras[0][0]'s size (w0, h0) is the viewport of every view.  -> float32 [N, h0, w0] of inverse depths in
    camera order.  With ``out_dev`` (device address of N*h0*w0 floats) the mesh arguments are device addresses, (address, count)
    tuples as for RenderDepth, and nothing is returned."""
    n, s, R, t, coff, cams = _view_tables(cameras, scales, Rs, ts)
    if out_dev is not None:
        (pp, V), (fp, F) = points, facets
        L.check(L.lib().mvs_render_depth_views_dev(L.ptr(int(pp)), int(V), L.ptr(int(fp)), int(F), n, L.ptr(s), L.ptr(R), L.ptr(t),
                                                   L.ptr(coff), cams, float(znear), float(zfar), L.ptr(int(out_dev)), L.ptr(stream)))
        return None
    pts = L.arr(points, np.float64).reshape(-1, 3)
    fac = L.arr(facets, np.int32).reshape(-1, 3)
    N = int(coff[-1])
    w0, h0 = (int(cameras[0][0].w), int(cameras[0][0].h)) if N and len(cameras[0]) else (0, 0)
    out = np.empty((N, h0, w0), np.float32)
    L.check(L.lib().mvs_render_depth_views(L.ptr(pts), len(pts), L.ptr(fac), len(fac), n, L.ptr(s), L.ptr(R), L.ptr(t), L.ptr(coff), cams,
                                           float(znear), float(zfar), L.ptr(out)))
    return out


def CheckConsistencyCore(curcam, refcams, depth, refdepths, min_dsp: float, max_dsp: float, reproj_err: int) -> np.ndarray:
    """R/Processor/Processor.cpp:72-126 — float32 raster in, filtered float32 raster out (what SaveDepth writes to DATA/CHECK)."""
    d = L.arr(depth, np.float32)
    refs = [L.arr(r, np.float32) for r in refdepths]
    ptrs = (C.c_void_p * max(1, len(refs)))(*[r.ctypes.data for r in refs])
    cams = (L.CCamera * max(1, len(refs)))(*[L.CCamera.of(c) for c in refcams])
    out = np.empty_like(d)
    cc = L.CCamera.of(curcam)
    L.check(L.lib().mvs_check_consistency(L.ptr(d), C.byref(cc), len(refs), ptrs, cams, float(min_dsp), float(max_dsp), int(reproj_err),
                                          L.ptr(out)))
    return out


def CheckConsistency(cameras, depths, min_dsp: float, max_dsp: float, reproj_err: int, out_dev: int | None = None, stream: int | None = None):
    """R/Processor/Processor.cpp:29-70 for one sequence: every frame against its two neighbours.
    ``depths`` is a float32 array [n, h, w] — or a device address when ``out_dev`` (a device address) is given."""
    cams = (L.CCamera * len(cameras))(*[L.CCamera.of(c) for c in cameras])
    if out_dev is not None:
        L.check(L.lib().mvs_check_consistency_seq_dev(len(cameras), L.ptr(int(depths)), cams, float(min_dsp), float(max_dsp), int(reproj_err),
                                                      L.ptr(int(out_dev)), L.ptr(stream)))
        return None
    d = L.arr(depths, np.float32)
    out = np.empty_like(d)
    L.check(L.lib().mvs_check_consistency_seq(len(cameras), L.ptr(d), cams, float(min_dsp), float(max_dsp), int(reproj_err), L.ptr(out)))
    return out


def RenderDepth(points, facets, camera, znear: float = 0.01, zfar: float = 2000.0, out_dev: int | None = None, stream: int | None = None):
    """Model2Depth::RenderDepth for one camera (R/Model2Depth/Model2Depth.cpp:58-156) without GLUT: float32 raster [h, w]
    of inverse depths, 0 where no triangle covers the pixel.  With ``out_dev`` the mesh arguments are device addresses
    (points: V*3 float64, facets: F*3 int32 — pass (address, count) tuples) and nothing is returned."""
    cc = L.CCamera.of(camera)
    if out_dev is not None:
        (pp, V), (fp, F) = points, facets
        L.check(L.lib().mvs_render_depth_dev(L.ptr(int(pp)), int(V), L.ptr(int(fp)), int(F), C.byref(cc), float(znear), float(zfar),
                                             L.ptr(int(out_dev)), L.ptr(stream)))
        return None
    pts = L.arr(points, np.float64).reshape(-1, 3)
    fac = L.arr(facets, np.int32).reshape(-1, 3)
    out = np.empty((camera.h, camera.w), np.float32)
    L.check(L.lib().mvs_render_depth(L.ptr(pts), len(pts), L.ptr(fac), len(fac), C.byref(cc), float(znear), float(zfar), L.ptr(out)))
    return out


def MatchFilter(raw, tex1, valid1, tex2, valid2, img1, img2, ssd_win: int, ssd_err: float, sample_interval: int):
    """The duplicate / SSD / gap cascade in front of RemoveOutliers (R/Processor/Processor.cpp:644-735) for the matches
    between the generated views of one frame pair.  raw [n, 6] = (view1, u1, v1, view2, u2, v2); tex [views, h*w] int32,
    valid [h*w] uint8, img [h, w, 3] uint8.  -> (matches [m, 4] = (u1, v1, u2, v2), sizes after the three stages)."""
    raw = L.arr(raw, np.int32).reshape(-1, 6)
    tex1, tex2 = L.arr(tex1, np.int32), L.arr(tex2, np.int32)
    valid1, valid2 = L.arr(valid1, np.uint8), L.arr(valid2, np.uint8)
    img1, img2 = L.arr(img1, np.uint8), L.arr(img2, np.uint8)
    h, w = img1.shape[:2]
    prm = L.CMatchFilterParams(w, h, tex1.shape[0], int(ssd_win), float(ssd_err), int(sample_interval), 0)
    out = np.empty((max(1, len(raw)), 4), np.int32)
    n_out = C.c_int64()
    cnt = np.zeros(3, np.int64)
    L.check(L.lib().mvs_match_filter(L.ptr(raw), len(raw), L.ptr(tex1), L.ptr(valid1), L.ptr(tex2), L.ptr(valid2), L.ptr(img1), L.ptr(img2),
                                     C.byref(prm), L.ptr(out), C.byref(n_out), L.ptr(cnt)))
    return out[:n_out.value].copy(), cnt
