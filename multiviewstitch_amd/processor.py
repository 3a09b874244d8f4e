"""``Processor::Deform`` (R/Processor/Processor.cpp:1111-1138) on files, through ``mvs_processor_deform``; the tail of
``Processor::AlignmentSeq`` (:952-1105) through ``mvs_processor_stitch_points`` / ``mvs_processor_cull_model``;
``Processor::Render`` (:1140-1192) through ``mvs_processor_render`` and its batched render ``mvs_render_depth_views``; the refinement of
those renders against the images, DepthOptimizer::RefineAllDepthMaps (DepthRecovery/DepthOptimizer.cpp:20-43), through
``mvs_refine_depth_maps``; the first rasters DATA/_depth<i>.raw, which the reference reads (:37-38) and never writes, through
``mvs_recover_depth_maps``; the loop
over adjacent sequences of ``Processor::CalcSimilarityTransformationSeq`` (:629-826) through ``mvs_sequence_pair_srt``; its head (:524-600)
through ``mvs_gen_new_views`` (Image3D::GenNewViews) and ``mvs_keypoint_cull`` (the background cull of the key points); the descriptor
matching between them, FeatureProc::MatchFeature (R/FeatureProc/FeatureProc.cpp:77-130), through ``mvs_sift_match_lists``; the SIFT
detection in front of the cull, FeatureProc::DetectFeature (:14-75,103-112), through ``mvs_sift_detect``; the point sampling between
``CheckConsistency`` and the stitch tail, GeometryRec::RunPointSample (R/Processor/Processor.cpp:933-949), through ``mvs_point_sample``;
the surface reconstruction between the stitch tail and the trim of the model, GeometryRec::RunPoisson (:1042-1058), through
``mvs_poisson_reconstruct``; the match and SIFT overlay pictures (:767-793, :604-615, FeatureProc.cpp:67-73) through
``mvs_match_overlays`` / ``mvs_sift_overlays`` and their file forms; the colours of the stitched model from the base images, a stage the
reference does not have, through ``mvs_colour_vertices`` and ``mvs_processor_colour_model``; the refinement of the SRT chain on the
sampled points, another stage the reference does not have, through ``mvs_srt_refine`` and ``mvs_processor_refine_srt``.  The functions
stand in pipeline order."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib as L
from . import io as _io
from . import srt as _srt
from .deformation import _stats, default_params


# ------------------------------------------------------------------ helpers ----
def _stream_order(stream):
    """the context in which torch allocates and frees in the order of the caller's HIP stream (0 or None: torch's current stream)"""
    if not stream:
        return contextlib.nullcontext()
    import torch
    return torch.cuda.stream(torch.cuda.ExternalStream(int(stream)))


def _is_dev(a):
    return hasattr(a, "data_ptr")


def _dev_ptr(a, dtype, what):
    """device address of a contiguous torch tensor of the given dtype; None -> NULL"""
    if a is None:
        return None
    if not _is_dev(a) or not a.is_contiguous() or str(a.dtype).split(".")[-1] != dtype:
        raise L.MvsError(-1, f"the device form takes {what} as a contiguous {dtype} tensor")
    return L.ptr(a)


def _out_like(like, shape, dtype):
    """an uninitialised output of dtype ``dtype`` (its name) where ``like`` lives: a torch tensor on its device, or a numpy array"""
    if _is_dev(like):
        import torch
        return torch.empty(shape, dtype=getattr(torch, dtype), device=like.device)
    return np.empty(shape, dtype)


def _params(struct, default, kw):
    """``struct`` filled by the library's ``default`` function (mvs_<name>_default_params for struct mvs_<name>_params), then the
    fields of ``kw`` replaced"""
    prm = struct()
    default(C.byref(prm))
    for k, v in kw.items():
        if k not in dict(struct._fields_):
            raise L.MvsError(-1, f"{default.__name__.replace('_default', '')} has no field {k}")
        setattr(prm, k, v)
    return prm


def _call_with_capacity(call, cap, off):
    """``call(cap)`` -> (status, outputs) allocates outputs of ``cap`` rows and fills the offsets ``off``, whose last entry is the
    number of rows the call needs.  A call that reports -1 with a larger need is made exactly once more, with that need."""
    off[:] = -1
    rc, out = call(cap)
    if rc == -1 and off[-1] > cap:
        cap = int(off[-1])
        off[:] = -1
        rc, out = call(cap)
    L.check(rc)
    return out


def _view_tables(cameras, scales, Rs, ts):
    """seq_tables for Render / RenderViews: the SRT may be absent (None for all three: the world frame, NULL pointers)."""
    n = len(cameras)
    if scales is None and Rs is None and ts is None:
        return (n, None, None, None) + L.seq_cams(cameras)
    if scales is None or Rs is None or ts is None:
        raise L.MvsError(-1, "scales, Rs and ts must all be given or all be None")
    return L.seq_tables(scales, Rs, ts, cameras)


def _key_lists(keys, descs, offsets, what):
    """per-list arrays -> (offsets, flat keys, flat descs, device form?); flat device tensors with their offsets pass through"""
    if offsets is not None:
        off = L.arr(offsets, np.int64).reshape(-1)
        if _is_dev(keys) != _is_dev(descs):
            raise L.MvsError(-1, f"{what}: keys and descs must both be tensors on the GPU or both arrays")
        if not _is_dev(keys):
            keys, descs = L.arr(keys, np.float32).reshape(-1, 4), L.arr(descs, np.float32).reshape(-1, 128)
        if len(off) < 1 or len(keys) < off[-1] or len(descs) < off[-1]:
            raise L.MvsError(-1, f"{what}: keys / descs must hold key_offsets[-1] rows")
        return off, keys, descs, _is_dev(keys)
    if len(keys) != len(descs):
        raise L.MvsError(-1, f"{what}: one descriptor list per key list")
    kl = [L.arr(k, np.float32).reshape(-1, 4) for k in keys]
    dl = [L.arr(d, np.float32).reshape(-1, 128) for d in descs]
    if any(len(k) != len(d) for k, d in zip(kl, dl)):
        raise L.MvsError(-1, f"{what}: a key list and its descriptor list differ in length")
    off = np.zeros(len(kl) + 1, np.int64)
    off[1:] = np.cumsum([len(k) for k in kl])
    flat_k = np.concatenate(kl) if len(kl) else np.zeros((0, 4), np.float32)
    flat_d = np.concatenate(dl) if len(dl) else np.zeros((0, 128), np.float32)
    return off, np.ascontiguousarray(flat_k), np.ascontiguousarray(flat_d), False


def _raw_table(raw, n1, n2):
    """raw[i][j] = (n_ij, 6) int32 -> (offsets int64[n1*n2 + 1], all rows back to back), pair k = i*n2 + j."""
    flat = [L.arr(raw[i][j], np.int32).reshape(-1, 6) for i in range(n1) for j in range(n2)]
    off = np.zeros(n1 * n2 + 1, np.int64)
    off[1:] = np.cumsum([len(m) for m in flat])
    allr = np.ascontiguousarray(np.concatenate(flat)) if off[-1] else np.zeros((0, 6), np.int32)
    return off, allr


# ------------------------------------------------------------------ consistency ----
def CheckConsistencyCore(curcam, refcams, depth, refdepths, min_dsp: float, max_dsp: float, reproj_err: int) -> np.ndarray:
    """R/Processor/Processor.cpp:72-126 — float32 raster in, filtered float32 raster out (what SaveDepth writes to DATA/CHECK)."""
    d = L.arr(depth, np.float32)
    refs = [L.arr(r, np.float32) for r in refdepths]
    ptrs = (C.c_void_p * max(1, len(refs)))(*[r.ctypes.data for r in refs])
    cams = L.cam_array(refcams)
    out = np.empty_like(d)
    cc = L.CCamera.of(curcam)
    L.check(L.lib().mvs_check_consistency(L.ptr(d), C.byref(cc), len(refs), ptrs, cams, float(min_dsp), float(max_dsp), int(reproj_err),
                                          L.ptr(out)))
    return out


def CheckConsistency(cameras, depths, min_dsp: float, max_dsp: float, reproj_err: int, out_dev: int | None = None, stream: int | None = None):
    """R/Processor/Processor.cpp:29-70 for one sequence: every frame against its two neighbours.
    ``depths`` is a float32 array [n, h, w] — or a device address when ``out_dev`` (a device address) is given."""
    cams = L.cam_array(cameras)
    if out_dev is not None:
        L.check(L.lib().mvs_check_consistency_seq_dev(len(cameras), L.ptr(int(depths)), cams, float(min_dsp), float(max_dsp), int(reproj_err),
                                                      L.ptr(int(out_dev)), L.ptr(stream)))
        return None
    d = L.arr(depths, np.float32)
    out = np.empty_like(d)
    L.check(L.lib().mvs_check_consistency_seq(len(cameras), L.ptr(d), cams, float(min_dsp), float(max_dsp), int(reproj_err), L.ptr(out)))
    return out


# ------------------------------------------------------------------ point sample ----
def point_sample_params(**kw) -> L.CPointSampleParams:
    """``mvs_point_sample_default_params`` (config.txt: MinDsp 0.0025, MaxDsp 0.3, MaxDspErr 0.01, MinConf 0.9, EdgeSzThres 4, PtSampRds 2,
    NbrFrmNum 2, NbrFrmStep 1) with the given fields replaced."""
    return _params(L.CPointSampleParams, L.lib().mvs_point_sample_default_params, kw)


def RunPointSample(cameras, depths, params: L.CPointSampleParams | None = None, stream: int | None = None, capacity: int | None = None):
    """GeometryRec::RunPointSample (R/Processor/Processor.cpp:933-949) for every sequence in one call (``mvs_point_sample``; the rules,
    this library's definition: include/mvs.h).  ``cameras[k]`` lists sequence k's cameras; ``depths[k]`` is its checked rasters
    [frames, h, w] float32 (``CheckConsistency``'s result) — numpy arrays, or contiguous torch tensors on the GPU (the device form: the
    results are tensors on the same device).  In the device form ``depths`` may also be ONE contiguous float32 tensor that holds the
    rasters of all cameras back to back in camera order: it is read in place, where a list of several tensors is first concatenated
    (a copy of all rasters).  ``stream`` is the HIP stream that produced the rasters (None: the legacy default stream); the kernels, the
    concatenation and the allocation of the results are all ordered on it, whatever torch's current stream is.
    -> a list with, per sequence, (points [m, 3] float64, normals [m, 3] float64, frame [m] int32, pixel [m] int32) in the order of
    rule 8: the rows ``io.write_npts`` takes.  ``capacity`` (rows) sizes the first attempt, by default two frames' worth of cells per
    sequence (later frames are mostly covered); a call that finds more points is repeated once with the right size."""
    prm = params if params is not None else point_sample_params()
    n = len(cameras)
    off, cams = L.seq_cams(cameras)
    need = sum(len(c) * int(c[0].w) * int(c[0].h) for c in cameras if len(c))
    whole = _is_dev(depths)
    if whole:
        if depths.numel() != need:
            raise L.MvsError(-1, f"depths must hold the {need} floats of all rasters")
    else:
        if len(depths) != n:
            raise L.MvsError(-1, f"{len(depths)} raster stacks for {n} sequences")
        for k in range(n):
            want = (len(cameras[k]),) + ((int(cameras[k][0].h), int(cameras[k][0].w)) if len(cameras[k]) else tuple(depths[k].shape[1:]))
            if tuple(depths[k].shape) != want:
                raise L.MvsError(-1, f"depths[{k}] must be [frames, h, w] = {want}")
    soff = np.zeros(n + 1, np.int64)
    dev = whole or (n > 0 and all(_is_dev(d) for d in depths))
    order = _stream_order(stream) if dev else contextlib.nullcontext()
    if dev:
        import torch
    r = max(1, int(prm.pt_samp_rds))
    cap = int(capacity) if capacity is not None else sum(2 * (-(-int(c[0].w) // r)) * (-(-int(c[0].h) // r)) for c in cameras if len(c))
    with order:
        if dev:
            flat = depths if whole else (torch.cat([d.reshape(-1) for d in depths]) if n > 1 else depths[0].reshape(-1))
            if flat.numel() == 0:
                flat = torch.zeros(1, dtype=torch.float32, device=flat.device)
            dptr, fn, tail = _dev_ptr(flat, "float32", "depths"), L.lib().mvs_point_sample_dev, (L.ptr(stream),)
        else:
            flat = np.concatenate([L.arr(d, np.float32).reshape(-1) for d in depths]) if n else np.zeros(1, np.float32)
            if flat.size == 0:
                flat = np.zeros(1, np.float32)
            dptr, fn, tail = L.ptr(flat), L.lib().mvs_point_sample, ()

        def call(cap):
            out = tuple(_out_like(flat, shape, dt) for shape, dt in (((cap, 3), "float64"), ((cap, 3), "float64"), (cap, "int32"), (cap, "int32")))
            return fn(n, L.ptr(off), cams, dptr, C.byref(prm), L.ptr(soff), *[L.ptr(a) for a in out], cap, *tail), out

        out = _call_with_capacity(call, max(1, cap), soff)
    return [tuple(a[soff[k]:soff[k + 1]] for a in out) for k in range(n)]


def PointSampleFiles(seq_dirs, cameras, params: L.CPointSampleParams | None = None, npts_paths=None) -> np.ndarray:
    """``mvs_processor_point_sample``: sequence k's checked rasters ``seq_dirs[k]``/DATA/CHECK/_depth<i>.raw -> ``seq_dirs[k]``/Rec/PointSample.npts
    (or ``npts_paths[k]``), the file ``StitchPointSets`` reads.  ``cameras[k]`` lists sequence k's cameras.  -> rows written per sequence."""
    n = len(cameras)
    if len(seq_dirs) != n or (npts_paths is not None and len(npts_paths) != n):
        raise L.MvsError(-1, f"{len(seq_dirs)} sequence dirs for {n} sequences")
    off, cams = L.seq_cams(cameras)
    dirs = (C.c_char_p * max(1, n))(*[os.fsencode(d) for d in seq_dirs])
    outs = (C.c_char_p * max(1, n))(*[os.fsencode(p) if p is not None else None for p in npts_paths]) if npts_paths is not None else None
    prm = params if params is not None else point_sample_params()
    cnt = np.zeros(n, np.int64)
    L.check(L.lib().mvs_processor_point_sample(n, dirs, L.ptr(off), cams, C.byref(prm), outs, L.ptr(cnt)))
    return cnt


# ------------------------------------------------------------------ views and cull ----
def GenNewViews(cameras, imgs, view_count: int, axis: int, rot_angle: float, stream: int | None = None):
    """Image3D::GenNewViews (R/Image3D/Image3D.cpp:109-222) for every frame of one sequence in one call: ``view_count`` rotated
    homography views of each base image (rotation about row ``axis`` of the camera's R, ``rot_angle`` degrees apart) and each view's
    texIndex table.  imgs [frames, h, w, 3] uint8 — a numpy array, or a contiguous torch tensor on the GPU (the device form;
    ``stream`` is then the HIP stream that produced it, and the results are tensors on the same device).
    -> (views [frames, view_count, h, w, 3] uint8, tex [frames, view_count, h*w] int32: the ``tex`` of ``MatchFilterPairs``).
    A pixel nothing paints is (0, 0, 0) with tex = -1; the views are rasters: ``JpegRoundTrip`` gives what the reference reads back from
    ``proj%d_%d.jpg``, ``SaveViews`` writes those files."""
    n = len(cameras)
    cams = L.cam_array(cameras)
    w, h = (int(cameras[0].w), int(cameras[0].h)) if n else (0, 0)
    vc = max(0, int(view_count))
    if tuple(imgs.shape) != (n, h, w, 3):
        raise L.MvsError(-1, f"imgs must be [frames = {n}, h = {h}, w = {w}, 3]")
    if _is_dev(imgs):
        iptr, fn, tail = _dev_ptr(imgs, "uint8", "imgs"), L.lib().mvs_gen_new_views_dev, (L.ptr(stream),)
    else:
        imgs = L.arr(imgs, np.uint8)
        iptr, fn, tail = L.ptr(imgs), L.lib().mvs_gen_new_views, ()
    views = _out_like(imgs, (n, vc, h, w, 3), "uint8")
    tex = _out_like(imgs, (n, vc, h * w), "int32")
    L.check(fn(n, cams, iptr, int(view_count), int(axis), float(rot_angle), L.ptr(views), L.ptr(tex), *tail))
    return views, tex


def KeypointCull(cameras, view_count: int, key_offsets, keys, descs, tex, depths, min_dsp: float, max_dsp: float, masks=None,
                 stream: int | None = None) -> dict:
    """``mvs_keypoint_cull`` on flat arrays (R/Processor/Processor.cpp:567-600): key_offsets int64 [frames*view_count + 1], keys
    [total, 4] float32 {x, y, s, o}, descs [total, 128] float32 or None, tex [frames, view_count, h*w] int32, depths [frames, h*w]
    float32, masks [frames, h*w] uint8 or None — numpy arrays, or all of them (but key_offsets) contiguous torch tensors on the GPU
    (the device form, ``stream`` = the HIP stream that produced them).
    -> dict(keep [total] uint8, out_offsets int64, keys [kept, 4], descs [kept, 128] or None), list i at out_offsets[i]:out_offsets[i+1]."""
    n = len(cameras)
    cams = L.cam_array(cameras)
    off = L.arr(key_offsets, np.int64).reshape(-1)
    if len(off) != n * int(view_count) + 1:
        raise L.MvsError(-1, "key_offsets must hold frames * view_count + 1 entries")
    total = int(off[-1])
    ooff = np.zeros(len(off), np.int64)
    if _is_dev(keys):
        ptrs = [_dev_ptr(a, dt, w) for a, dt, w in ((keys, "float32", "keys"), (descs, "float32", "descs"), (tex, "int32", "tex"),
                                                  (depths, "float32", "depths"), (masks, "uint8", "masks"))]
        fn, tail = L.lib().mvs_keypoint_cull_dev, (L.ptr(stream),)
    else:
        keys = L.arr(keys, np.float32).reshape(-1, 4)
        descs = L.arr(descs, np.float32).reshape(-1, 128) if descs is not None else None
        tex, depths = L.arr(tex, np.int32), L.arr(depths, np.float32)
        masks = L.arr(masks, np.uint8) if masks is not None else None
        npx = int(cameras[0].w) * int(cameras[0].h) if n else 0
        if len(keys) != total or (descs is not None and len(descs) != total) or tex.size != n * int(view_count) * npx or depths.size != n * npx or \
                (masks is not None and masks.size != n * npx):
            raise L.MvsError(-1, "keys / descs must hold key_offsets[-1] rows; tex, depths and masks one raster per view / frame")
        ptrs = [L.ptr(a) for a in (keys, descs, tex, depths, masks)]
        fn, tail = L.lib().mvs_keypoint_cull, ()
    keep = _out_like(keys, max(1, total), "uint8")
    ok = _out_like(keys, (max(1, total), 4), "float32")
    od = _out_like(keys, (max(1, total), 128), "float32") if descs is not None else None
    L.check(fn(n, int(view_count), cams, L.ptr(off), *ptrs[:4], float(min_dsp), float(max_dsp), ptrs[4], L.ptr(keep), L.ptr(ooff), L.ptr(ok),
               L.ptr(od), *tail))
    kept = int(ooff[-1])
    return dict(keep=keep[:total], out_offsets=ooff, keys=ok[:kept], descs=od[:kept] if od is not None else None)


def CullKeypoints(cameras, depths, tex, keys, descs, min_dsp: float, max_dsp: float, masks=None):
    """The background cull of the SIFT key points (R/Processor/Processor.cpp:567-600) for one sequence: keys[i] = [k_i, 4] float32
    {x, y, s, o} of generated view i % view_count of frame i // view_count, descs[i] = [k_i, 128] float32 (or ``descs`` None); depths
    [frames, h, w] float32, tex [frames, view_count, h*w] int32 (``GenNewViews``), masks [frames, h, w] uint8 or None (isSegment off).
    A key survives when its base pixel is mapped, valid and inside the mask, and its world point projects inside every other frame.
    -> (keys[i], descs[i] or None) with the survivors of every list in their order."""
    n = len(cameras)
    vc = int(np.asarray(tex).shape[1])
    if len(keys) != n * vc or (descs is not None and len(descs) != len(keys)):
        raise L.MvsError(-1, "one key list (and descriptor list) per frame and view")
    lists = [L.arr(k, np.float32).reshape(-1, 4) for k in keys]
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(k) for k in lists])
    flat = np.concatenate(lists) if len(lists) else np.zeros((0, 4), np.float32)
    dflat = np.concatenate([L.arr(d, np.float32).reshape(-1, 128) for d in descs]) if descs is not None else None
    r = KeypointCull(cameras, vc, off, flat, dflat, tex, depths, min_dsp, max_dsp, masks)
    o = r["out_offsets"]
    out_keys = [r["keys"][o[i]:o[i + 1]].copy() for i in range(len(lists))]
    return out_keys, ([r["descs"][o[i]:o[i + 1]].copy() for i in range(len(lists))] if descs is not None else None)


# ------------------------------------------------------------------ foreground masks ----
def grabcut_params(**kw) -> L.CGrabCutParams:
    """``mvs_grabcut_default_params`` (margins 0.1 each, gamma 50, 3 iterations, 4096 rounds per cut) with the given fields replaced;
    hl, hr, vl, vr are ParamParser's margin ratios."""
    return _params(L.CGrabCutParams, L.lib().mvs_grabcut_default_params, kw)


def GridMinCut(excess, cap, max_rounds: int = 4096, stream: int | None = None, with_rounds: bool = False):
    """``mvs_grid_mincut``: the maximal minimum-cut source set (rule G1, include/mvs.h) of every grid.  excess [n, gh, gw] int32 (above 0:
    capacity from the source, below 0: to the sink), cap [n, 8, gh, gw] int32 >= 0 in the direction order of the header — numpy arrays,
    or contiguous int32 torch tensors on the GPU (the device form; ``stream`` is then the HIP stream that produced them).
    -> source_side [n, gh, gw] uint8 (1 / 0) where the inputs live; with ``with_rounds`` also the rounds the solver took."""
    if len(excess.shape) != 3 or tuple(cap.shape) != (excess.shape[0], 8) + tuple(excess.shape[1:]):
        raise L.MvsError(-1, "excess must be [n, gh, gw] and cap [n, 8, gh, gw]")
    n, gh, gw = (int(v) for v in excess.shape)
    rounds = C.c_int32(0)
    if _is_dev(excess):
        eptr, cptr = _dev_ptr(excess, "int32", "excess"), _dev_ptr(cap, "int32", "cap")
        fn, tail = L.lib().mvs_grid_mincut_dev, (L.ptr(stream),)
    else:
        excess, cap = L.arr(excess, np.int32), L.arr(cap, np.int32)
        eptr, cptr, fn, tail = L.ptr(excess), L.ptr(cap), L.lib().mvs_grid_mincut, ()
    side = _out_like(excess, (n, gh, gw), "uint8")
    L.check(fn(n, gw, gh, eptr, cptr, int(max_rounds), L.ptr(side), C.byref(rounds), *tail))
    return (side, rounds.value) if with_rounds else side


def GrabCutMasks(imgs, params: L.CGrabCutParams | None = None, stream: int | None = None, with_half: bool = False):
    """Image3D::LoadModel's foreground masks with Segment 1 (R/Image3D/Image3D.cpp:23-51) for every frame in one call
    (``mvs_grabcut_masks``; the rules, this library's definition: include/mvs.h).  imgs [frames, h, w, 3] uint8 — a numpy array, or a
    contiguous torch tensor on the GPU (the device form; ``stream`` is then the HIP stream that produced it).
    -> masks [frames, h, w] uint8, 255 / 0: the ``masks`` of ``CullKeypoints``; with ``with_half`` also the half-size masks
    [frames, h // 2, w // 2] (1 / 0)."""
    prm = params if params is not None else grabcut_params()
    if len(imgs.shape) != 4 or imgs.shape[-1] != 3:
        raise L.MvsError(-1, "imgs must be [frames, h, w, 3]")
    n, h, w = (int(v) for v in imgs.shape[:3])
    if _is_dev(imgs):
        iptr, fn, tail = _dev_ptr(imgs, "uint8", "imgs"), L.lib().mvs_grabcut_masks_dev, (L.ptr(stream),)
    else:
        imgs = L.arr(imgs, np.uint8)
        iptr, fn, tail = L.ptr(imgs), L.lib().mvs_grabcut_masks, ()
    mask = _out_like(imgs, (n, h, w), "uint8")
    half = _out_like(imgs, (n, max(1, h // 2), max(1, w // 2)), "uint8") if with_half else None
    L.check(fn(n, w, h, iptr, C.byref(prm), L.ptr(mask), L.ptr(half), *tail))
    return (mask, half) if with_half else mask


# ------------------------------------------------------------------ SIFT ----
def sift_params(**kw) -> L.CSiftParams:
    """``mvs_sift_default_params`` (first_octave -1, 3 DoG levels, 2 orientations, thresholds 0.02 / 10, sigma 1.6 / 0.5, no margins,
    no feature cap) with the given fields replaced; hl, hr, vl, vr are ParamParser's margin ratios."""
    return _params(L.CSiftParams, L.lib().mvs_sift_default_params, kw)


def DetectFeature(views, params: L.CSiftParams | None = None, stream: int | None = None, capacity: int | None = None):
    """FeatureProc::DetectFeature (R/FeatureProc/FeatureProc.cpp:14-75,103-112) for every raster of ``views`` [..., h, w, 3] uint8 in one
    call (``mvs_sift_detect``; the rules: include/mvs.h).  Every leading index is a list, in memory order: the views of ``GenNewViews``
    give list frame * view_count + view, what ``CullKeypoints`` and ``KeypointCull`` expect.
    A numpy array -> (keys[l] = [k_l, 4] float32 {x, y, s, o}, descs[l] = [k_l, 128] float32).  A contiguous torch tensor on the GPU (the
    device form; ``stream`` is then the HIP stream that produced it) -> (key_offsets int64 [lists + 1], keys [total, 4], descs [total, 128])
    with keys and descs tensors on the same device: the flat form of ``KeypointCull`` and ``MatchFeature``.  ``capacity`` (rows) sizes
    the first attempt; a call that finds more keys is repeated once with the right size."""
    prm = params if params is not None else sift_params()
    if len(views.shape) < 3 or views.shape[-1] != 3:
        raise L.MvsError(-1, "views must be [..., h, w, 3]")
    h, w = int(views.shape[-3]), int(views.shape[-2])
    n = int(np.prod(views.shape[:-3], dtype=np.int64))
    off = np.zeros(n + 1, np.int64)
    dev = _is_dev(views)
    if not dev:
        views = L.arr(views, np.uint8)

    def call(cap):
        keys, descs = _out_like(views, (cap, 4), "float32"), _out_like(views, (cap, 128), "float32")
        if dev:
            rc = L.lib().mvs_sift_detect_dev(n, w, h, _dev_ptr(views, "uint8", "views"), C.byref(prm), L.ptr(off), L.ptr(keys), L.ptr(descs), cap, L.ptr(stream))
        else:
            rc = L.lib().mvs_sift_detect(n, w, h, L.ptr(views), C.byref(prm), L.ptr(off), L.ptr(keys), L.ptr(descs), cap)
        return rc, (keys, descs)

    keys, descs = _call_with_capacity(call, max(1, int(capacity) if capacity is not None else n * min(int(prm.max_features), 2048)), off)
    total = int(off[-1])
    if dev:
        return off, keys[:total], descs[:total]
    return [keys[off[i]:off[i + 1]].copy() for i in range(n)], [descs[off[i]:off[i + 1]].copy() for i in range(n)]


def DetectFeatureSingleView(img, params: L.CSiftParams | None = None):
    """FeatureProc::DetectFeatureSingleView for one raster [h, w, 3] uint8 -> (keys [k, 4], descs [k, 128])."""
    keys, descs = DetectFeature(L.arr(img, np.uint8)[None], params)
    return keys[0], descs[0]


def LoadSequenceModels(cameras, imgs, depths, view_count: int, axis: int, rot_angle: float, sift: L.CSiftParams | None = None,
                       min_dsp: float | None = None, max_dsp: float | None = None, masks=None, segment: L.CGrabCutParams | None = None,
                       jpeg_quality: int | None = None) -> dict:
    """The model loop of Processor::CalcSimilarityTransformationSeq for one sequence (R/Processor/Processor.cpp:524-547, LoadModel's
    GenNewViews): -> dict(cameras, depths, tex, imgs, views).  With ``sift`` (``sift_params(...)``; then ``min_dsp`` / ``max_dsp`` are
    required, ``masks`` optional) the head of the function runs to its end (:562-600): ``DetectFeature`` on the generated views and
    ``CullKeypoints`` on its keys; the result also holds ``keys`` and ``descs`` (per list), a complete ``sequences[k]`` entry from which
    ``CalcSimilarityTransformationSeq`` makes ``raw`` itself.  Without ``sift`` the entry lacks ``raw`` (or ``keys`` / ``descs``), which
    the caller then supplies from a SIFT of their own on ``views``.  With ``segment`` (``grabcut_params(...)``: ParamParser's Segment 1;
    not together with ``masks``) the masks are made here, by ``GrabCutMasks`` on ``imgs``; they go to ``CullKeypoints`` and into the result
    as ``masks``.
    With ``jpeg_quality`` the views pass through ``JpegRoundTrip`` (4:2:0, no restart markers: ``cv::imwrite``'s stream at that quality)
    before ``DetectFeature`` and are returned that way: the pixels SiftGPU reads from ``proj%d_%d.jpg`` (R/FeatureProc/FeatureProc.cpp:26).
    With None nothing changes.
    This array form passes views, keys and descriptors through host memory between the three calls; a caller that wants them to stay in
    HBM chains ``mvs_gen_new_views_dev``, ``mvs_sift_detect_dev`` and ``mvs_keypoint_cull_dev`` on one stream."""
    if segment is not None and masks is not None:
        raise L.MvsError(-1, "give masks or segment, not both")
    img = L.arr(imgs, np.uint8)
    d = L.arr(depths, np.float32)
    if len(d) != len(cameras):
        raise L.MvsError(-1, "one raster per camera")
    views, tex = GenNewViews(cameras, img, view_count, axis, rot_angle)
    if jpeg_quality is not None:
        views = JpegRoundTrip(views.reshape((-1,) + views.shape[2:]), quality=jpeg_quality).reshape(views.shape)
    out = dict(cameras=list(cameras), depths=d, tex=tex, imgs=img, views=views)
    if segment is not None:
        masks = out["masks"] = GrabCutMasks(img, segment)
    if sift is not None:
        if min_dsp is None or max_dsp is None:
            raise L.MvsError(-1, "sift needs min_dsp and max_dsp for the key-point cull")
        keys, descs = DetectFeature(views, sift)
        out["keys"], out["descs"] = CullKeypoints(cameras, d, tex, keys, descs, min_dsp, max_dsp, masks)
    return out


# ------------------------------------------------------------------ match ----
def MatchFeatureSingleView(descs1, descs2, distmax: float = 0.7, ratiomax: float = 0.8, max_sift: int = 4096) -> np.ndarray:
    """SiftMatchGPU::GetSiftMatch for one list pair (R/FeatureProc/FeatureProc.cpp:77-101, in index form): descs [n, 128] float32.
    -> [m, 2] int32 (i, j), the mutual best matches for ascending i (the rules: include/mvs.h, mvs_sift_match_lists)."""
    d1, d2 = L.arr(descs1, np.float32).reshape(-1, 128), L.arr(descs2, np.float32).reshape(-1, 128)
    prm = L.CSiftMatchParams(1, int(max_sift), float(distmax), float(ratiomax))
    buf = np.empty((max(1, min(len(d1), len(d2))), 2), np.int32)
    n = C.c_int64()
    L.check(L.lib().mvs_sift_match(len(d1), L.ptr(d1), len(d2), L.ptr(d2), C.byref(prm), L.ptr(buf), C.byref(n)))
    return buf[:n.value].copy()


def MatchFeature(keys1, descs1, keys2, descs2, view_count: int, distmax: float = 0.7, ratiomax: float = 0.8, max_sift: int = 4096,
                 stream: int | None = None, key_offsets1=None, key_offsets2=None):
    """FeatureProc::MatchFeature for two adjacent sequences (R/FeatureProc/FeatureProc.cpp:114-130, call site Processor.cpp:634): every
    list of the first sequence against every list of the second in one call.  keys[l] = [k_l, 4] float32 {x, y, s, o} and descs[l] =
    [k_l, 128] float32 of list l = frame * view_count + view, as ``CullKeypoints`` returns them — or, with ``key_offsets1`` /
    ``key_offsets2`` (int64 [lists + 1]), the flat arrays of ``KeypointCull``: numpy arrays, or contiguous float32 torch tensors on
    the GPU (the device form; ``stream`` is then the HIP stream that produced them).
    -> raw[i][j] = (n_ij, 6) int32 (view1, u1, v1, view2, u2, v2) between frame i of the first and frame j of the second sequence:
    the ``raw`` of ``MatchFilterPairs`` and ``SequencePairSRT``."""
    vc = int(view_count)
    off1, k1, d1, dev1 = _key_lists(keys1, descs1, key_offsets1, "sequence 1")
    off2, k2, d2, dev2 = _key_lists(keys2, descs2, key_offsets2, "sequence 2")
    if dev1 != dev2:
        raise L.MvsError(-1, "both sequences must be in the same form")
    if vc < 1 or (len(off1) - 1) % vc or (len(off2) - 1) % vc:
        raise L.MvsError(-1, "need view_count >= 1 and view_count lists per frame")
    n1, n2 = (len(off1) - 1) // vc, (len(off2) - 1) // vc
    prm = L.CSiftMatchParams(vc, int(max_sift), float(distmax), float(ratiomax))
    if dev1:
        ptrs = [_dev_ptr(a, "float32", w) for a, w in ((k1, "keys"), (d1, "descs"), (k2, "keys"), (d2, "descs"))]
        fn, tail = L.lib().mvs_sift_match_lists_dev, (L.ptr(stream),)
    else:
        ptrs = [L.ptr(a) for a in (k1, d1, k2, d2)]
        fn, tail = L.lib().mvs_sift_match_lists, ()
    roff = np.zeros(max(1, n1 * n2) + 1, np.int64)
    cap = int(min(np.minimum(np.diff(off1), int(max_sift)).sum() * (len(off2) - 1), np.minimum(np.diff(off2), int(max_sift)).sum() * (len(off1) - 1)))
    raw = np.empty((max(1, cap), 6), np.int32)                           # a list pair cannot hold more matches than its shorter list
    L.check(fn(n1, n2, C.byref(prm), L.ptr(off1), ptrs[0], ptrs[1], L.ptr(off2), ptrs[2], ptrs[3], L.ptr(roff), L.ptr(raw), len(raw), None, *tail))
    return [[raw[roff[i * n2 + j]:roff[i * n2 + j + 1]].copy() for j in range(n2)] for i in range(n1)]


# ------------------------------------------------------------------ filter and SRT ----
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


def MatchFilterPairs(raw, tex1, valid1, tex2, valid2, imgs1, imgs2, ssd_win: int, ssd_err: float, sample_interval: int, stream: int | None = None):
    """The cascade of ``MatchFilter`` for every frame pair of two adjacent sequences in one call (R/Processor/Processor.cpp:645-735).
    raw[i][j] = (n_ij, 6) raw matches between frame i of the first sequence and frame j of the second; tex [frames, views, h*w] int32,
    valid [frames, h*w] uint8, imgs [frames, h, w, 3] uint8 — numpy arrays, or all six contiguous torch tensors on the GPU (the device
    form; ``stream`` is then the HIP stream that produced them).  -> (matches[i][j] = (m_ij, 4) int32 (u1, v1, u2, v2),
    sizes after the three stages int64 [n1, n2, 3])."""
    names = ("tex1", "valid1", "tex2", "valid2", "imgs1", "imgs2")
    types = ("int32", "uint8", "int32", "uint8", "uint8", "uint8")
    stacks = (tex1, valid1, tex2, valid2, imgs1, imgs2)
    if _is_dev(tex1):
        if any(a is None for a in stacks):
            raise L.MvsError(-1, "the device form takes six contiguous tensors")
        ptrs = [_dev_ptr(a, dt, w) for a, dt, w in zip(stacks, types, names)]
        fn, tail = L.lib().mvs_match_filter_pairs_dev, (L.ptr(stream),)
    else:
        stacks = tuple(L.arr(a, dt) for a, dt in zip(stacks, types))
        ptrs = [L.ptr(a) for a in stacks]
        fn, tail = L.lib().mvs_match_filter_pairs, ()
    n1, n2 = int(stacks[4].shape[0]), int(stacks[5].shape[0])
    h, w = int(stacks[4].shape[1]), int(stacks[4].shape[2])
    off, allr = _raw_table(raw, n1, n2)
    prm = L.CMatchFilterParams(w, h, int(stacks[0].shape[1]), int(ssd_win), float(ssd_err), int(sample_interval), 0)
    out = np.empty((max(1, len(allr)), 4), np.int32)
    ooff = np.zeros(n1 * n2 + 1, np.int64)
    cnt = np.zeros((n1, n2, 3), np.int64)
    L.check(fn(n1, n2, L.ptr(off), L.ptr(allr), *ptrs, C.byref(prm), L.ptr(out), L.ptr(ooff), L.ptr(cnt), *tail))
    return [[out[ooff[i * n2 + j]:ooff[i * n2 + j + 1]].copy() for j in range(n2)] for i in range(n1)], cnt


def SequencePairSRT(cams1, cams2, depths1, depths2, raw, tex1, tex2, imgs1, imgs2, ssd_win: int, ssd_err: float, sample_interval: int,
                    min_dsp: float, max_dsp: float, min_match_count: int = 7, ransac_iters: int = 200, pixel_err: float = 60.0,
                    adapt_ratio: float = 0.75, state: int = 1) -> dict:
    """One turn of the loop over adjacent sequences (R/Processor/Processor.cpp:629-826, SIFT matching and the match JPEGs left out):
    valid masks from the rasters, the match-filter cascade of every frame pair, the survivors lifted to 3-D, the key-frame pair
    selection and the closed-form fit on the selected pair.  depths [frames, h, w] float32; raw, tex, imgs as ``MatchFilterPairs``.
    -> dict(frm_idx1, frm_idx2, err, n_keep, pair_err, state) as ``srt.select_keyframe_pair``, plus scale, R, t, residual,
    stage_counts [n1, n2, 3] and matches = the fitted 3-D matches (n_sel, 6); raises MvsError (MVS_E_DEGENERATE) when no pair
    qualifies, as the reference exits."""
    n1, n2 = len(cams1), len(cams2)
    d1, d2 = L.arr(depths1, np.float32), L.arr(depths2, np.float32)
    tex1, tex2 = L.arr(tex1, np.int32), L.arr(tex2, np.int32)
    imgs1, imgs2 = L.arr(imgs1, np.uint8), L.arr(imgs2, np.uint8)
    if len(d1) != n1 or len(d2) != n2 or len(tex1) != n1 or len(tex2) != n2 or len(imgs1) != n1 or len(imgs2) != n2:
        raise L.MvsError(-1, "one raster, tex stack and image per camera")
    h, w = imgs1.shape[1:3]
    off, allr = _raw_table(raw, n1, n2)
    prm = L.CSeqPairParams(L.CMatchFilterParams(w, h, tex1.shape[1], int(ssd_win), float(ssd_err), int(sample_interval), 0), float(min_dsp),
                           float(max_dsp), int(min_match_count), int(ransac_iters), float(pixel_err), float(adapt_ratio))
    c1, c2 = L.cam_array(cams1), L.cam_array(cams2)
    st, f1, f2, s, res, ns = C.c_uint32(state), C.c_int32(), C.c_int32(), C.c_double(), C.c_double(), C.c_int64()
    R, t = np.empty((3, 3)), np.empty(3)
    cnt = np.zeros((n1, n2, 3), np.int64)
    nk, perr = np.zeros((n1, n2), np.int64), np.zeros((n1, n2))
    sel = np.empty((max(1, int(np.diff(off).max())), 6))
    vp = lambda x: C.cast(C.byref(x), C.c_void_p)
    L.check(L.lib().mvs_sequence_pair_srt(n1, n2, C.cast(c1, C.c_void_p), C.cast(c2, C.c_void_p), L.ptr(d1), L.ptr(d2), L.ptr(off), L.ptr(allr),
                                          L.ptr(tex1), L.ptr(tex2), L.ptr(imgs1), L.ptr(imgs2), vp(prm), vp(st), vp(f1), vp(f2), vp(s), L.ptr(R),
                                          L.ptr(t), vp(res), L.ptr(cnt), L.ptr(nk), L.ptr(perr), vp(ns), L.ptr(sel)))
    return dict(frm_idx1=f1.value, frm_idx2=f2.value, err=float(perr[f1.value, f2.value]), n_keep=nk, pair_err=perr, state=st.value,
                scale=s.value, R=R, t=t, residual=res.value, stage_counts=cnt, matches=sel[:ns.value].copy())


def _pair_match_pictures(match_dir, k, a, b, raw, params):
    """``match_dir``match<k>_<i>_<j>.jpg of sequence pair k (R/Processor/Processor.cpp:767-793) from the lists ``MatchFilterPairs`` returns for
    the pair's inputs: the valid masks as ``mvs_sequence_pair_srt`` forms them (inside [min_dsp, max_dsp], compared in double), so the
    lists are the bits the chain used; one fresh ``cv::RNG`` per sequence pair (:768)."""
    mn, mx = float(params["min_dsp"]), float(params["max_dsp"])
    valid = []
    for s in (a, b):
        d = L.arr(s["depths"], np.float32).astype(np.float64)
        valid.append((~((d < mn) | (d > mx))).astype(np.uint8).reshape(len(d), -1))
    matches, _ = MatchFilterPairs(raw, a["tex"], valid[0], b["tex"], valid[1], a["imgs"], b["imgs"], params["ssd_win"], params["ssd_err"],
                                  params["sample_interval"])
    MatchOverlayFiles(match_dir, k, a["imgs"], b["imgs"], matches)


def CalcSimilarityTransformationSeq(sequences, params: dict, state, srt_txt=None, match_dir=None):
    """The loop over adjacent sequences of Processor::CalcSimilarityTransformationSeq (R/Processor/Processor.cpp:629-826) and the chain
    AlignmentSeq makes of it (:851-871).  ``sequences[k]`` = dict(cameras, depths, tex, imgs) of sequence k, plus ``raw`` (raw[i][j],
    the matches towards sequence k + 1) for every sequence but the last; ``params`` = the keyword arguments of ``SequencePairSRT``
    (ssd_win, ssd_err, sample_interval, min_dsp, max_dsp, ...).  A sequence without ``raw`` but with ``keys`` and ``descs`` (per-list
    arrays, as ``CullKeypoints`` returns them; the next sequence must have them too) gets its ``raw`` from ``MatchFeature``, whose
    ``distmax``, ``ratiomax`` and ``max_sift`` are then taken out of ``params`` (:634).  One ``SequencePairSRT`` per adjacent pair with ONE rand() stream
    through all of them: ``state`` is the srand seed — an int, or a one-element uint32 numpy array that receives the advanced state.
    After pair k every earlier entry is composed with it (:819-823); identity is appended for the last sequence (:851-853);
    ``srt_txt`` (a path) writes the chain as SRT.txt (:855-871).  ``match_dir`` (a path; the reference's is ./Match/) writes pair k's
    match pictures match<k>_<i>_<j>.jpg (:767-793, ``MatchOverlayFiles``) in front of pair k's fit, so they exist when the fit raises, as
    in the reference.  One deviation: the reference draws the lists after ``RemoveOutliers`` for the pairs that reached it;
    ``mvs_sequence_pair_srt`` does not hand out those masks, so the pictures show every pair's list as the match filter left it.  With
    the default None nothing is drawn and nothing changes.
    -> (scales [n], Rs [n, 3, 3], ts [n, 3], select_frames [(frm_idx1, frm_idx2)] per pair): the input of ``StitchPointSets``."""
    st = int(np.asarray(state).reshape(-1)[0])
    params = dict(params)
    match = {k: params.pop(k) for k in ("distmax", "ratiomax", "max_sift") if k in params}
    scales, Rs, ts, select = [], [], [], []
    for k in range(len(sequences) - 1):
        a, b = sequences[k], sequences[k + 1]
        raw = a["raw"] if "raw" in a else MatchFeature(a["keys"], a["descs"], b["keys"], b["descs"], int(np.asarray(a["tex"]).shape[1]), **match)
        if match_dir is not None:
            _pair_match_pictures(match_dir, k, a, b, raw, params)
        r = SequencePairSRT(a["cameras"], b["cameras"], a["depths"], b["depths"], raw, a["tex"], b["tex"], a["imgs"], b["imgs"],
                            state=st, **params)
        st = r["state"]
        select.append((r["frm_idx1"], r["frm_idx2"]))
        for k0 in range(k):
            scales[k0], Rs[k0], ts[k0] = _srt.compose(r["scale"], r["R"], r["t"], scales[k0], Rs[k0], ts[k0])
        scales.append(r["scale"]); Rs.append(r["R"]); ts.append(r["t"])
    scales.append(1.0); Rs.append(np.eye(3)); ts.append(np.zeros(3))
    if isinstance(state, np.ndarray):
        state.reshape(-1)[0] = st
    scales, Rs, ts = np.array(scales), np.array(Rs).reshape(-1, 3, 3), np.array(ts).reshape(-1, 3)
    if srt_txt is not None:
        _io.write_srt_txt(srt_txt, scales, Rs, ts)
    return scales, Rs, ts, select


# ------------------------------------------------------------------ chain refinement ----
def srt_refine_params(**kw) -> L.CSrtRefineParams:
    """``mvs_srt_refine_default_params`` (rel_dist 0.02, min_cos 0.7, damping 1e-9, tol 1e-9, iters 20, stride 1, fixed_seq -1: the last,
    min_pairs 64, flags 0 — rel_dist, min_cos and min_pairs are choices nobody has measured on a real sequence) with the given fields
    replaced."""
    return _params(L.CSrtRefineParams, L.lib().mvs_srt_refine_default_params, kw)


def RefineSRT(points, normals, scales, Rs, ts, params: L.CSrtRefineParams | None = None, stream: int | None = None):
    """Joint similarity ICP of the SRT chain on the sequences' oriented points (``mvs_srt_refine``; the rules I1-I9, this library's
    definition: include/mvs.h), between ``RunPointSample`` and the stitch tail.  ``points[k]``, ``normals[k]``: sequence k's rows
    [m_k, 3] float64 in its own frame, as ``RunPointSample`` returns them — numpy arrays, or contiguous torch tensors on the GPU (the
    device form: several tensors are first concatenated; ``stream`` is the HIP stream that produced them and everything is ordered on
    it).  ``scales``, ``Rs``, ``ts``: the chain, not modified.
    -> (scales [n], Rs [n, 3, 3], ts [n, 3], report): the refined chain and report = dict(iters_done, history [iters_done, 2]: accepted
    matches and rms residual before each step in common-frame units, pair_count [n, n]: the accepted matches of the last search, queries
    of row a against the points of column b)."""
    prm = params if params is not None else srt_refine_params()
    s = L.arr(scales, np.float64).reshape(-1).copy()
    n = len(s)
    if len(points) != n or len(normals) != n:
        raise L.MvsError(-1, f"{len(points)} point sets and {len(normals)} normal sets for {n} sequences")
    R = L.arr(Rs, np.float64).reshape(n, 3, 3).copy()
    t = L.arr(ts, np.float64).reshape(n, 3).copy()
    dev = n > 0 and all(_is_dev(a) for a in list(points) + list(normals))
    if not dev and any(_is_dev(a) for a in list(points) + list(normals)):
        raise L.MvsError(-1, "points and normals must all be tensors on the GPU or all arrays")
    for k in range(n):
        if len(points[k].shape) != 2 or points[k].shape[1] != 3 or tuple(normals[k].shape) != tuple(points[k].shape):
            raise L.MvsError(-1, f"points[{k}] and normals[{k}] must both be [m, 3]")
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([int(p.shape[0]) for p in points])
    done = C.c_int32(0)
    hist = np.zeros((max(1, int(prm.iters)), 2), np.float64)
    pc = np.zeros((n, n), np.int64)
    with (_stream_order(stream) if dev else contextlib.nullcontext()):
        if dev:
            import torch
            fp = torch.cat([p for p in points]) if n > 1 else points[0]
            fn_ = torch.cat([q for q in normals]) if n > 1 else normals[0]
            if fp.numel() == 0:
                fp, fn_ = (torch.zeros((1, 3), dtype=torch.float64, device=fp.device) for _ in range(2))
            pp, pn, fn, tail = _dev_ptr(fp, "float64", "points"), _dev_ptr(fn_, "float64", "normals"), L.lib().mvs_srt_refine_dev, (L.ptr(stream),)
        else:
            fp = np.ascontiguousarray(np.concatenate([L.arr(p, np.float64) for p in points])) if n else np.zeros((1, 3))
            fn_ = np.ascontiguousarray(np.concatenate([L.arr(q, np.float64) for q in normals])) if n else np.zeros((1, 3))
            if fp.size == 0:
                fp, fn_ = np.zeros((1, 3)), np.zeros((1, 3))
            pp, pn, fn, tail = L.ptr(fp), L.ptr(fn_), L.lib().mvs_srt_refine, ()
        L.check(fn(pp, pn, L.ptr(off), n, L.ptr(s), L.ptr(R), L.ptr(t), C.byref(prm), C.byref(done), L.ptr(hist), L.ptr(pc), *tail))
    return s, R, t, dict(iters_done=done.value, history=hist[:done.value].copy(), pair_count=pc)


def RefineSRTFiles(npts_paths, srt_in, srt_out, params: L.CSrtRefineParams | None = None) -> dict:
    """``mvs_processor_refine_srt``: sequence k's ``npts_paths[k]`` (what ``PointSampleFiles`` wrote) and the chain of ``srt_in`` (SRT.txt)
    -> the refined chain in ``srt_out``, the file a caller passes on to ``StitchPointSets`` (through ``io.read_srt_txt``).
    -> dict(iters_done, history) as ``RefineSRT``."""
    prm = params if params is not None else srt_refine_params()
    n = len(npts_paths)
    paths = (C.c_char_p * max(1, n))(*[os.fsencode(p) for p in npts_paths])
    done = C.c_int32(0)
    hist = np.zeros((max(1, int(prm.iters)), 2), np.float64)
    L.check(L.lib().mvs_processor_refine_srt(n, paths, os.fsencode(srt_in), C.byref(prm), os.fsencode(srt_out), C.byref(done), L.ptr(hist)))
    return dict(iters_done=done.value, history=hist[:done.value].copy())


# ------------------------------------------------------------------ stitch tail ----
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


# ------------------------------------------------------------------ surface reconstruction ----
def poisson_params(**kw) -> L.CPoissonParams:
    """``mvs_poisson_default_params`` (scale 1.1, samples_per_node 1.5, solve_tol 1e-8, config.txt's PsnDptMax 10 and PsnDptMin 7,
    max_cycles 64) with the given fields replaced."""
    return _params(L.CPoissonParams, L.lib().mvs_poisson_default_params, kw)


def _poisson_info(info: L.CPoissonInfo) -> dict:
    return dict(origin=np.array(info.origin[:]), h=info.h, iso=info.iso, rel_residual=info.rel_residual, n_used=info.n_used,
                n_vertices=info.n_vertices, n_faces=info.n_faces, depth=info.depth, cycles=info.cycles)


def _run_poisson(points, normals, prm, dprm, stream, capacity, sprm=None):
    """the call behind ``RunPoisson`` (``dprm`` None: mvs_poisson_reconstruct), ``RunPoissonDensity`` (mvs_poisson_reconstruct_density) and
    ``RunPoissonScreened`` (``sprm`` given: mvs_poisson_reconstruct_screened), host or device form
    -> (vertices, faces, vertex density or None, info struct, density info struct or None[, screen info struct])"""
    name = "mvs_poisson_reconstruct" if dprm is None else "mvs_poisson_reconstruct_density" if sprm is None else "mvs_poisson_reconstruct_screened"
    dev = _is_dev(points)
    if dev != _is_dev(normals):
        raise L.MvsError(-1, "points and normals must both be tensors on the GPU or both arrays")
    order = _stream_order(stream) if dev else contextlib.nullcontext()
    if dev:
        import torch
        if tuple(points.shape) != tuple(normals.shape) or points.dim() != 2 or points.shape[1] != 3:
            raise L.MvsError(-1, "points and normals must be [n, 3]")
        pp, pn, n = _dev_ptr(points, "float64", "points"), _dev_ptr(normals, "float64", "normals"), int(points.shape[0])
        fn, tail = getattr(L.lib(), name + "_dev"), (L.ptr(stream),)
    else:
        points, normals = L.arr(points, np.float64).reshape(-1, 3), L.arr(normals, np.float64).reshape(-1, 3)
        if points.shape != normals.shape:
            raise L.MvsError(-1, "points and normals must be [n, 3]")
        pp, pn, n = L.ptr(points), L.ptr(normals), len(points)
        fn, tail = getattr(L.lib(), name), ()
    if n == 0:                                                  # a pointer to nothing is still a pointer
        pp = pn = L.ptr(np.zeros(3))
    if capacity is None:
        dmax = max(0, min(int(prm.depth_max), 9))
        capacity = (12 * 4 ** dmax, 24 * 4 ** dmax)
    info, dinfo = L.CPoissonInfo(), None if dprm is None else L.CPoissonDensityInfo()
    sinfo = None if sprm is None else L.CPoissonScreenInfo()
    with order:
        def call(vcap, fcap):
            v, f = _out_like(points, (max(1, vcap), 3), "float64"), _out_like(points, (max(1, fcap), 3), "int32")
            if dprm is None:
                return fn(n, pp, pn, C.byref(prm), C.byref(info), L.ptr(v), vcap, L.ptr(f), fcap, *tail), v, f, None
            d = _out_like(points, (max(1, vcap),), "float64")
            if sprm is not None:
                return fn(n, pp, pn, C.byref(prm), C.byref(dprm), C.byref(sprm), C.byref(info), C.byref(dinfo), C.byref(sinfo), L.ptr(v), L.ptr(d), vcap,
                          L.ptr(f), fcap, *tail), v, f, d
            return fn(n, pp, pn, C.byref(prm), C.byref(dprm), C.byref(info), C.byref(dinfo), L.ptr(v), L.ptr(d), vcap, L.ptr(f), fcap, *tail), v, f, d

        vcap, fcap = int(capacity[0]), int(capacity[1])
        rc, v, f, d = call(vcap, fcap)
        if rc == -1 and (info.n_vertices > vcap or info.n_faces > fcap):
            vcap, fcap = int(info.n_vertices), int(info.n_faces)
            rc, v, f, d = call(vcap, fcap)
    L.check(rc)
    out = v[:info.n_vertices], f[:info.n_faces], None if d is None else d[:info.n_vertices], info, dinfo
    return out if sprm is None else out + (sinfo,)


def RunPoisson(points, normals, params: L.CPoissonParams | None = None, stream: int | None = None, capacity: tuple | None = None):
    """GeometryRec::RunPoisson (R/Processor/Processor.cpp:1042-1058) through ``mvs_poisson_reconstruct`` (the rules, this library's
    definition: include/mvs.h).  ``points`` and ``normals`` are [n, 3] float64 — numpy arrays, or contiguous torch tensors on the GPU
    (the device form: the results are tensors on the same device, and the kernels and the allocation of the results are ordered on
    ``stream``, the HIP stream that produced the points; None: the legacy default stream).
    -> (vertices [V, 3] float64, faces [F, 3] int32, info dict: origin, h, iso, rel_residual, n_used, n_vertices, n_faces, depth, cycles).
    ``capacity`` = (vertex rows, face rows) sizes the first attempt, by default 12 * 4^Dmax vertices and twice as many faces (a closed
    surface of modest area at the finest depth the call can pick); a call that finds more is repeated once with the right sizes."""
    v, f, _, info, _ = _run_poisson(points, normals, params if params is not None else poisson_params(), None, stream, capacity)
    return v, f, _poisson_info(info)


def PoissonFiles(psr_npts, model_obj, params: L.CPoissonParams | None = None, dparams: L.CPoissonDensityParams | None = None,
                 trim_ratio: float | None = None, sparams: "L.CPoissonScreenParams | None" = None,
                 bparams: "L.CPoissonBandParams | None" = None):
    """``mvs_processor_poisson``: ``psr_npts`` (Result/PSR.npts, what ``StitchPointSets`` wrote) -> ``model_obj`` (Result/Model.obj with
    `v`, `vn` and `f` lines, what ``CullPoissonModel`` reads).  -> (V, F) written.  With ``dparams`` (``poisson_density_params``) or
    ``trim_ratio`` the call is ``mvs_processor_poisson_density``: the normals weighted by the sampling density when ``dparams`` sets
    WEIGHT_NORMALS, the mesh trimmed where its vertex density lies below ``trim_ratio`` times the mean point density.  With ``sparams``
    (``poisson_screen_params``) the call is ``mvs_processor_poisson_screened``: the field pulled to the iso value at every point.
    With ``bparams`` (``poisson_band_params``) the call is ``mvs_processor_poisson_band``, the band-refined levels up to depth 10;
    ``bparams`` with ``dparams`` AND ``trim_ratio`` (0.0: no trim) is ``mvs_processor_poisson_band_density``, those levels weighted and
    trimmed by the sampling density as above; ``bparams`` with only one of the two raises, as it did before that call existed.
    ``bparams`` together with ``sparams`` raises here: the band levels with screening are ``PoissonBandScreenedFiles``."""
    prm = params if params is not None else poisson_params()
    V, F = C.c_int64(), C.c_int64()
    if bparams is not None:
        if sparams is not None:
            raise L.MvsError(-1, "PoissonFiles: bparams cannot be combined with sparams (the band levels are unscreened)")
        if (dparams is None) != (trim_ratio is None):
            raise L.MvsError(-1, "PoissonFiles: bparams with the sampling density needs dparams and trim_ratio together (trim_ratio 0.0: no trim)")
        if dparams is not None:
            L.check(L.lib().mvs_processor_poisson_band_density(os.fsencode(psr_npts), C.byref(prm), C.byref(bparams), C.byref(dparams), float(trim_ratio),
                                                               os.fsencode(model_obj), C.byref(V), C.byref(F), None))
        else:
            L.check(L.lib().mvs_processor_poisson_band(os.fsencode(psr_npts), C.byref(prm), C.byref(bparams), os.fsencode(model_obj), C.byref(V), C.byref(F), None))
    elif sparams is not None:
        L.check(L.lib().mvs_processor_poisson_screened(os.fsencode(psr_npts), C.byref(prm), C.byref(dparams) if dparams is not None else None,
                                                       C.byref(sparams), float(trim_ratio or 0.0), os.fsencode(model_obj), C.byref(V), C.byref(F)))
    elif dparams is None and trim_ratio is None:
        L.check(L.lib().mvs_processor_poisson(os.fsencode(psr_npts), C.byref(prm), os.fsencode(model_obj), C.byref(V), C.byref(F)))
    else:
        L.check(L.lib().mvs_processor_poisson_density(os.fsencode(psr_npts), C.byref(prm), C.byref(dparams) if dparams is not None else None,
                                                      float(trim_ratio or 0.0), os.fsencode(model_obj), C.byref(V), C.byref(F)))
    return V.value, F.value


def poisson_band_params(**kw) -> L.CPoissonBandParams:
    """``mvs_poisson_band_default_params`` (base_depth 8, band 2) with the given fields replaced."""
    return _params(L.CPoissonBandParams, L.lib().mvs_poisson_band_default_params, kw)


def _poisson_band_info(binfo: L.CPoissonBandInfo) -> dict:
    return dict(n_active_blocks=list(binfo.n_active_blocks), n_free=list(binfo.n_free), rel_residual=list(binfo.rel_residual),
                bnorm=list(binfo.bnorm), iterations=list(binfo.iterations), n_open_edges=binfo.n_open_edges,
                scratch_bytes=binfo.scratch_bytes, base_depth=binfo.base_depth, failed_level=binfo.failed_level)


def _run_poisson_band(points, normals, prm, bprm, dprm, stream, capacity, sprm=None):
    """the call behind ``RunPoissonBand`` (``dprm`` None: mvs_poisson_reconstruct_band), ``RunPoissonBandDensity``
    (mvs_poisson_reconstruct_band_density) and ``RunPoissonBandScreened`` (``sprm`` given: mvs_poisson_reconstruct_band_screened), host or
    device form
    -> (vertices, faces, vertex density or None, info struct, band info struct, density info struct or None[, screen info struct, band
    screen info struct])"""
    name = "mvs_poisson_reconstruct_band" if dprm is None else "mvs_poisson_reconstruct_band_density" if sprm is None else \
        "mvs_poisson_reconstruct_band_screened"
    dev = _is_dev(points)
    if dev != _is_dev(normals):
        raise L.MvsError(-1, "points and normals must both be tensors on the GPU or both arrays")
    order = _stream_order(stream) if dev else contextlib.nullcontext()
    if dev:
        import torch
        if tuple(points.shape) != tuple(normals.shape) or points.dim() != 2 or points.shape[1] != 3:
            raise L.MvsError(-1, "points and normals must be [n, 3]")
        pp, pn, n = _dev_ptr(points, "float64", "points"), _dev_ptr(normals, "float64", "normals"), int(points.shape[0])
        fn, tail = getattr(L.lib(), name + "_dev"), (L.ptr(stream),)
    else:
        points, normals = L.arr(points, np.float64).reshape(-1, 3), L.arr(normals, np.float64).reshape(-1, 3)
        if points.shape != normals.shape:
            raise L.MvsError(-1, "points and normals must be [n, 3]")
        pp, pn, n = L.ptr(points), L.ptr(normals), len(points)
        fn, tail = getattr(L.lib(), name), ()
    nothing = np.zeros(3)                                       # a pointer to nothing is still a pointer; the name keeps it alive
    if n == 0:
        pp = pn = L.ptr(nothing)
    if capacity is None:
        dmax = max(0, min(int(prm.depth_max), L.POISSON_BAND_MAX_DEPTH))
        capacity = (12 * 4 ** dmax, 24 * 4 ** dmax)
    info, binfo, dinfo = L.CPoissonInfo(), L.CPoissonBandInfo(), None if dprm is None else L.CPoissonDensityInfo()
    sinfo, bsinfo = L.CPoissonScreenInfo(), L.CPoissonBandScreenInfo()
    screen = () if sprm is None else (C.byref(sprm), C.byref(sinfo), C.byref(bsinfo))
    with order:
        def call(vcap, fcap):
            # v, f and d are named here and returned: the addresses handed to the library stay those of live arrays
            v, f = _out_like(points, (max(1, vcap), 3), "float64"), _out_like(points, (max(1, fcap), 3), "int32")
            if dprm is None:
                return fn(n, pp, pn, C.byref(prm), C.byref(bprm), C.byref(info), C.byref(binfo), L.ptr(v), vcap, L.ptr(f), fcap, *tail), v, f, None
            d = _out_like(points, (max(1, vcap),), "float64")
            rc = fn(n, pp, pn, C.byref(prm), C.byref(bprm), C.byref(dprm), C.byref(info), C.byref(binfo), C.byref(dinfo), L.ptr(v), L.ptr(d), vcap,
                    L.ptr(f), fcap, *tail, *screen)
            return rc, v, f, d

        vcap, fcap = int(capacity[0]), int(capacity[1])
        rc, v, f, d = call(vcap, fcap)
        if rc == -1 and (info.n_vertices > vcap or info.n_faces > fcap):
            vcap, fcap = int(info.n_vertices), int(info.n_faces)
            rc, v, f, d = call(vcap, fcap)
    try:
        L.check(rc)
    except L.MvsError as e:
        e.info, e.band_info = _poisson_info(info), _poisson_band_info(binfo)
        raise
    out = v[:info.n_vertices], f[:info.n_faces], None if d is None else d[:info.n_vertices], info, binfo, dinfo
    return out if sprm is None else out + (sinfo, bsinfo)


def RunPoissonBand(points, normals, params: L.CPoissonParams | None = None, bparams: L.CPoissonBandParams | None = None,
                   stream: int | None = None, capacity: tuple | None = None):
    """``mvs_poisson_reconstruct_band`` (rules 24-31 of include/mvs.h, this library's definition): a dense base level of depth
    ``bparams.base_depth`` refined level by level on the blocks within ``bparams.band`` blocks of the points, up to depth 10.  Arguments
    as ``RunPoisson``.  -> (vertices [V, 3] float64, faces [F, 3] int32, info dict as ``RunPoisson``'s — depth, h and iso those of the
    finest level, cycles and rel_residual those of the base solve —, band info dict: per level (lists indexed by the level)
    n_active_blocks, n_free, rel_residual, bnorm, iterations; n_open_edges, scratch_bytes, base_depth, failed_level).  When the call
    fails, the exception carries ``info`` and ``band_info`` as far as they were written."""
    v, f, _, info, binfo, _ = _run_poisson_band(points, normals, params if params is not None else poisson_params(),
                                                bparams if bparams is not None else poisson_band_params(), None, stream, capacity)
    return v, f, _poisson_info(info), _poisson_band_info(binfo)


WEIGHT_NORMALS = 1                          # MVS_POISSON_WEIGHT_NORMALS


def poisson_density_params(**kw) -> L.CPoissonDensityParams:
    """``mvs_poisson_density_default_params`` (max_gain 4, flags 0: no weighting, density_drop 1) with the given fields replaced."""
    return _params(L.CPoissonDensityParams, L.lib().mvs_poisson_density_default_params, kw)


def RunPoissonDensity(points, normals, params: L.CPoissonParams | None = None, dparams: L.CPoissonDensityParams | None = None,
                      stream: int | None = None, capacity: tuple | None = None):
    """``mvs_poisson_reconstruct_density`` (rules 14-17 of include/mvs.h, this library's definition): ``RunPoisson`` with the sampling
    density — the normals weighted by mean density / local density when ``dparams.flags`` holds ``WEIGHT_NORMALS`` (off by default: the
    mesh is then ``RunPoisson``'s) — and the density of every vertex.  Arguments as ``RunPoisson``.
    -> (vertices [V, 3] float64, faces [F, 3] int32, density [V] float64, info dict: that of ``RunPoisson`` plus mean_density,
    min_point_density, max_point_density, density_depth, n_clamped)."""
    v, f, d, info, dinfo = _run_poisson(points, normals, params if params is not None else poisson_params(),
                                        dparams if dparams is not None else poisson_density_params(), stream, capacity)
    out = _poisson_info(info)
    out.update(mean_density=dinfo.mean_density, min_point_density=dinfo.min_point_density, max_point_density=dinfo.max_point_density,
               density_depth=dinfo.density_depth, n_clamped=dinfo.n_clamped)
    return v, f, d, out


def _poisson_density_info(dinfo: L.CPoissonDensityInfo) -> dict:
    return dict(mean_density=dinfo.mean_density, min_point_density=dinfo.min_point_density, max_point_density=dinfo.max_point_density,
                density_depth=dinfo.density_depth, n_clamped=dinfo.n_clamped)


def RunPoissonBandDensity(points, normals, params: L.CPoissonParams | None = None, bparams: L.CPoissonBandParams | None = None,
                          dparams: L.CPoissonDensityParams | None = None, stream: int | None = None, capacity: tuple | None = None):
    """``mvs_poisson_reconstruct_band_density`` (rules 32-35 of include/mvs.h, this library's definition): ``RunPoissonBand`` with the
    sampling density carried over every level — the normals of the base level and of every band level weighted by mean density / local
    density when ``dparams.flags`` holds ``WEIGHT_NORMALS`` (off by default: the mesh is then ``RunPoissonBand``'s) — and the density of
    every vertex, the values ``TrimByValue`` trims by.  Arguments as ``RunPoisson``.
    -> (vertices [V, 3] float64, faces [F, 3] int32, vertex_density [V] float64, info dict and band info dict as ``RunPoissonBand``'s,
    density info dict: mean_density, min_point_density, max_point_density, density_depth, n_clamped).  When the call fails, the
    exception carries ``info`` and ``band_info`` as far as they were written."""
    v, f, d, info, binfo, dinfo = _run_poisson_band(points, normals, params if params is not None else poisson_params(),
                                                    bparams if bparams is not None else poisson_band_params(),
                                                    dparams if dparams is not None else poisson_density_params(), stream, capacity)
    return v, f, d, _poisson_info(info), _poisson_band_info(binfo), _poisson_density_info(dinfo)


def poisson_screen_params(**kw) -> L.CPoissonScreenParams:
    """``mvs_poisson_screen_default_params`` (alpha 4) with the given fields replaced."""
    return _params(L.CPoissonScreenParams, L.lib().mvs_poisson_screen_default_params, kw)


def RunPoissonScreened(points, normals, params: L.CPoissonParams | None = None, dparams: L.CPoissonDensityParams | None = None,
                       sparams: L.CPoissonScreenParams | None = None, stream: int | None = None, capacity: tuple | None = None):
    """``mvs_poisson_reconstruct_screened`` (rules 19-23 of include/mvs.h, this library's definition): ``RunPoissonDensity`` followed by
    a second solve that pulls the field to the iso value at every point with the weight ``sparams.alpha`` (4 by default; 0: the bytes of
    ``RunPoissonDensity``).  Arguments as ``RunPoisson``.
    -> (vertices [V, 3] float64, faces [F, 3] int32, density [V] float64, info dict: that of ``RunPoissonDensity`` plus target, lambda,
    occupied, active_nodes, screen_cycles, screen_rel_residual, iso_unscreened)."""
    v, f, d, info, dinfo, sinfo = _run_poisson(points, normals, params if params is not None else poisson_params(),
                                               dparams if dparams is not None else poisson_density_params(), stream, capacity,
                                               sparams if sparams is not None else poisson_screen_params())
    out = _poisson_info(info)
    out.update(mean_density=dinfo.mean_density, min_point_density=dinfo.min_point_density, max_point_density=dinfo.max_point_density,
               density_depth=dinfo.density_depth, n_clamped=dinfo.n_clamped)
    out.update({"target": sinfo.target, "lambda": sinfo.lambda_, "occupied": sinfo.occupied, "active_nodes": sinfo.active_nodes,
                "screen_cycles": sinfo.cycles, "screen_rel_residual": sinfo.rel_residual, "iso_unscreened": sinfo.iso_unscreened})
    return v, f, d, out


def _poisson_screen_info(sinfo: L.CPoissonScreenInfo) -> dict:
    return {"target": sinfo.target, "lambda": sinfo.lambda_, "occupied": sinfo.occupied, "active_nodes": sinfo.active_nodes,
            "screen_cycles": sinfo.cycles, "screen_rel_residual": sinfo.rel_residual, "iso_unscreened": sinfo.iso_unscreened}


def _poisson_band_screen_info(bsinfo: L.CPoissonBandScreenInfo) -> dict:
    return {"lambda": list(bsinfo.lambda_), "target": list(bsinfo.target), "occupied": list(bsinfo.occupied),
            "active_nodes": list(bsinfo.active_nodes)}


def RunPoissonBandScreened(points, normals, params: L.CPoissonParams | None = None, bparams: L.CPoissonBandParams | None = None,
                           dparams: L.CPoissonDensityParams | None = None, sparams: L.CPoissonScreenParams | None = None,
                           stream: int | None = None, capacity: tuple | None = None):
    """``mvs_poisson_reconstruct_band_screened`` (rules 36-41 of include/mvs.h, this library's definition): ``RunPoissonBandDensity``
    with a screened solve on the base level and on every band level, the field pulled to the level's target at every point with the
    weight ``sparams.alpha`` (4 by default; 0: the bytes of ``RunPoissonBandDensity``).  Arguments as ``RunPoisson``.
    -> (vertices [V, 3] float64, faces [F, 3] int32, vertex_density [V] float64, info dict, band info dict and density info dict as
    ``RunPoissonBandDensity``'s, screen info dict of the base level: target, lambda, occupied, active_nodes, screen_cycles,
    screen_rel_residual, iso_unscreened; band screen info dict: per level (lists indexed by the level) lambda, target, occupied,
    active_nodes).  When the call fails, the exception carries ``info`` and ``band_info`` as far as they were written."""
    v, f, d, info, binfo, dinfo, sinfo, bsinfo = _run_poisson_band(points, normals, params if params is not None else poisson_params(),
                                                                   bparams if bparams is not None else poisson_band_params(),
                                                                   dparams if dparams is not None else poisson_density_params(), stream, capacity,
                                                                   sparams if sparams is not None else poisson_screen_params())
    return (v, f, d, _poisson_info(info), _poisson_band_info(binfo), _poisson_density_info(dinfo), _poisson_screen_info(sinfo),
            _poisson_band_screen_info(bsinfo))


def PoissonBandScreenedFiles(psr_npts, model_obj, params: L.CPoissonParams | None = None, bparams: L.CPoissonBandParams | None = None,
                             dparams: L.CPoissonDensityParams | None = None, sparams: L.CPoissonScreenParams | None = None,
                             trim_ratio: float = 0.0):
    """``mvs_processor_poisson_band_screened``: ``PoissonFiles`` through ``mvs_poisson_reconstruct_band_screened`` — reconstruct, trim
    where the vertex density lies below ``trim_ratio`` times the mean point density (0.0: no trim), vertex normals, write.  A parameter
    struct left None takes its defaults.  -> (V, F, n_open_edges), the open edges counted on the untrimmed mesh."""
    V, F, opened = C.c_int64(), C.c_int64(), C.c_int64()
    L.check(L.lib().mvs_processor_poisson_band_screened(os.fsencode(psr_npts), None if params is None else C.byref(params),
                                                        None if bparams is None else C.byref(bparams), None if dparams is None else C.byref(dparams),
                                                        None if sparams is None else C.byref(sparams), float(trim_ratio), os.fsencode(model_obj),
                                                        C.byref(V), C.byref(F), C.byref(opened)))
    return V.value, F.value, opened.value


def TrimByValue(vertices, faces, values, threshold: float, normals=None, stream: int | None = None):
    """``mvs_mesh_trim_by_value`` (rule 18 of include/mvs.h): the faces whose three vertices have ``values[v] >= threshold`` and the
    vertices those faces use, in their order, the faces renumbered.  Arrays, or contiguous torch tensors on the GPU (the device form,
    ordered on ``stream``).  -> (vertices, faces), or (vertices, faces, normals) when ``normals`` is given."""
    dev = _is_dev(vertices)
    if any(_is_dev(a) != dev for a in (faces, values)) or (normals is not None and _is_dev(normals) != dev):
        raise L.MvsError(-1, "vertices, faces, values and normals must all be tensors on the GPU or all arrays")
    order = _stream_order(stream) if dev else contextlib.nullcontext()
    if dev:
        import torch
        ptrs = [_dev_ptr(vertices, "float64", "vertices"), _dev_ptr(normals, "float64", "normals"), _dev_ptr(faces, "int32", "faces"),
                _dev_ptr(values, "float64", "values")]
        V, F = int(vertices.shape[0]), int(faces.shape[0])
        if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or values.numel() != V or \
                (normals is not None and tuple(normals.shape) != tuple(vertices.shape)):
            raise L.MvsError(-1, "vertices and normals must be [V, 3], faces [F, 3], values [V]")
        fn, tail = L.lib().mvs_mesh_trim_by_value_dev, (L.ptr(stream),)
    else:
        vertices, faces, values = L.arr(vertices, np.float64).reshape(-1, 3), L.arr(faces, np.int32).reshape(-1, 3), L.arr(values, np.float64).reshape(-1)
        normals = L.arr(normals, np.float64).reshape(-1, 3) if normals is not None else None
        V, F = len(vertices), len(faces)
        if len(values) != V or (normals is not None and len(normals) != V):
            raise L.MvsError(-1, "vertices and normals must be [V, 3], faces [F, 3], values [V]")
        ptrs = [L.ptr(vertices), L.ptr(normals), L.ptr(faces), L.ptr(values)]
        fn, tail = L.lib().mvs_mesh_trim_by_value, ()
    nV, nF = C.c_int64(), C.c_int64()
    with order:
        ov, of = _out_like(vertices, (max(1, V), 3), "float64"), _out_like(vertices, (max(1, F), 3), "int32")
        on = _out_like(vertices, (max(1, V), 3), "float64") if normals is not None else None
        if V == 0 or F == 0:                                    # a pointer to nothing is still a pointer: the outputs stand in
            ptrs = [L.ptr(ov), L.ptr(on), L.ptr(of), L.ptr(ov)]
        L.check(fn(V, ptrs[0], ptrs[1], F, ptrs[2], ptrs[3], float(threshold), L.ptr(ov), L.ptr(on), L.ptr(of), C.byref(nV), C.byref(nF), *tail))
    if normals is not None:
        return ov[:nV.value], of[:nF.value], on[:nV.value]
    return ov[:nV.value], of[:nF.value]


def CullPoissonModel(model_obj, scales, Rs, ts, cameras, out_obj, all_seq_proj: bool = True):
    """The trim of the Poisson model (R/Processor/Processor.cpp:1057-1105): ReadObj (normals computed when the file has no `vn`),
    the AllSeqProj cull with its facet remap, RetainConnectRegion, WriteObj.  -> (V, F) written."""
    n, s, R, t, coff, cams = L.seq_tables(scales, Rs, ts, cameras)
    V, F = C.c_int64(), C.c_int64()
    L.check(L.lib().mvs_processor_cull_model(os.fsencode(model_obj), n, L.ptr(s), L.ptr(R), L.ptr(t), L.ptr(coff), cams,
                                             int(bool(all_seq_proj)), os.fsencode(out_obj), C.byref(V), C.byref(F)))
    return V.value, F.value


# ------------------------------------------------------------------ deform ----
def Deform(model_obj, template_obj, parts_path, cam_R, dist_thres: float, out_obj, params: L.CParams | None = None) -> dict:
    """./Result/Model.obj + ./Template/meanbody.obj + ./Template/part/parts -> ./Result/deform.obj.
    ``cam_R`` is the rotation of cameras[0][0]; the view ray is its third row (R^T.col(2))."""
    R = L.arr(cam_R, np.float64).reshape(9)
    prm = params if params is not None else default_params()
    st = L.CStats()
    rc = L.check(L.lib().mvs_processor_deform(os.fsencode(model_obj), os.fsencode(template_obj), os.fsencode(parts_path), L.ptr(R),
                                              float(dist_thres), C.byref(prm), os.fsencode(out_obj), C.byref(st)))
    return _stats(st, rc)


# ------------------------------------------------------------------ render ----
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


# ------------------------------------------------------------------ depth refinement ----
def depth_refine_params(**kw) -> L.CDepthRefineParams:
    """``mvs_depth_refine_default_params`` (config.txt: MinDsp 0.0025, MaxDsp 0.3, SSDError 40, SSDWin 7; refFrmCount 5 of
    DepthOptimizer.cpp:45; rel_range 0.04, steps 8, flags ``REFINE_SUBSTEP``) with the given fields replaced."""
    return _params(L.CDepthRefineParams, L.lib().mvs_depth_refine_default_params, kw)


def _flat_stack(stacks, n, dev, dtype, what):
    """the per-sequence stacks of a call as one flat array where they live (``dev``: torch, on the current stream); never empty"""
    if dev:
        import torch
        flat = torch.cat([a.reshape(-1) for a in stacks]) if n > 1 else stacks[0].reshape(-1)
        if flat.numel() == 0:
            flat = torch.zeros(1, dtype=getattr(torch, dtype), device=flat.device)
        return flat, _dev_ptr(flat, dtype, what)
    flat = np.concatenate([L.arr(a, dtype).reshape(-1) for a in stacks]) if n else np.zeros(1, dtype)
    if flat.size == 0:
        flat = np.zeros(1, dtype)
    return flat, L.ptr(flat)


def RefineAllDepthMaps(cameras, imgs, depths, params: L.CDepthRefineParams | None = None, stream: int | None = None, with_detail: bool = False):
    """DepthOptimizer::RefineAllDepthMaps (DepthRecovery/DepthOptimizer.cpp:20-43) for every sequence in one call
    (``mvs_refine_depth_maps``; the rules, this library's definition: include/mvs.h).  ``cameras[k]`` lists sequence k's cameras;
    ``imgs[k]`` is its RGB base images [frames, h, w, 3] uint8 and ``depths[k]`` its rendered rasters [frames, h, w] float32
    (``RenderViews``' result) — numpy arrays, or contiguous torch tensors on the GPU (the device form: the results are tensors on the
    same device).  ``stream`` is the HIP stream that produced them (None: the legacy default stream); the kernels, the concatenation
    of the sequences and the allocation of the results are all ordered on it, whatever torch's current stream is.
    -> a list with, per sequence, the refined rasters [frames, h, w] float32: what ``CheckConsistency`` and ``RunPointSample`` read.
    With ``with_detail`` each entry is (refined, k [frames, h, w] int8, sum int32, cnt uint8): the winning hypothesis of every pixel
    (-128 where the pixel kept its input), its sum of squared grey differences and the reference frames that took part."""
    prm = params if params is not None else depth_refine_params()
    n = len(cameras)
    off, cams = L.seq_cams(cameras)
    if len(imgs) != n or len(depths) != n:
        raise L.MvsError(-1, f"{len(imgs)} image stacks and {len(depths)} raster stacks for {n} sequences")
    shapes = []
    for k in range(n):
        want = (len(cameras[k]),) + ((int(cameras[k][0].h), int(cameras[k][0].w)) if len(cameras[k]) else tuple(depths[k].shape[1:]))
        if tuple(depths[k].shape) != want or tuple(imgs[k].shape) != want + (3,):
            raise L.MvsError(-1, f"depths[{k}] must be [frames, h, w] = {want} and imgs[{k}] [frames, h, w, 3]")
        shapes.append(want)
    dev = n > 0 and all(_is_dev(a) for a in depths) and all(_is_dev(a) for a in imgs)
    if not dev and (any(_is_dev(a) for a in depths) or any(_is_dev(a) for a in imgs)):
        raise L.MvsError(-1, "imgs and depths must all be tensors on the GPU or all arrays")
    order = _stream_order(stream) if dev else contextlib.nullcontext()
    with order:
        fimg, iptr = _flat_stack(imgs, n, dev, "uint8", "imgs")
        fdep, dptr = _flat_stack(depths, n, dev, "float32", "depths")
        size = int(fdep.numel()) if dev else fdep.size
        out = _out_like(fdep, size, "float32")
        det = tuple(_out_like(fdep, size, dt) for dt in ("int8", "int32", "uint8")) if with_detail else (None, None, None)
        fn, tail = (L.lib().mvs_refine_depth_maps_dev, (L.ptr(stream),)) if dev else (L.lib().mvs_refine_depth_maps, ())
        L.check(fn(n, L.ptr(off), cams, iptr, dptr, C.byref(prm), L.ptr(out), *[L.ptr(a) for a in det], *tail))
    res, at = [], 0
    for shape in shapes:
        m = int(np.prod(shape, dtype=np.int64))
        cut = tuple(a[at:at + m].reshape(shape) for a in ((out,) + det if with_detail else (out,)))
        res.append(cut if with_detail else cut[0])
        at += m
    return res


def RefineDepthFiles(seq_dirs, cameras, imgs, params: L.CDepthRefineParams | None = None) -> None:
    """``mvs_processor_refine_depths``: sequence k's rendered rasters ``seq_dirs[k]``/DATA/Render/_depth<i>.raw (what ``Render`` wrote) ->
    ``seq_dirs[k]``/DATA/Refine/_depth<i>.raw.  ``cameras[k]`` lists sequence k's cameras, ``imgs[k]`` is its RGB base images
    [frames, h, w, 3] uint8 in memory (``RefineDepthFilesFromJpeg`` reads them from the sequence directories)."""
    n = len(cameras)
    if len(seq_dirs) != n or len(imgs) != n:
        raise L.MvsError(-1, f"{len(seq_dirs)} sequence dirs and {len(imgs)} image stacks for {n} sequences")
    for k in range(n):
        want = (len(cameras[k]),) + ((int(cameras[k][0].h), int(cameras[k][0].w), 3) if len(cameras[k]) else tuple(imgs[k].shape[1:]))
        if tuple(imgs[k].shape) != want:
            raise L.MvsError(-1, f"imgs[{k}] must be [frames, h, w, 3] = {want}")
    off, cams = L.seq_cams(cameras)
    dirs = (C.c_char_p * max(1, n))(*[os.fsencode(d) for d in seq_dirs])
    flat, iptr = _flat_stack(imgs, n, False, "uint8", "imgs")
    prm = params if params is not None else depth_refine_params()
    L.check(L.lib().mvs_processor_refine_depths(n, dirs, L.ptr(off), cams, iptr, C.byref(prm)))


# ------------------------------------------------------------------ depth recovery ----
def depth_recover_params(**kw) -> L.CDepthRecoverParams:
    """``mvs_depth_recover_default_params`` (config.txt: MinDsp 0.0025, MaxDsp 0.3, SSDError 40, SSDWin 7; refFrmCount 5 of
    DepthOptimizer.cpp:45; peak 0.9, levels 128, min_refs 2 — choices nobody has measured on a real sequence; flags
    ``RECOVER_SUBSTEP``) with the given fields replaced."""
    return _params(L.CDepthRecoverParams, L.lib().mvs_depth_recover_default_params, kw)


def RecoverDepthMaps(cameras, imgs, params: L.CDepthRecoverParams | None = None, stream: int | None = None, with_detail: bool = False):
    """The first inverse-depth rasters of every sequence from its images alone, in one call (``mvs_recover_depth_maps``; the rules
    R1-R9, this library's definition: include/mvs.h): what the reference reads as DATA/_depth<i>.raw and never writes.  ``cameras[k]``
    lists sequence k's cameras; ``imgs[k]`` is its RGB base images [frames, h, w, 3] uint8 — numpy arrays, or contiguous torch tensors
    on the GPU (the device form: the results are tensors on the same device).  ``stream`` is the HIP stream that produced them (None:
    the legacy default stream); the kernels, the concatenation of the sequences and the allocation of the results are all ordered on
    it, whatever torch's current stream is.
    -> a list with, per sequence, the rasters [frames, h, w] float32 (+0.0 where no level was accepted): what ``CheckConsistency``
    reads.  With ``with_detail`` each entry is (rasters, level [frames, h, w] int16, sum int32, cnt uint8): the winning level of
    every pixel (-1 where none was accepted), its sum of squared grey differences and the reference frames that took part."""
    return _recover(cameras, imgs, params if params is not None else depth_recover_params(), None, stream, with_detail)


def _recover(cameras, imgs, prm, aprm, stream, with_detail):
    """the call behind ``RecoverDepthMaps`` (``aprm`` None) and ``RecoverDepthMapsAggregated``"""
    n = len(cameras)
    off, cams = L.seq_cams(cameras)
    if len(imgs) != n:
        raise L.MvsError(-1, f"{len(imgs)} image stacks for {n} sequences")
    shapes = []
    for k in range(n):
        want = (len(cameras[k]),) + ((int(cameras[k][0].h), int(cameras[k][0].w)) if len(cameras[k]) else tuple(imgs[k].shape[1:3]))
        if tuple(imgs[k].shape) != want + (3,):
            raise L.MvsError(-1, f"imgs[{k}] must be [frames, h, w, 3] = {want + (3,)}")
        shapes.append(want)
    dev = n > 0 and all(_is_dev(a) for a in imgs)
    if not dev and any(_is_dev(a) for a in imgs):
        raise L.MvsError(-1, "imgs must all be tensors on the GPU or all arrays")
    order = _stream_order(stream) if dev else contextlib.nullcontext()
    with order:
        fimg, iptr = _flat_stack(imgs, n, dev, "uint8", "imgs")
        size = max(1, sum(int(np.prod(s, dtype=np.int64)) for s in shapes))
        out = _out_like(fimg, size, "float32")
        kinds = ("int16", "int32", "uint8") + (("int32",) if aprm is not None else ())
        det = tuple(_out_like(fimg, size, dt) for dt in kinds) if with_detail else (None,) * len(kinds)
        name = "mvs_recover_depth_maps" + ("_aggregated" if aprm is not None else "") + ("_dev" if dev else "")
        head = (C.byref(prm),) + ((C.byref(aprm),) if aprm is not None else ())
        L.check(getattr(L.lib(), name)(n, L.ptr(off), cams, iptr, *head, L.ptr(out), *[L.ptr(a) for a in det], *((L.ptr(stream),) if dev else ())))
    res, at = [], 0
    for shape in shapes:
        m = int(np.prod(shape, dtype=np.int64))
        cut = tuple(a[at:at + m].reshape(shape) for a in ((out,) + det if with_detail else (out,)))
        res.append(cut if with_detail else cut[0])
        at += m
    return res


def depth_aggregate_params(**kw) -> L.CDepthAggregateParams:
    """``mvs_depth_aggregate_default_params`` (p1 8, p2 128, cost_cap 255 — choices nobody has measured on a real sequence; paths 8;
    max_volume_mb 0: the library's budget) with the given fields replaced."""
    return _params(L.CDepthAggregateParams, L.lib().mvs_depth_aggregate_default_params, kw)


def RecoverDepthMapsAggregated(cameras, imgs, params: L.CDepthRecoverParams | None = None, aparams: L.CDepthAggregateParams | None = None,
                               stream: int | None = None, with_detail: bool = False):
    """``RecoverDepthMaps`` with semi-global path aggregation of the cost volume before the winner is taken
    (``mvs_recover_depth_maps_aggregated``; the rules S1-S6, this library's definition: include/mvs.h).  Arguments and results as
    ``RecoverDepthMaps``; ``aparams`` holds the penalties, the cost cap, the number of paths and the memory budget.  With ``with_detail``
    each entry is (rasters, level int16, sum int32, cnt uint8, agg int32): the winner's raw sum and count, and its aggregated cost S
    (-1 outside the rectangle of candidates)."""
    return _recover(cameras, imgs, params if params is not None else depth_recover_params(),
                    aparams if aparams is not None else depth_aggregate_params(), stream, with_detail)


def _recover_files_args(seq_dirs, cameras):
    n = len(cameras)
    if len(seq_dirs) != n:
        raise L.MvsError(-1, f"{len(seq_dirs)} sequence dirs for {n} sequences")
    off, cams = L.seq_cams(cameras)
    return n, (C.c_char_p * max(1, n))(*[os.fsencode(d) for d in seq_dirs]), off, cams


def RecoverDepthFiles(seq_dirs, cameras, imgs, params: L.CDepthRecoverParams | None = None) -> None:
    """``mvs_processor_recover_depths``: ``RecoverDepthMaps`` of all sequences written to ``seq_dirs[k]``/DATA/_depth<i>.raw, the rasters
    ``CheckConsistency`` on files reads.  ``cameras[k]`` lists sequence k's cameras, ``imgs[k]`` is its RGB base images
    [frames, h, w, 3] uint8 in memory (``RecoverDepthFilesFromJpeg`` reads them from the sequence directories)."""
    n, dirs, off, cams = _recover_files_args(seq_dirs, cameras)
    if len(imgs) != n:
        raise L.MvsError(-1, f"{len(imgs)} image stacks for {n} sequences")
    for k in range(n):
        want = (len(cameras[k]),) + ((int(cameras[k][0].h), int(cameras[k][0].w), 3) if len(cameras[k]) else tuple(imgs[k].shape[1:]))
        if tuple(imgs[k].shape) != want:
            raise L.MvsError(-1, f"imgs[{k}] must be [frames, h, w, 3] = {want}")
    flat, iptr = _flat_stack(imgs, n, False, "uint8", "imgs")
    prm = params if params is not None else depth_recover_params()
    L.check(L.lib().mvs_processor_recover_depths(n, dirs, L.ptr(off), cams, iptr, C.byref(prm)))


def RecoverDepthFilesFromJpeg(seq_dirs, cameras, params: L.CDepthRecoverParams | None = None) -> None:
    """``mvs_processor_recover_depths_files``: ``RecoverDepthFiles`` with the RGB frames read from ``seq_dirs[k]``%05d.jpg."""
    n, dirs, off, cams = _recover_files_args(seq_dirs, cameras)
    prm = params if params is not None else depth_recover_params()
    L.check(L.lib().mvs_processor_recover_depths_files(n, dirs, L.ptr(off), cams, C.byref(prm)))


def RecoverDepthFilesAggregated(seq_dirs, cameras, imgs, params: L.CDepthRecoverParams | None = None,
                                aparams: L.CDepthAggregateParams | None = None) -> None:
    """``mvs_processor_recover_depths_aggregated``: ``RecoverDepthFiles`` with ``RecoverDepthMapsAggregated`` in place of the plain sweep."""
    n, dirs, off, cams = _recover_files_args(seq_dirs, cameras)
    if len(imgs) != n:
        raise L.MvsError(-1, f"{len(imgs)} image stacks for {n} sequences")
    for k in range(n):
        want = (len(cameras[k]),) + ((int(cameras[k][0].h), int(cameras[k][0].w), 3) if len(cameras[k]) else tuple(imgs[k].shape[1:]))
        if tuple(imgs[k].shape) != want:
            raise L.MvsError(-1, f"imgs[{k}] must be [frames, h, w, 3] = {want}")
    flat, iptr = _flat_stack(imgs, n, False, "uint8", "imgs")
    prm = params if params is not None else depth_recover_params()
    aprm = aparams if aparams is not None else depth_aggregate_params()
    L.check(L.lib().mvs_processor_recover_depths_aggregated(n, dirs, L.ptr(off), cams, iptr, C.byref(prm), C.byref(aprm)))


def RecoverDepthFilesAggregatedFromJpeg(seq_dirs, cameras, params: L.CDepthRecoverParams | None = None,
                                        aparams: L.CDepthAggregateParams | None = None) -> None:
    """``mvs_processor_recover_depths_aggregated_files``: ``RecoverDepthFilesAggregated`` with the RGB frames read from
    ``seq_dirs[k]``%05d.jpg."""
    n, dirs, off, cams = _recover_files_args(seq_dirs, cameras)
    prm = params if params is not None else depth_recover_params()
    aprm = aparams if aparams is not None else depth_aggregate_params()
    L.check(L.lib().mvs_processor_recover_depths_aggregated_files(n, dirs, L.ptr(off), cams, C.byref(prm), C.byref(aprm)))


# ------------------------------------------------------------------ vertex colours ----
def colour_params(**kw) -> L.CColourParams:
    """``mvs_colour_default_params`` (min_cos 0.2, occ_tol 0.01, flags 0, fill 128 128 128 — choices nobody has measured on a real
    sequence) with the given fields replaced; ``fill`` takes three byte values, ``flags`` may be ``COLOUR_BEST``."""
    fill = kw.pop("fill", None)
    prm = _params(L.CColourParams, L.lib().mvs_colour_default_params, kw)
    if fill is not None:
        prm.fill[:] = [int(v) for v in fill]
    return prm


def ColourVertices(points, normals, cameras, imgs, depths=None, scales=None, Rs=None, ts=None, params: L.CColourParams | None = None,
                   stream: int | None = None, with_counts: bool = False):
    """The colour of every vertex from the base images of all cameras of all sequences, in one call (``mvs_colour_vertices``; the rules
    C1-C8, this library's definition: include/mvs.h).  ``points`` / ``normals`` [V, 3] float64 in the world frame; ``cameras[k]`` lists
    sequence k's cameras, all of one size; ``imgs`` [N, h, w, 3] uint8 and ``depths`` [N, h, w] float32 (the rasters of ``RenderViews``,
    or None: no occlusion test) hold all cameras in camera order; ``scales`` / ``Rs`` / ``ts`` are the SRT chain (None for all three: the
    world frame).  The arrays are numpy arrays, or contiguous torch tensors on the GPU (the device form: the results are tensors on the
    same device); ``stream`` is the HIP stream that produced them (None: the legacy default stream), and the allocation of the results
    is ordered on it.  -> colours [V, 3] uint8 in the channel order of the images; with ``with_counts`` (colours, n_views [V] int32)."""
    prm = params if params is not None else colour_params()
    n, s, R, t, coff, cams = _view_tables(cameras, scales, Rs, ts)
    N = int(coff[-1])
    w0, h0 = (int(cameras[0][0].w), int(cameras[0][0].h)) if N and len(cameras[0]) else (0, 0)
    arrays = [points, normals, imgs] + ([depths] if depths is not None else [])
    dev = all(_is_dev(a) for a in arrays)
    if not dev and any(_is_dev(a) for a in arrays):
        raise L.MvsError(-1, "points, normals, imgs and depths must all be tensors on the GPU or all arrays")
    if not dev:
        points, normals = L.arr(points, np.float64), L.arr(normals, np.float64)
        imgs = L.arr(imgs, np.uint8)
        depths = None if depths is None else L.arr(depths, np.float32)
    V = int(points.shape[0]) if len(points.shape) == 2 else -1
    if tuple(points.shape) != (V, 3) or tuple(normals.shape) != (V, 3):
        raise L.MvsError(-1, "points and normals must be [V, 3]")
    if tuple(imgs.shape) != (N, h0, w0, 3):
        raise L.MvsError(-1, f"imgs must be [N, h, w, 3] = {(N, h0, w0, 3)}")
    if depths is not None and tuple(depths.shape) != (N, h0, w0):
        raise L.MvsError(-1, f"depths must be [N, h, w] = {(N, h0, w0)}")
    order = _stream_order(stream) if dev else contextlib.nullcontext()
    with order:
        col = _out_like(points, (V, 3), "uint8")
        cnt = _out_like(points, (V,), "int32") if with_counts else None
        if dev:
            ptrs = (_dev_ptr(points, "float64", "points"), _dev_ptr(normals, "float64", "normals"))
            iptr, dptr = _dev_ptr(imgs, "uint8", "imgs"), _dev_ptr(depths, "float32", "depths")
            fn, tail = L.lib().mvs_colour_vertices_dev, (L.ptr(stream),)
        else:
            ptrs, iptr, dptr = (L.ptr(points), L.ptr(normals)), L.ptr(imgs), L.ptr(depths)
            fn, tail = L.lib().mvs_colour_vertices, ()
        L.check(fn(*ptrs, V, n, L.ptr(s), L.ptr(R), L.ptr(t), L.ptr(coff), cams, iptr, dptr, C.byref(prm), L.ptr(col), L.ptr(cnt), *tail))
    return (col, cnt) if with_counts else col


def ColourModelFiles(model_obj, srt_txt, seq_dirs, cameras, out_obj, params: L.CColourParams | None = None, znear: float = 0.01,
                     zfar: float = 2000.0) -> int:
    """``mvs_processor_colour_model``: ``model_obj`` (Model.obj, PSR%d.obj, deform.obj) coloured from the frames ``seq_dirs[k]``%05d.jpg
    of every sequence and written to ``out_obj`` with ``v x y z r g b`` lines.  The chain comes from ``srt_txt``; the occlusion test uses
    the mesh rendered from every camera (``RenderViews``), and is skipped for a file without facets.  -> vertices that received a colour."""
    n, _, _, _, coff, cams = _view_tables(cameras, None, None, None)
    if len(seq_dirs) != n:
        raise L.MvsError(-1, f"{len(seq_dirs)} sequence dirs for {n} sequences")
    dirs = (C.c_char_p * max(1, n))(*[os.fsencode(d) for d in seq_dirs])
    prm = params if params is not None else colour_params()
    nc = C.c_int64()
    L.check(L.lib().mvs_processor_colour_model(os.fsencode(model_obj), os.fsencode(srt_txt), n, L.ptr(coff), cams, dirs, C.byref(prm),
                                               float(znear), float(zfar), os.fsencode(out_obj), C.byref(nc)))
    return nc.value


# ------------------------------------------------------------------ base images ----
def _jpeg_order(order):
    if order not in ("BGR", "RGB"):
        raise L.MvsError(-1, "order must be 'BGR' or 'RGB'")
    return L.JPEG_RGB if order == "RGB" else L.JPEG_BGR


def JpegInfo(data) -> dict:
    """``mvs_jpeg_info``: the header walk of one JPEG stream (rules J1, J2 of include/mvs.h; host code, no device needed) ->
    dict(w, h, components, h_samp, v_samp, restart_interval, n_segments, sof).  A stream the decoder rejects raises MVS_E_IO naming the
    feature."""
    buf = np.frombuffer(bytes(data) or b"\0", np.uint8)
    info = L.CJpegInfo()
    L.check(L.lib().mvs_jpeg_info(L.ptr(buf), len(bytes(data)), C.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in L.CJpegInfo._fields_}


def DecodeJpegs(datas, order: str = "BGR", device=None, stream: int | None = None):
    """``mvs_jpeg_decode``: the baseline JPEG streams ``datas`` (bytes each, all of one size) -> [n, h, w, 3] uint8, every image through
    each kernel in one launch (rules J1-J8 of include/mvs.h: this library's definition, pinned byte for byte against libjpeg-turbo's
    default decompressor).  ``order`` "BGR" is ``cv::imread``'s layout (what ``GenNewViews`` and the match filter take), "RGB" what
    ``RefineAllDepthMaps`` documents.  With ``device`` (a torch device) the result is a tensor there and the pixels never visit the host
    (``mvs_jpeg_decode_dev`` in the order of ``stream``, a HIP stream handle; None: the legacy default stream); otherwise a numpy
    array."""
    flags = _jpeg_order(order)
    datas = [bytes(d) for d in datas]
    n = len(datas)
    if n < 1:
        raise L.MvsError(-1, "need at least one stream")
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(d) for d in datas])
    blob = np.frombuffer(b"".join(datas) or b"\0", np.uint8)
    info = JpegInfo(datas[0])
    shape = (n, info["h"], info["w"], 3)
    if device is None:
        out = np.empty(shape, np.uint8)
        L.check(L.lib().mvs_jpeg_decode(n, L.ptr(off), L.ptr(blob), flags, L.ptr(out)))
        return out
    import torch
    order_ctx = _stream_order(stream)
    with order_ctx:
        out = torch.empty(shape, dtype=torch.uint8, device=device)
        L.check(L.lib().mvs_jpeg_decode_dev(n, L.ptr(off), L.ptr(blob), flags, L.ptr(out), L.ptr(stream)))
    return out


# ------------------------------------------------------------------ JPEG encode ----
_SAMPLING = {"444": 444, "422": 422, "420": 420, 444: 444, 422: 422, 420: 420}


def jpeg_encode_params(**kw) -> L.CJpegEncodeParams:
    """``mvs_jpeg_encode_default_params`` (quality 95, sampling 420, restart_interval 0: what ``cv::imwrite`` writes) with the given fields
    replaced; ``restart_interval=L.JPEG_RESTART_ROW`` is one MCU row per interval."""
    return _params(L.CJpegEncodeParams, L.lib().mvs_jpeg_encode_default_params, kw)


def _jpeg_enc_call(imgs, quality, sampling, restart_interval, order):
    """-> (n, h, w, flags, params) of an encoder call on ``imgs`` [n, h, w, 3] or, with ``order`` "GREY", [n, h, w]"""
    if order not in ("BGR", "RGB", "GREY"):
        raise L.MvsError(-1, "order must be 'BGR', 'RGB' or 'GREY'")
    if sampling not in _SAMPLING:
        raise L.MvsError(-1, "sampling must be '444', '422' or '420'")
    shape = tuple(int(x) for x in imgs.shape)
    if (len(shape) != 3 if order == "GREY" else len(shape) != 4 or shape[3] != 3) or shape[0] < 1:
        raise L.MvsError(-1, "imgs must be [n, h, w, 3] uint8, or [n, h, w] with order 'GREY', n >= 1")
    flags = L.JPEG_GREY if order == "GREY" else L.JPEG_RGB if order == "RGB" else L.JPEG_BGR
    prm = jpeg_encode_params(quality=int(quality), sampling=_SAMPLING[sampling], restart_interval=int(restart_interval))
    return shape[0], shape[1], shape[2], flags, prm


def JpegEncodeBound(w: int, h: int, quality: int = 95, sampling="420", restart_interval: int = 0, order: str = "BGR") -> int:
    """``mvs_jpeg_encode_bound``: bytes that hold any stream of one w x h image with these parameters (host code, no device needed)."""
    _, _, _, flags, prm = _jpeg_enc_call(np.empty((1, 1, 1) if order == "GREY" else (1, 1, 1, 3), np.uint8), quality, sampling, restart_interval, order)
    return int(L.check(L.lib().mvs_jpeg_encode_bound(int(w), int(h), flags, C.byref(prm))))


def EncodeJpegs(imgs, quality: int = 95, sampling="420", restart_interval: int = 0, order: str = "BGR", device=None, stream: int | None = None,
                capacity: int | None = None):
    """``mvs_jpeg_encode``: ``imgs`` [n, h, w, 3] uint8 in ``order`` "BGR" (``cv::imwrite``'s layout) or "RGB", or [n, h, w] with ``order``
    "GREY" -> the baseline JPEG stream of every image, all images through each kernel in one launch (rules E1-E9 of include/mvs.h: this
    library's definition, pinned byte for byte against libjpeg-turbo's default compressor).  A numpy array -> list[bytes].  With
    ``device`` (a torch device; ``imgs`` may already be a tensor there) -> (data uint8 tensor [total], offsets int64 numpy [n + 1]):
    ``mvs_jpeg_encode_dev`` in the order of ``stream`` (a HIP stream handle; None: the legacy default stream); pixels and streams never
    visit the host.  ``capacity`` (bytes; default n x ``mvs_jpeg_encode_bound``) sizes the output; a call that needs more raises
    MVS_E_INVALID_ARG, and the error carries ``offsets`` as the call wrote them."""
    dev = device is not None or _is_dev(imgs)
    if not dev:
        imgs = L.arr(imgs, np.uint8)
    n, h, w, flags, prm = _jpeg_enc_call(imgs, quality, sampling, restart_interval, order)
    cap = int(capacity) if capacity is not None else n * int(L.check(L.lib().mvs_jpeg_encode_bound(w, h, flags, C.byref(prm))))
    off = np.zeros(n + 1, np.int64)

    def finish(rc):
        try:
            L.check(rc)
        except L.MvsError as e:
            e.offsets = off
            raise

    if not dev:
        out = np.empty(max(1, cap), np.uint8)
        finish(L.lib().mvs_jpeg_encode(n, w, h, L.ptr(imgs), flags, C.byref(prm), L.ptr(off), L.ptr(out), cap))
        return [out[off[i]:off[i + 1]].tobytes() for i in range(n)]
    import torch
    order_ctx = _stream_order(stream)
    with order_ctx:
        src = imgs if _is_dev(imgs) else torch.as_tensor(L.arr(imgs, np.uint8)).to(device)
        out = torch.empty(max(1, cap), dtype=torch.uint8, device=src.device)
        finish(L.lib().mvs_jpeg_encode_dev(n, w, h, _dev_ptr(src, "uint8", "imgs"), flags, C.byref(prm), L.ptr(off), L.ptr(out), cap, L.ptr(stream)))
    return out[:int(off[n])], off


def JpegRoundTrip(imgs, quality: int = 95, sampling="420", restart_interval: int = 0, order: str = "BGR", stream: int | None = None):
    """``mvs_jpeg_roundtrip``: the pixels ``DecodeJpegs(EncodeJpegs(imgs, ...), order)`` returns, [n, h, w, 3] uint8, without a stream in
    between (the transform launch of the encoder, then the decoder's inverse DCT and pixel launches): what SIFT sees after the reference
    wrote a view to ``proj%d_%d.jpg`` and read it back.  A numpy array -> a numpy array; a contiguous torch tensor on the GPU -> a tensor
    there (``mvs_jpeg_roundtrip_dev`` in the order of ``stream``)."""
    dev = _is_dev(imgs)
    if not dev:
        imgs = L.arr(imgs, np.uint8)
    n, h, w, flags, prm = _jpeg_enc_call(imgs, quality, sampling, restart_interval, order)
    if not dev:
        out = np.empty((n, h, w, 3), np.uint8)
        L.check(L.lib().mvs_jpeg_roundtrip(n, w, h, L.ptr(imgs), flags, C.byref(prm), L.ptr(out)))
        return out
    import torch
    order_ctx = _stream_order(stream)
    with order_ctx:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=imgs.device)
        L.check(L.lib().mvs_jpeg_roundtrip_dev(n, w, h, _dev_ptr(imgs, "uint8", "imgs"), flags, C.byref(prm), L.ptr(out), L.ptr(stream)))
    return out


def DepthPreview(depths, stream: int | None = None):
    """``mvs_depth_preview``: RenderDepthMap's grey image (R/Common/Utils.h:189-217) of every raster of ``depths`` [n, h, w] float32 ->
    [n, h, w] uint8: 255 * (d - d_min) / (d_max - d_min) truncated over the valid (d >= 0, finite) pixels of the raster, 255 elsewhere;
    0 where d_max == d_min.  A numpy array, or a contiguous torch tensor on the GPU (the device form, in the order of ``stream``)."""
    dev = _is_dev(depths)
    if not dev:
        depths = L.arr(depths, np.float32)
    if len(depths.shape) != 3 or depths.shape[0] < 1:
        raise L.MvsError(-1, "depths must be [n, h, w] float32, n >= 1")
    n, h, w = (int(x) for x in depths.shape)
    if not dev:
        out = np.empty((n, h, w), np.uint8)
        L.check(L.lib().mvs_depth_preview(n, w, h, L.ptr(depths), L.ptr(out)))
        return out
    import torch
    order_ctx = _stream_order(stream)
    with order_ctx:
        out = torch.empty((n, h, w), dtype=torch.uint8, device=depths.device)
        L.check(L.lib().mvs_depth_preview_dev(n, w, h, _dev_ptr(depths, "float32", "depths"), L.ptr(out), L.ptr(stream)))
    return out


def SaveViews(seq_dir, views, quality: int = 95, sampling="420", restart_interval: int = 0, order: str = "BGR") -> None:
    """``mvs_processor_save_views``: the views of ``GenNewViews`` [frames, view_count, h, w, 3] uint8 -> ``seq_dir``Views/proj<frame>_<view>.jpg
    (R/Image3D/Image3D.cpp:218-219), the bytes ``EncodeJpegs`` returns for them."""
    v = L.arr(views, np.uint8)
    if v.ndim != 5 or v.shape[4] != 3 or order not in ("BGR", "RGB"):
        raise L.MvsError(-1, "views must be [frames, view_count, h, w, 3] in order 'BGR' or 'RGB'")
    _, h, w, flags, prm = _jpeg_enc_call(v.reshape((-1,) + v.shape[2:]), quality, sampling, restart_interval, order)
    L.check(L.lib().mvs_processor_save_views(os.fsencode(seq_dir), int(v.shape[0]), int(v.shape[1]), w, h, L.ptr(v), flags, C.byref(prm)))


def DepthPreviewFiles(seq_dir, sub: str, n: int, w: int, h: int, quality: int = 95, restart_interval: int = 0) -> None:
    """``mvs_processor_depth_previews``: ``seq_dir``DATA/``sub``/_depth<i>.raw, i < n, each w x h -> _depth<i>.jpg beside it: ``EncodeJpegs``
    (grey) of ``DepthPreview`` of the rasters.  ``sub`` is "CHECK", "Render" or "Refine"."""
    prm = jpeg_encode_params(quality=int(quality), restart_interval=int(restart_interval))
    L.check(L.lib().mvs_processor_depth_previews(os.fsencode(seq_dir), os.fsencode(sub), int(n), int(w), int(h), C.byref(prm)))


# ------------------------------------------------------------------ overlay pictures ----
def draw_prim(kind: int, x0: int, y0: int, x1: int = 0, y1: int = 0, size: int = 1, colour=(0, 0, 0)):
    """one ``mvs_draw_prim`` as a record of ``L.DRAW_PRIM_DTYPE``: ``kind`` is ``L.DRAW_DISC`` / ``L.DRAW_RING`` (centre (x0, y0), radius
    ``size``) or ``L.DRAW_SEGMENT`` ((x0, y0) - (x1, y1), thickness ``size``); ``colour`` in the canvas's channel order"""
    return (int(x0), int(y0), int(x1), int(y1), int(kind), int(size), tuple(int(c) for c in colour), (0, 0, 0))


def cv_rng_colours(n: int, state: int = 0xFFFFFFFF):
    """``mvs_cv_rng_colours`` (rule O6 of include/mvs.h; host code): the next ``n`` line colours of the ``cv::RNG`` at ``state`` (default: a
    fresh generator) -> (bgr uint8 [n, 3], the advanced state)."""
    st = C.c_uint64(int(state))
    out = np.zeros((max(1, int(n)), 3), np.uint8)
    L.lib().mvs_cv_rng_colours(C.byref(st), int(n), L.ptr(out))
    return out[:max(0, int(n))].copy(), int(st.value)


def _lists(lists, n, dtype, cols, what):
    """``lists[i]`` = the rows of list i -> (offsets int64 [n + 1], all rows back to back)"""
    if len(lists) != n:
        raise L.MvsError(-1, f"{what}: {len(lists)} lists for {n} canvases")
    flat = [np.asarray(p, dtype=dtype).reshape((-1,) + cols) for p in lists]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in flat])
    allr = np.ascontiguousarray(np.concatenate(flat)) if off[-1] else np.zeros((0,) + cols, dtype)
    return off, allr


def _canvas_io(imgs, device, stream, in_place, out_shape=None):
    """the pixels of an overlay call where they are to be worked on -> (source, output, device form?): numpy arrays, or torch tensors on
    the GPU allocated in the order of ``stream``; ``in_place`` makes the output the source (``out == in``)"""
    if device is None and not _is_dev(imgs):
        src = L.arr(imgs, np.uint8)
        return src, np.empty(out_shape or src.shape, np.uint8), False
    import torch
    with _stream_order(stream):
        src = imgs if _is_dev(imgs) else torch.as_tensor(L.arr(imgs, np.uint8)).to(device)
        out = src if in_place and out_shape is None else torch.empty(out_shape or tuple(src.shape), dtype=torch.uint8, device=src.device)
    return src, out, True


def DrawOverlays(imgs, prims, device=None, stream: int | None = None, in_place: bool = False):
    """``mvs_draw_overlays``: ``imgs`` [n, h, w, 3] uint8 with ``prims[i]`` (records of ``draw_prim``) painted on canvas i in list order
    (rules O1-O5 of include/mvs.h: discs, rings and thick segments, exact integer coverage, a later primitive over an earlier one), all
    canvases in one launch.  A numpy array -> a numpy array; with ``device`` (a torch device), or ``imgs`` a contiguous tensor there, ->
    a tensor (``mvs_draw_overlays_dev`` in the order of ``stream``; ``in_place`` paints into ``imgs`` itself)."""
    src, out, dev = _canvas_io(imgs, device, stream, in_place)
    if len(src.shape) != 4 or src.shape[3] != 3:
        raise L.MvsError(-1, "imgs must be [n, h, w, 3] uint8")
    n, h, w = (int(x) for x in src.shape[:3])
    off, flat = _lists(prims, n, L.DRAW_PRIM_DTYPE, (), "DrawOverlays")
    if not dev:
        L.check(L.lib().mvs_draw_overlays(n, w, h, L.ptr(src), L.ptr(off), L.ptr(flat), L.ptr(out)))
        return out
    with _stream_order(stream):
        L.check(L.lib().mvs_draw_overlays_dev(n, w, h, _dev_ptr(src, "uint8", "imgs"), L.ptr(off), L.ptr(flat), L.ptr(out), L.ptr(stream)))
    return out


def _match_lists(imgs1, imgs2, matches):
    n1, n2 = int(imgs1.shape[0]), int(imgs2.shape[0])
    if len(imgs1.shape) != 4 or imgs1.shape[3] != 3 or tuple(imgs1.shape[1:]) != tuple(imgs2.shape[1:]):
        raise L.MvsError(-1, "imgs1 and imgs2 must be [frames, h, w, 3] uint8 of one size")
    if len(matches) != n1 or any(len(row) != n2 for row in matches):
        raise L.MvsError(-1, "matches must be matches[i][j], one list per frame pair")
    off, flat = _lists([matches[i][j] for i in range(n1) for j in range(n2)], n1 * n2, np.int32, (4,), "matches")
    return n1, n2, int(imgs1.shape[1]), int(imgs1.shape[2]), off, flat


def _rng_state(rng_state):
    """None (a fresh default generator, NULL) or a one-element uint64 numpy array that the call advances"""
    if rng_state is None:
        return None
    if not isinstance(rng_state, np.ndarray) or rng_state.dtype != np.uint64 or rng_state.size != 1 or not rng_state.flags.c_contiguous:
        raise L.MvsError(-1, "rng_state must be None or a one-element uint64 numpy array (it receives the advanced state)")
    return rng_state


def MatchOverlays(imgs1, imgs2, matches, rng_state=None, device=None, stream: int | None = None):
    """``mvs_match_overlays``: the match pictures of R/Processor/Processor.cpp:767-793 for every frame pair of two adjacent sequences ->
    [n1 * n2, 2 h, w, 3] uint8, canvas i * n2 + j = ``imgs1[i]`` over ``imgs2[j]`` (BGR, [frames, h, w, 3]) with two rings and a line
    per match of ``matches[i][j]`` ((m, 4) int32 (u1, v1, u2, v2): what ``MatchFilterPairs`` returns), the line colours from one
    ``cv::RNG`` through all pairs (``rng_state``: None for a fresh one, or a one-element uint64 array that is advanced by 6 draws per
    match).  numpy in -> numpy out; with ``device``, or image tensors on the GPU, -> a tensor there (one launch stacks and draws)."""
    if _is_dev(imgs1) != _is_dev(imgs2):
        raise L.MvsError(-1, "imgs1 and imgs2 must both be tensors on the GPU or both arrays")
    dev = device is not None or _is_dev(imgs1)
    if not _is_dev(imgs1):
        imgs1, imgs2 = L.arr(imgs1, np.uint8), L.arr(imgs2, np.uint8)
    n1, n2, h, w, off, flat = _match_lists(imgs1, imgs2, matches)
    st = _rng_state(rng_state)
    if not dev:
        out = np.empty((n1 * n2, 2 * h, w, 3), np.uint8)
        L.check(L.lib().mvs_match_overlays(n1, n2, w, h, L.ptr(imgs1), L.ptr(imgs2), L.ptr(off), L.ptr(flat), L.ptr(st), L.ptr(out)))
        return out
    import torch
    with _stream_order(stream):
        a = imgs1 if _is_dev(imgs1) else torch.as_tensor(imgs1).to(device)
        b = imgs2 if _is_dev(imgs2) else torch.as_tensor(imgs2).to(device)
        out = torch.empty((n1 * n2, 2 * h, w, 3), dtype=torch.uint8, device=a.device)
        L.check(L.lib().mvs_match_overlays_dev(n1, n2, w, h, _dev_ptr(a, "uint8", "imgs1"), _dev_ptr(b, "uint8", "imgs2"), L.ptr(off), L.ptr(flat),
                                               L.ptr(st), L.ptr(out), L.ptr(stream)))
    return out


def SiftOverlays(views, keys, device=None, stream: int | None = None, in_place: bool = False):
    """``mvs_sift_overlays``: the SIFT pictures of R/FeatureProc/FeatureProc.cpp:67-69: ``views`` [n, h, w, 3] uint8 with a filled
    radius-1 mark in (0, 255, 0) at ``cvRound`` of the (x, y) of every key of ``keys[i]`` ((k, 4) float32 as ``DetectFeature`` returns
    them).  numpy, or torch tensors with ``device`` as ``DrawOverlays``."""
    src, out, dev = _canvas_io(views, device, stream, in_place)
    if len(src.shape) != 4 or src.shape[3] != 3:
        raise L.MvsError(-1, "views must be [n, h, w, 3] uint8")
    n, h, w = (int(x) for x in src.shape[:3])
    off, flat = _lists(keys, n, np.float32, (4,), "SiftOverlays")
    if not dev:
        L.check(L.lib().mvs_sift_overlays(n, w, h, L.ptr(src), L.ptr(off), L.ptr(flat), L.ptr(out)))
        return out
    with _stream_order(stream):
        L.check(L.lib().mvs_sift_overlays_dev(n, w, h, _dev_ptr(src, "uint8", "views"), L.ptr(off), L.ptr(flat), L.ptr(out), L.ptr(stream)))
    return out


def MatchOverlayFiles(match_dir, k: int, imgs1, imgs2, matches, rng_state=None, quality: int = 95, sampling="420", restart_interval: int = 0,
                      order: str = "BGR") -> None:
    """``mvs_processor_match_overlays``: the pictures of ``MatchOverlays`` for sequence pair ``k`` -> ``match_dir``match<k>_<i>_<j>.jpg
    (R/Processor/Processor.cpp:787; the reference's directory is ./Match/), the bytes ``EncodeJpegs`` returns for the canvases.  Drawn and
    encoded on the GPU in batches under MVS_OVERLAY_BATCH_BYTES; only the streams come back.  With ``order`` "RGB" the colours are
    written the other way round: the picture is the same."""
    imgs1, imgs2 = L.arr(imgs1, np.uint8), L.arr(imgs2, np.uint8)
    n1, n2, h, w, off, flat = _match_lists(imgs1, imgs2, matches)
    prm = jpeg_encode_params(quality=int(quality), sampling=_SAMPLING.get(sampling, -1), restart_interval=int(restart_interval))
    L.check(L.lib().mvs_processor_match_overlays(os.fsencode(match_dir), int(k), n1, n2, w, h, L.ptr(imgs1), L.ptr(imgs2), L.ptr(off), L.ptr(flat),
                                                 _jpeg_order(order), L.ptr(_rng_state(rng_state)), C.byref(prm)))


def SiftOverlayFiles(seq_dir, sub: str, views, keys, quality: int = 95, sampling="420", restart_interval: int = 0, order: str = "BGR") -> None:
    """``mvs_processor_sift_overlays``: ``views`` [frames, view_count, h, w, 3] with the marks of ``SiftOverlays`` for ``keys[i * view_count
    + j]`` -> ``seq_dir``Views/``sub``/proj<i>_<j>.jpg; ``sub`` is "Sift" (FeatureProc.cpp:67-73) or "Sift1" (after the background
    cull, Processor.cpp:604-615)."""
    v = L.arr(views, np.uint8)
    if v.ndim != 5 or v.shape[4] != 3:
        raise L.MvsError(-1, "views must be [frames, view_count, h, w, 3] uint8")
    f, vc, h, w = (int(x) for x in v.shape[:4])
    off, flat = _lists(keys, f * vc, np.float32, (4,), "SiftOverlayFiles")
    prm = jpeg_encode_params(quality=int(quality), sampling=_SAMPLING.get(sampling, -1), restart_interval=int(restart_interval))
    L.check(L.lib().mvs_processor_sift_overlays(os.fsencode(seq_dir), os.fsencode(sub), f, vc, w, h, L.ptr(v), L.ptr(off), L.ptr(flat),
                                                _jpeg_order(order), C.byref(prm)))


def LoadImages(seq_dirs, cameras, order: str = "BGR") -> list:
    """``mvs_processor_load_images``: camera i of sequence k from ``seq_dirs[k]``%05d.jpg (R/Processor/Processor.cpp:532) -> per sequence
    [frames, h, w, 3] uint8; the files are read on host threads and all sequences of one size are decoded in one call."""
    n = len(cameras)
    if len(seq_dirs) != n:
        raise L.MvsError(-1, f"{len(seq_dirs)} sequence dirs for {n} sequences")
    off, cams = L.seq_cams(cameras)
    dirs = (C.c_char_p * max(1, n))(*[os.fsencode(d) for d in seq_dirs])
    sizes = [sum(int(c.w) * int(c.h) * 3 for c in seq) for seq in cameras]
    flat = np.zeros(max(1, sum(sizes)), np.uint8)
    L.check(L.lib().mvs_processor_load_images(n, dirs, L.ptr(off), cams, _jpeg_order(order), L.ptr(flat)))
    res, at = [], 0
    for k, seq in enumerate(cameras):
        if len(seq) and any((int(c.w), int(c.h)) != (int(seq[0].w), int(seq[0].h)) for c in seq):
            raise L.MvsError(-1, f"the cameras of sequence {k} differ in size")
        shape = (len(seq), int(seq[0].h), int(seq[0].w), 3) if len(seq) else (0, 0, 0, 3)
        res.append(flat[at:at + sizes[k]].reshape(shape))
        at += sizes[k]
    return res


def LoadSequenceFiles(seq_dir, cameras, view_count: int, axis: int, rot_angle: float, **kw) -> dict:
    """``LoadSequenceModels`` from a sequence directory: the frames ``seq_dir``%05d.jpg (``LoadImages``, BGR as ``cv::imread``) and the
    checked rasters ``seq_dir``/DATA/CHECK/_depth<i>.raw (``mvs_depth_raw_read``) -> the ``sequences[k]`` entry of
    ``CalcSimilarityTransformationSeq``.  ``kw`` goes to ``LoadSequenceModels`` (sift, min_dsp, max_dsp, masks, segment, jpeg_quality)."""
    (imgs,) = LoadImages([seq_dir], [cameras], "BGR")
    depths = np.empty((len(cameras),) + tuple(imgs.shape[1:3]), np.float32)
    for i, cam in enumerate(cameras):
        path = os.path.join(os.fspath(seq_dir), "DATA", "CHECK", f"_depth{i}.raw")
        L.check(L.lib().mvs_depth_raw_read(os.fsencode(path), int(cam.w), int(cam.h), L.ptr(depths[i])))
    return LoadSequenceModels(cameras, imgs, depths, view_count, axis, rot_angle, **kw)


def RefineDepthFilesFromJpeg(seq_dirs, cameras, params: L.CDepthRefineParams | None = None) -> None:
    """``mvs_processor_refine_depths_files``: ``RefineDepthFiles`` with the RGB frames read from ``seq_dirs[k]``%05d.jpg."""
    n = len(cameras)
    if len(seq_dirs) != n:
        raise L.MvsError(-1, f"{len(seq_dirs)} sequence dirs for {n} sequences")
    off, cams = L.seq_cams(cameras)
    dirs = (C.c_char_p * max(1, n))(*[os.fsencode(d) for d in seq_dirs])
    prm = params if params is not None else depth_refine_params()
    L.check(L.lib().mvs_processor_refine_depths_files(n, dirs, L.ptr(off), cams, C.byref(prm)))
