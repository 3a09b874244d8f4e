"""numpy restatement of the depth-consistency filter, Processor::CheckConsistencyCore and Processor::CheckConsistency
(R/Processor/Processor.cpp:29-126) with the four camera maps of R/Camera/Camera.cpp:40-72, in the reference's order of operations and
in float64 on float32 rasters (LoadDepth widens them).  numpy never contracts a*b+c, so every value is the literal IEEE one.  Besides
the filtered raster it says, per pixel, which test decided and for which reference, and counts the projections that sat on an edge
of the double -> int rule.  A count is taken over the pixels still alive when the test was made, as the reference's `break` has it."""
import types

import numpy as np

from tests.ref_stitch import cvt_i32

OWN_RANGE, FWD_OUT, REF_RANGE, BACK_OUT, ERR_ABOVE, KEPT = range(6)
REASONS = ("own depth out of range", "forward projection outside the reference image", "reference depth out of range",
           "back projection outside the current image", "error above the threshold", "kept")
COUNTS = ("trunc_m1_0", "non_finite", "zc_zero", "zc_negative", "beyond_int32", "on_threshold")


def cvt_floor(x):
    """a WRONG rule: rounds down, so (-1, 0) becomes -1 where C truncation gives 0"""
    x = np.asarray(x, np.float64)
    ok = (x > -2147483649.0) & (x < 2147483648.0)
    return np.where(ok, np.floor(np.where(ok, x, 0.0)), -2147483648.0).astype(np.int32)


def cvt_bare(x):
    """a WRONG rule: what a bare (int)x does on the GPU, NaN becomes 0 and everything else saturates"""
    x = np.asarray(x, np.float64)
    return np.trunc(np.where(np.isnan(x), 0.0, np.clip(x, -2147483648.0, 2147483647.0))).astype(np.int32)


def check_range(u, v, w, h):
    """CheckRange (R/Common/Utils.h:20-22)"""
    return (u >= 0) & (u < w) & (v >= 0) & (v < h)


def world_from_img(cam, u, v, d):
    """GetCamCoordFromImg (Camera.cpp:40-44) then GetWorldCoordFromCam (:61-67): (x, y, z) of pixels (u, v) at depth d"""
    R, t = np.asarray(cam.R, np.float64).reshape(3, 3), np.asarray(cam.t, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        x = (u - float(cam.cx)) * d / float(cam.fx)
        y = (v - float(cam.cy)) * d / float(cam.fy)
        x, y, z = x - t[0], y - t[1], d - t[2]
        return ((R[0, 0] * x + R[1, 0] * y) + R[2, 0] * z,
                (R[0, 1] * x + R[1, 1] * y) + R[2, 1] * z,
                (R[0, 2] * x + R[1, 2] * y) + R[2, 2] * z)


def img_from_world(cam, p, counts, cvt=cvt_i32):
    """GetCamCoordFromWorld (:68-72) then GetImgCoordFromCam (:45-48) -> (u, v) int32; the edge classes of this projection are
    added to ``counts``"""
    R, t = np.asarray(cam.R, np.float64).reshape(3, 3), np.asarray(cam.t, np.float64).reshape(3)
    x, y, z = p
    with np.errstate(all="ignore"):
        xc = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
        yc = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
        zc = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]
        uf = float(cam.fx) * xc / zc + float(cam.cx) + 0.5
        vf = float(cam.fy) * yc / zc + float(cam.cy) + 0.5
        fin = np.isfinite(uf) & np.isfinite(vf)
        big = lambda a: np.isfinite(a) & ((a >= 2147483648.0) | (a <= -2147483649.0))
        counts["trunc_m1_0"] += int((((uf > -1) & (uf < 0)) | ((vf > -1) & (vf < 0))).sum())
        counts["non_finite"] += int((~fin).sum())
        counts["zc_zero"] += int((zc == 0).sum())
        counts["zc_negative"] += int((zc < 0).sum())
        counts["beyond_int32"] += int((big(uf) | big(vf)).sum())
    return cvt(uf), cvt(vf)


def check_core(depth, cur, ref_depths, ref_cams, min_dsp, max_dsp, reproj_err, cvt=cvt_i32):
    """Processor::CheckConsistencyCore (:66-115).  depth [h, w] float32 and one raster of the same size per reference.
    -> namespace(out float32 [h, w], reason int8 [h, w] (OWN_RANGE .. KEPT), ref int8 [h, w] (the deciding reference, -1 for
    OWN_RANGE and KEPT), counts dict over COUNTS, read = per reference the raster indices that live pixels landed on).  ``cvt`` is the double -> int rule; the
    host test passes wrong ones (cvt_floor, cvt_bare) to show that the scenes tell them from the right one."""
    w, h = int(cur.w), int(cur.h)
    dsp = np.asarray(depth, np.float32).reshape(h * w)
    mn, mx, thr = float(min_dsp), float(max_dsp), int(reproj_err)
    counts = dict.fromkeys(COUNTS, 0)
    reason = np.full(h * w, KEPT, np.int8)
    ref = np.full(h * w, -1, np.int8)
    read = []
    dp = dsp.astype(np.float64)
    with np.errstate(invalid="ignore"):
        own = (dp >= mn) & (dp <= mx)                                                     # :78
    reason[~own] = OWN_RANGE                                                              # :110-112
    alive = np.flatnonzero(own)
    i, j = alive % w, alive // w
    with np.errstate(all="ignore"):
        p3d = world_from_img(cur, i.astype(np.float64), j.astype(np.float64), 1.0 / dp[alive])   # :80

    def fall(sel, why, k):
        reason[alive[sel]] = why
        ref[alive[sel]] = k

    for k, (rd, rc) in enumerate(zip(ref_depths, ref_cams)):                              # :82
        rd = np.asarray(rd, np.float32).reshape(-1).astype(np.float64)
        u, v = img_from_world(rc, p3d, counts, cvt)                                            # :83
        ok = check_range(u, v, int(rc.w), int(rc.h))                                      # :84
        fall(~ok, FWD_OUT, k)                                                             # :104-107
        alive, i, j, u, v, p3d = alive[ok], i[ok], j[ok], u[ok], v[ok], tuple(c[ok] for c in p3d)
        read.append(v.astype(np.int64) * w + u)
        r = rd[read[-1]]                                                                  # the CURRENT width, :85
        with np.errstate(invalid="ignore"):
            ok = (r >= mn) & (r <= mx)
        fall(~ok, REF_RANGE, k)                                                           # :99-102
        alive, i, j, u, v, r, p3d = alive[ok], i[ok], j[ok], u[ok], v[ok], r[ok], tuple(c[ok] for c in p3d)
        with np.errstate(all="ignore"):
            q = world_from_img(rc, u.astype(np.float64), v.astype(np.float64), 1.0 / r)   # :87
        u, v = img_from_world(cur, q, counts, cvt)                                             # :88
        ok = check_range(u, v, w, h)                                                      # :89
        fall(~ok, BACK_OUT, k)
        alive, i, j, u, v, p3d = alive[ok], i[ok], j[ok], u[ok], v[ok], tuple(c[ok] for c in p3d)
        du, dv = i - u.astype(np.int64), j - v.astype(np.int64)
        sq = du * du + dv * dv
        counts["on_threshold"] += int((sq == thr * thr).sum())
        ok = ~(np.sqrt(sq.astype(np.float64)) > thr)                                      # :93-94
        fall(~ok, ERR_ABOVE, k)
        alive, i, j, p3d = alive[ok], i[ok], j[ok], tuple(c[ok] for c in p3d)
    out = np.where(reason == KEPT, dsp, np.float32(0.0)).astype(np.float32)               # `dp = 0.0f`: +0
    return types.SimpleNamespace(out=out.reshape(h, w), reason=reason.reshape(h, w), ref=ref.reshape(h, w), counts=counts, read=read)


def neighbours(i, n):
    """the reference frames of frame i of n (:49-55): i - 1 then i + 1, those that exist"""
    return [idx for idx in (i - 1, i, i + 1) if 0 <= idx < n and idx != i]


def check_seq(depths, cams, min_dsp, max_dsp, reproj_err):
    """Processor::CheckConsistency for one sequence (:42-57): every frame against its neighbours' ORIGINAL rasters.
    -> (out float32 [n, h, w], the per-frame results of check_core)"""
    depths = np.asarray(depths, np.float32)
    n = len(cams)
    res = [check_core(depths[i], cams[i], [depths[k] for k in neighbours(i, n)], [cams[k] for k in neighbours(i, n)], min_dsp, max_dsp,
                      reproj_err) for i in range(n)]
    return np.stack([r.out for r in res]), res
