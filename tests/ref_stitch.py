"""numpy checker of the stitch tail of Processor::AlignmentSeq (R/Processor/Processor.cpp:952-1105), built from oracle
primitives (O.srt_relative / O.srt_apply for the maps, O.vertex_normals(kind="plyobj"), O.retain_connect_region) and a
vectorised projection with camera_dev.h's operation order.  numpy never contracts a*b+c, so every value is the literal IEEE one."""
import numpy as np

from oracle import binding as O

INT_MIN = np.int32(-2147483648)


def cvt_i32(x):
    """(int)x as x86 cvttsd2si: truncation toward zero, NaN and out-of-range give INT_MIN."""
    x = np.asarray(x, np.float64)
    ok = (x > -2147483649.0) & (x < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), float(INT_MIN)).astype(np.int32)


def project(cam, p):
    """GetCamCoordFromWorld then GetImgCoordFromCam (R/Camera/Camera.cpp:45-48,68-72): (u, v) int32 per point."""
    R, t = np.asarray(cam.R, np.float64).reshape(9), np.asarray(cam.t, np.float64).reshape(3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        cx = ((R[0] * x + R[1] * y) + R[2] * z) + t[0]
        cy = ((R[3] * x + R[4] * y) + R[5] * z) + t[1]
        cz = ((R[6] * x + R[7] * y) + R[8] * z) + t[2]
        u = cvt_i32(cam.fx * cx / cz + cam.cx + 0.5)
        v = cvt_i32(cam.fy * cy / cz + cam.cy + 0.5)
    return u, v


def inside_all(cams, q, alive):
    """AND over the cameras of CheckRange(u, v, W, H) (R/Common/Utils.h:20-22), evaluated on the points still alive only."""
    for cam in cams:
        idx = np.flatnonzero(alive)
        if len(idx) == 0:
            break
        u, v = project(cam, q[idx])
        ok = (u >= 0) & (u < cam.w) & (v >= 0) & (v < cam.h)
        alive[idx[~ok]] = False
    return alive


def cull_sequences(pts_list, scales, Rs, ts, cameras):
    """:966-1004 — one mask per sequence; k0 == k is not mapped, k0 != k maps by srt_relative(k0, k) forward."""
    n = len(pts_list)
    masks = []
    for k in range(n):
        p = np.ascontiguousarray(pts_list[k], np.float64)
        alive = np.ones(len(p), bool)
        for k0 in range(n):
            if k0 == k:
                q = p
            else:
                s, R, t = O.srt_relative(scales[k0], Rs[k0], ts[k0], scales[k], Rs[k], ts[k])
                q, _ = O.srt_apply(p, None, s, R, t)
            alive = inside_all(cameras[k0], q, alive)
        masks.append(alive)
    return masks


def cull_all_seq(pts, scales, Rs, ts, cameras):
    """:1064-1083 — every k0 maps by the inverse (1/s_k0) R_k0^T (p - t_k0)."""
    p = np.ascontiguousarray(pts, np.float64)
    alive = np.ones(len(p), bool)
    for k0 in range(len(scales)):
        q, _ = O.srt_apply(p, None, scales[k0], Rs[k0], ts[k0], inverse=True)
        alive = inside_all(cameras[k0], q, alive)
    return alive


def stitch(pts_list, nrm_list, scales, Rs, ts, cameras, truncate=False):
    """:966-1027 — per sequence: the in-place compaction (kept points, then the untouched tail unless truncate), then
    s R p + t, R n.  -> (list of (points, normals), n_keep)."""
    masks = cull_sequences(pts_list, scales, Rs, ts, cameras)
    out, nk = [], []
    for k, m in enumerate(masks):
        p, n = np.asarray(pts_list[k], np.float64), np.asarray(nrm_list[k], np.float64)
        c = int(m.sum())
        if truncate:
            cp, cn = p[m], n[m]
        else:
            cp, cn = np.concatenate([p[m], p[c:]]), np.concatenate([n[m], n[c:]])
        wp, wn = O.srt_apply(np.ascontiguousarray(cp), np.ascontiguousarray(cn), scales[k], Rs[k], ts[k])
        out.append((wp, wn))
        nk.append(c)
    return out, np.array(nk, np.int64)


def cull_model(pts, nrm, faces, scales, Rs, ts, cameras, all_seq_proj=True):
    """:1057-1104 after ReadObj — normals computed when nrm is None, the AllSeqProj cull with the facet remap, then
    RetainConnectRegion.  -> (points, normals, faces)."""
    pts = np.ascontiguousarray(pts, np.float64)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    if nrm is None:
        nrm = O.vertex_normals(pts, faces, kind="plyobj")
    if all_seq_proj:
        keep = cull_all_seq(pts, scales, Rs, ts, cameras)
        new = np.full(len(pts), -1, np.int64)
        new[keep] = np.arange(int(keep.sum()))
        fk = keep[faces].all(1)
        faces = new[faces[fk]].astype(np.int32)
        pts, nrm = pts[keep], nrm[keep]
    return O.retain_connect_region(pts, nrm, faces)


def edge_points(cam, rng, n=400):
    """Camera-frame points whose u (or v) lands on w - 1 / w (h - 1 / h) to within a few ulps, z < 0, z = 0, NaN, 1e300 —
    taken back to the camera's world frame."""
    R, t = np.asarray(cam.R, np.float64).reshape(3, 3), np.asarray(cam.t, np.float64)
    pcs = []
    z = rng.uniform(0.5, 8.0, n)
    for edge_u in (cam.w - 1, cam.w, 0):
        x = (edge_u - cam.cx - 0.5) * z / cam.fx
        y = rng.uniform(-0.3, 0.3, n) * z
        for k in (-2, -1, 0, 1, 2):
            xx = x.copy()
            for _ in range(abs(k)):
                xx = np.nextafter(xx, np.sign(k) * np.inf)
            pcs.append(np.stack([xx, y, z], 1))
    for edge_v in (cam.h - 1, cam.h):
        y = (edge_v - cam.cy - 0.5) * z / cam.fy
        pcs.append(np.stack([rng.uniform(-0.3, 0.3, n) * z, y, z], 1))
        pcs.append(np.stack([rng.uniform(-0.3, 0.3, n) * z, np.nextafter(y, np.inf), z], 1))
    pcs.append(np.stack([rng.normal(size=n), rng.normal(size=n), -rng.uniform(0.1, 5, n)], 1))     # behind the camera
    pcs.append(np.stack([rng.normal(size=n), rng.normal(size=n), np.zeros(n)], 1))                  # on its plane
    pc = np.concatenate(pcs)
    p = (pc - t) @ R                                                                                 # R^T (pc - t)
    odd = np.array([[np.nan, 0, 5], [0, np.nan, 5], [np.inf, 0, 5], [1e300, 0, 5], [0, -1e300, 5], [1e300, 1e300, 1e300],
                    [0, 0, 0], [-1e300, 0, 1e-300]])
    return np.concatenate([p, pc, odd])
