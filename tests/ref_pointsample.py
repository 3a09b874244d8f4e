"""numpy restatement of mvs_point_sample (include/mvs.h), written from its eight rules: every operation is an fp64 + - * / sqrt on numpy
arrays in the order the rules state.  The camera maps are explicit sums and products (no ``@``, ``np.dot`` or ``np.linalg.norm``: BLAS may
fuse or reorder).  Besides the result ``sample`` returns diagnostics: the pixels surviving rules 1, 2, 3, 5 and the cells of rule 6, the
cells coverage suppressed, the in-range coverage projections that rule 4 rejected, and the smallest margin of every kind of decision
that an fp64 operation feeds (rules 1 and the validity of rule 4 compare a float32 widened exactly: no operation, no margin)."""
import numpy as np

INT_MIN = -2 ** 31


def params(dsp_min=0.0025, dsp_max=0.3, max_dsp_err=0.01, min_conf=0.9, edge_sz_thres=4.0, pt_samp_rds=2, nbr_frm_num=2, nbr_frm_step=1):
    return dict(dsp_min=dsp_min, dsp_max=dsp_max, max_dsp_err=max_dsp_err, min_conf=min_conf, edge_sz_thres=edge_sz_thres,
                pt_samp_rds=pt_samp_rds, nbr_frm_num=nbr_frm_num, nbr_frm_step=nbr_frm_step)


def cvt_i32(x):
    """the double -> int rule: truncation toward zero, INT_MIN for NaN, infinities and values outside int32"""
    x = np.asarray(x, np.float64)
    ok = (x > -2147483649.0) & (x < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), INT_MIN).astype(np.int64)


def _cam(c):
    return [float(v) for v in np.asarray(c.R, np.float64).reshape(9)], [float(v) for v in np.asarray(c.t, np.float64).reshape(3)]


def world_from_img(c, u, v, z):
    R, t = _cam(c)
    px, py, pz = (u - c.cx) * z / c.fx, (v - c.cy) * z / c.fy, z
    tx, ty, tz = px - t[0], py - t[1], pz - t[2]
    return ((R[0] * tx + R[3] * ty) + R[6] * tz, (R[1] * tx + R[4] * ty) + R[7] * tz, (R[2] * tx + R[5] * ty) + R[8] * tz)


def cam_from_world(c, P):
    R, t = _cam(c)
    x, y, z = P
    return (((R[0] * x + R[1] * y) + R[2] * z) + t[0], ((R[3] * x + R[4] * y) + R[5] * z) + t[1], ((R[6] * x + R[7] * y) + R[8] * z) + t[2])


def length(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


class Margins(dict):
    def see(self, kind, values):
        values = np.asarray(values, np.float64)
        values = values[np.isfinite(values)]
        if values.size:
            self[kind] = min(self.get(kind, np.inf), float(values.min()))


def agrees(P, cam, raster, p, mg):
    """rule 4 for the points P = (x, y, z) arrays -> (agree, u', v', in_img); u', v' are meaningful where Xc.z > 0"""
    with np.errstate(all="ignore"):
        xc = cam_from_world(cam, P)
        zpos = xc[2] > 0.0
        mg.see("z", np.abs(xc[2]) / length(*xc))
        fu, fv = cam.fx * xc[0] / xc[2] + cam.cx + 0.5, cam.fy * xc[1] / xc[2] + cam.cy + 0.5
        for c in (fu[zpos], fv[zpos]):
            mg.see("coord", np.abs(c - np.round(c)))
        u, v = cvt_i32(fu), cvt_i32(fv)
        in_img = zpos & (u >= 0) & (u < cam.w) & (v >= 0) & (v < cam.h)
        dg = np.zeros(len(u))
        dg[in_img] = raster[v[in_img], u[in_img]].astype(np.float64)
        valid = in_img & (dg >= p["dsp_min"]) & (dg <= p["dsp_max"])
        diff = np.abs(dg - 1.0 / xc[2])
        if p["max_dsp_err"] > 0:
            mg.see("dsp", np.abs(diff[valid] - p["max_dsp_err"]) / p["max_dsp_err"])
        return valid & (diff <= p["max_dsp_err"]), u, v, in_img


def frame_rules(cams, depths, f, p, mg, counts):
    """rules 1-3 and 5 for every pixel of frame f -> (passes [h, w] bool, P [3][h, w], N [3][h, w])"""
    c = cams[f]
    h, w = depths[f].shape
    d = depths[f].astype(np.float64)
    valid = (d >= p["dsp_min"]) & (d <= p["dsp_max"])                                  # rule 1
    counts["valid"] += int(valid.sum())
    vv, uu = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        z = 1.0 / d
        P = world_from_img(c, uu, vv, z)
        ok = np.zeros((h, w), bool)                                                    # rule 2
        ok[1:-1, 1:-1] = valid[1:-1, 1:-1] & valid[1:-1, :-2] & valid[1:-1, 2:] & valid[:-2, 1:-1] & valid[2:, 1:-1]
        counts["neighbours"] += int(ok.sum())
        sh = lambda a, dv, du: np.roll(np.roll(a, -dv, 0), -du, 1)                    # a[v + dv, u + du]; the rolled border is never ok
        Pl, Pr = tuple(sh(a, 0, -1) for a in P), tuple(sh(a, 0, 1) for a in P)
        Pu, Pd = tuple(sh(a, -1, 0) for a in P), tuple(sh(a, 1, 0) for a in P)
        lim_x, lim_y = p["edge_sz_thres"] * (z / abs(c.fx)), p["edge_sz_thres"] * (z / abs(c.fy))     # rule 3
        keep = ok.copy()
        for Q, lim in ((Pl, lim_x), (Pr, lim_x), (Pu, lim_y), (Pd, lim_y)):
            ln = length(*sub(Q, P))
            mg.see("edge", (np.abs(ln - lim) / lim)[ok])
            keep &= ~(ln > lim)
        a, b = sub(Pr, Pl), sub(Pd, Pu)
        n = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
        ln = length(*n)
        mg.see("len", (ln / (length(*a) * length(*b)))[keep])
        keep &= ln > 0.0
        n = (n[0] / ln, n[1] / ln, n[2] / ln)
        zero = np.zeros(1)
        C = world_from_img(c, zero, zero, zero)
        e = sub(P, (C[0][0], C[1][0], C[2][0]))
        dot = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        mg.see("flip", (np.abs(dot) / length(*e))[keep])
        flip = dot > 0.0
        n = tuple(np.where(flip, -q, q) for q in n)
    counts["edge"] += int(keep.sum())
    reach = min(p["nbr_frm_num"], (len(cams) - 1) // p["nbr_frm_step"])              # rule 5: no j beyond this gives a frame of the sequence
    nbrs = [f + s * j * p["nbr_frm_step"] for j in range(1, reach + 1) for s in (-1, 1)]
    nbrs = [g for g in nbrs if 0 <= g < len(cams)]
    passes = keep.copy()
    if nbrs:
        sel = np.nonzero(keep)
        Ps = tuple(q[sel] for q in P)
        agree = np.zeros(len(sel[0]), np.int64)
        for g in nbrs:
            agree += agrees(Ps, cams[g], depths[g], p, mg)[0]
        need = p["min_conf"] * float(len(nbrs))
        if need > 0:
            mg.see("conf", np.abs(agree.astype(np.float64) - need) / need)
        passes[sel] = agree.astype(np.float64) >= need
    counts["confidence"] += int(passes.sum())
    return passes, P, n


def sample_sequence(cams, depths, p):
    """one sequence: cams[n], depths [n, h, w] float32 -> dict(points, normals, frame, pixel, cand [n, ch * cw], counts, margins)"""
    n = len(cams)
    mg = Margins()
    counts = dict(valid=0, neighbours=0, edge=0, confidence=0, candidates=0, suppressed=0, emitted=0, cover_rejected=0)
    if n == 0:
        return dict(points=np.zeros((0, 3)), normals=np.zeros((0, 3)), frame=np.zeros(0, np.int32), pixel=np.zeros(0, np.int32),
                    cand=np.zeros((0, 0), np.int32), counts=counts, margins=mg)
    h, w = depths[0].shape
    r = p["pt_samp_rds"]
    ch, cw = -(-h // r), -(-w // r)
    big = np.iinfo(np.int64).max
    cand = np.full((n, ch, cw), -1, np.int64)
    geo = []
    for f in range(n):
        passes, P, N = frame_rules(cams, depths, f, p, mg, counts)
        geo.append((P, N))
        idx = np.where(passes, np.arange(h * w, dtype=np.int64).reshape(h, w), big)
        pad = np.full((ch * r, cw * r), big, np.int64)
        pad[:h, :w] = idx
        best = pad.reshape(ch, r, cw, r).min(axis=(1, 3))                              # rule 6: the lowest row-major index of the cell
        cand[f] = np.where(best == big, -1, best)
    counts["candidates"] = int((cand >= 0).sum())
    cover = np.zeros((n, ch, cw), bool)
    out = dict(points=[], normals=[], frame=[], pixel=[])
    for f in range(n):                                                                 # rule 7
        emit = (cand[f] >= 0) & ~cover[f]
        counts["suppressed"] += int(((cand[f] >= 0) & cover[f]).sum())
        px = np.sort(cand[f][emit])                                                    # rule 8: pixel index ascending
        v, u = px // w, px % w
        P, N = geo[f]
        Ps = tuple(q[v, u] for q in P)
        out["points"].append(np.stack(Ps, 1))
        out["normals"].append(np.stack([q[v, u] for q in N], 1))
        out["frame"].append(np.full(len(px), f, np.int32))
        out["pixel"].append(px.astype(np.int32))
        for g in range(f + 1, n):
            ok, gu, gv, in_img = agrees(Ps, cams[g], depths[g], p, mg)
            counts["cover_rejected"] += int((in_img & ~ok).sum())
            cover[g, gv[ok] // r, gu[ok] // r] = True
    counts["emitted"] = int(sum(len(a) for a in out["pixel"]))
    res = {k: np.concatenate(a) for k, a in out.items()}
    res.update(cand=cand.reshape(n, ch * cw).astype(np.int32), counts=counts, margins=mg)
    return res


def sample(cameras, depths, p):
    """``cameras[k]`` / ``depths[k]`` per sequence -> a list of sample_sequence results: a sequence does not see another sequence"""
    return [sample_sequence(c, d, p) for c, d in zip(cameras, depths)]
