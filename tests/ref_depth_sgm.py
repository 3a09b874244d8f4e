"""numpy restatement of mvs_recover_depth_maps_aggregated (include/mvs.h), written from its rules S1-S6 on top of the per-level cost tables
``sums``/``cnts`` that tests/ref_depth_recover.py builds for every frame (R1-R5).  The volume C of a frame is one int64 array
[L, rh, rw] over the rectangle; a path direction is walked as whole-array steps — a column of the rectangle at a time for (±1, 0), a row at a
time for every other direction, the row before it moved by dx — and S is the plain sum of the directions.  Nothing here follows the
kernels' lines, lanes or launches.  Besides the result ``aggregate`` returns the smallest margin of every fp64-fed decision: ``coord`` and
``z`` (R5, from the tables), ``accept`` and ``peak`` (S4's two tests, relative as in ref_depth_recover), ``range`` (S5's d against dsp_min
and dsp_max) and ``nudge`` (R9)."""
import numpy as np

from tests import ref_depth_recover as R
from tests.ref_depth_refine import Margins

SUBSTEP, NONE = R.SUBSTEP, R.NONE
DIRECTIONS = {4: ((1, 0), (-1, 0), (0, 1), (0, -1)),
              8: ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))}
FAR = 1 << 40          # a level outside [0, L - 1]: it never wins a minimum


def aparams(p1=8, p2=128, cost_cap=255, paths=8, max_volume_mb=0, reserved=0):
    return dict(p1=p1, p2=p2, cost_cap=cost_cap, paths=paths, max_volume_mb=max_volume_mb, reserved=reserved)


def volume(sums, cnts, p, a, rh, rw):
    """S1 -> C int64 [L, rh, rw]"""
    n_len = 2 * p["ssd_win"] + 1
    elig = cnts >= p["min_refs"]
    den = np.where(elig, cnts, 1) * n_len * n_len
    C = np.where(elig, np.minimum(a["cost_cap"], sums // den), a["cost_cap"])
    return C.reshape(len(sums), rh, rw)


def _step(C, prev, a):
    """one step of S2 on whole arrays: C [L, m] at the pixels p, prev = L_r [L, m] at q = p - r"""
    M = prev.min(axis=0, keepdims=True)
    far = np.full_like(prev[:1], FAR)
    below = np.concatenate([far, prev[:-1]])          # L_r(q, l - 1)
    above = np.concatenate([prev[1:], far])           # L_r(q, l + 1)
    return C + np.minimum(np.minimum(prev, M + a["p2"]), np.minimum(below, above) + a["p1"]) - M


def path(C, dx, dy, a):
    """S2 for the direction r = (dx, dy) -> L_r int64 [L, rh, rw]"""
    L, rh, rw = C.shape
    Lr = np.empty_like(C)
    if dy == 0:
        xs = range(rw) if dx > 0 else range(rw - 1, -1, -1)
        for i, x in enumerate(xs):
            Lr[:, :, x] = C[:, :, x] if i == 0 else _step(C[:, :, x], Lr[:, :, x - dx], a)
        return Lr
    ys = range(rh) if dy > 0 else range(rh - 1, -1, -1)
    xx = np.arange(rw)
    inside = (xx - dx >= 0) & (xx - dx < rw)           # q = (x - dx, y - dy) lies in the rectangle (the row does)
    for i, y in enumerate(ys):
        if i == 0:
            Lr[:, y] = C[:, y]
            continue
        prev = Lr[:, y - dy][:, np.clip(xx - dx, 0, rw - 1)]
        Lr[:, y] = np.where(inside[None], _step(C[:, y], prev, a), C[:, y])
    return Lr


def aggregate_frame(fr, p, a, mg, shape):
    """S1-S6 for one frame from ``fr``, its result of ref_depth_recover.recover_frame -> dict(out, level, sum, cnt, agg [h, w], C, S, Lmax)"""
    h, w = shape
    N, L = p["ssd_win"], p["levels"]
    rh, rw = max(0, h - 2 * N), max(0, w - 2 * N)
    out = np.zeros((h, w), np.float32)
    ll, ss, cc, aa = np.full((h, w), NONE, np.int16), np.full((h, w), -1, np.int32), np.zeros((h, w), np.uint8), np.full((h, w), -1, np.int32)
    res = dict(out=out, level=ll, sum=ss, cnt=cc, agg=aa, cand=fr["cand"], C=None, S=None, Lmax=0)
    if rh == 0 or rw == 0:
        return res
    sums, cnts = fr["sums"], fr["cnts"]
    for kind, least in fr["tables"][4].items():                                            # coord and z: the margins of R5
        mg.see(kind, least)
    C = volume(sums, cnts, p, a, rh, rw)
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS[a["paths"]]:
        Lr = path(C, dx, dy, a)
        res["Lmax"] = max(res["Lmax"], int(Lr.max()))
        S += Lr
    S2 = S.reshape(L, rh * rw)
    best = S2.argmin(axis=0)                                                               # S3: the first of the smallest
    idx = np.arange(rh * rw)
    _, worst, any_l = R.choose(sums, cnts, p["min_refs"])
    bs, bc, ws, wc = sums[best, idx], cnts[best, idx], sums[worst, idx], cnts[worst, idx]
    elig = bc >= p["min_refs"]
    dls, step = R.level_values(p)
    with np.errstate(all="ignore"):
        m = bs.astype(np.float64) / bc.astype(np.float64)
        mw = ws.astype(np.float64) / wc.astype(np.float64)
        rms = np.sqrt(m / float((2 * N + 1) * (2 * N + 1)))
        if p["ssd_err"] > 0:
            mg.see("accept", (np.abs(rms - p["ssd_err"]) / p["ssd_err"])[elig])
        bar = p["peak"] * mw
        mg.see("peak", (np.abs(m - bar) / bar)[elig & (ws > 0)])
        acc = elig & (rms <= p["ssd_err"]) & (m < bar)                                     # S4
        d = np.asarray(dls)[best]
        if p["flags"] & SUBSTEP:                                                           # S5
            both = (best - 1 >= 0) & (best + 1 <= L - 1)
            lo, hi = np.clip(best - 1, 0, L - 1), np.clip(best + 1, 0, L - 1)
            cm, c0, cp = S2[lo, idx].astype(np.float64), S2[best, idx].astype(np.float64), S2[hi, idx].astype(np.float64)
            den = (cm - 2.0 * c0) + cp
            o = 0.5 * ((cm - cp) / den)
            ds = p["dsp_min"] + (best.astype(np.float64) + o) * step
            tried = both & (den > 0.0)
            mg.see("range", np.minimum(np.abs(ds - p["dsp_min"]), np.abs(ds - p["dsp_max"]))[tried & acc])
            d = np.where(tried & (ds >= p["dsp_min"]) & (ds <= p["dsp_max"]), ds, d)
        inner = acc & (d != p["dsp_min"]) & (d != p["dsp_max"])
        mg.see("nudge", np.minimum(np.abs(d - p["dsp_min"]), np.abs(d - p["dsp_max"]))[inner])
        val = R.value(d, p)                                                                # S6
    cand = fr["cand"]
    out[cand] = np.where(acc, val, np.float32(0.0))
    ll[cand] = np.where(acc, best, NONE).astype(np.int16)
    ss[cand] = np.where(elig, bs, -1).astype(np.int32)
    cc[cand] = np.where(elig, bc, 0).astype(np.uint8)
    aa[cand] = S2[best, idx].astype(np.int32)
    res.update(C=C, S=S, best=best.reshape(rh, rw), accepted=acc)
    return res


def aggregate(plain, imgs, p, a):
    """``plain``: the list ref_depth_recover.recover returned for the same sequences, images and R-parameters (flags, peak and ssd_err may
    differ: S4-S6 read them from ``p``) -> per sequence dict(out, level, sum, cnt, agg [n, h, w], frames, margins)"""
    res = []
    for seq, im in zip(plain, imgs):
        mg = Margins()
        shape = tuple(np.asarray(im).shape[1:3])
        frames = [aggregate_frame(fr, p, a, mg, shape) for fr in seq["frames"]]
        n = len(frames)
        r = {key: (np.stack([fr[key] for fr in frames]) if n else np.zeros((0,) + shape, dt))
             for key, dt in (("out", np.float32), ("level", np.int16), ("sum", np.int32), ("cnt", np.uint8), ("agg", np.int32))}
        r.update(frames=frames, margins=mg)
        res.append(r)
    return res
