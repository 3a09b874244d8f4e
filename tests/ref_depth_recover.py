"""numpy restatement of mvs_recover_depth_maps (include/mvs.h), written from its rules R1-R9: every floating-point operation is an fp64
+ - * / sqrt on numpy arrays in the order the rules state, every sum of squared grey differences an exact int64.  The grey conversion,
the reference frames and the camera maps are those of tests/ref_depth_refine.py.  R6 is stated here on the whole cost table of a pixel —
the first level that reaches the smallest mean, the first that reaches the largest — not as the single ascending pass of
csrc/depth_recover_rules.h, and no level reuses the sum of the one before it.  Besides the result ``recover`` returns the cost tables of
every level and the smallest margin of every kind of decision an fp64 operation feeds: ``coord`` (a projected coordinate against the next
integer), ``z`` (|Xc.z|), ``accept`` (R7's root mean square against ssd_err, relative), ``peak`` (R7's m against peak * m_W, relative to
the latter; a flat curve of zeros compares two exact zeros and has no margin), ``range`` (the substep's d against dsp_min and dsp_max) and
``nudge`` (an accepted d that is not a level end against dsp_min and dsp_max: the distance R9's float32 rounding would have to cross)."""
import numpy as np

from tests.ref_depth_refine import Margins, cam_from_world, cvt_i32, grey, references, world_from_img

SUBSTEP = 1
NONE = -1


def params(dsp_min=0.0025, dsp_max=0.3, ssd_err=40.0, peak=0.9, ssd_win=7, ref_frm_count=5, levels=128, min_refs=2, flags=SUBSTEP, reserved=0):
    return dict(dsp_min=dsp_min, dsp_max=dsp_max, ssd_err=ssd_err, peak=peak, ssd_win=ssd_win, ref_frm_count=ref_frm_count, levels=levels,
                min_refs=min_refs, flags=flags, reserved=reserved)


def level_values(p):
    """R4 -> (d_l for l = 0 .. L - 1 as a list of floats, step)"""
    L = p["levels"]
    step = (p["dsp_max"] - p["dsp_min"]) / float(L - 1)
    return [p["dsp_min"] + float(l) * step for l in range(L - 1)] + [p["dsp_max"]], step


def costs_at(cams, G, f, uu, vv, ds, N, ref_frm_count, mg):
    """R5 for the pixels (uu, vv) of frame f at the disparities ds (a list; each a float or an array per pixel) -> (sums [len(ds), m]
    int64, cnts [len(ds), m] int64, how often Xc.z <= 0 (``behind``) or a landing pixel lay outside the interior (``outside``), and per
    pixel the smallest ``coord`` and ``z`` margin of its own decisions [m])"""
    n, h, w = G.shape
    m = len(uu)
    sums, cnts = np.zeros((len(ds), m), np.int64), np.zeros((len(ds), m), np.int64)
    Gi = G.astype(np.int64)
    ab = np.arange(-N, N + 1)
    cur = Gi[f][vv[:, None, None] + ab[None, :, None], uu[:, None, None] + ab[None, None, :]]                # [m, len, len]
    seen = dict(behind=0, outside=0)
    own = np.full(m, np.inf)
    with np.errstate(all="ignore"):
        for l, dl in enumerate(ds):
            P = world_from_img(cams[f], uu, vv, 1.0 / (dl + np.zeros(m)))
            for g in references(f, n, ref_frm_count):
                c = cams[g]
                xc = cam_from_world(c, P)
                zpos = xc[2] > 0.0
                mg.see("z", np.abs(xc[2]))
                own = np.minimum(own, np.abs(xc[2]))
                fu, fv = c.fx * xc[0] / xc[2] + c.cx + 0.5, c.fy * xc[1] / xc[2] + c.cy + 0.5
                for q in (fu, fv):
                    dist = np.abs(q - np.round(q))
                    mg.see("coord", dist[zpos])
                    own = np.where(zpos, np.minimum(own, dist), own)
                u2, v2 = cvt_i32(fu), cvt_i32(fv)
                ok = zpos & (u2 >= N) & (u2 < w - N) & (v2 >= N) & (v2 < h - N)
                seen["behind"] += int((~zpos).sum())
                seen["outside"] += int((zpos & ~ok).sum())
                ref = Gi[g][v2[ok][:, None, None] + ab[None, :, None], u2[ok][:, None, None] + ab[None, None, :]]
                df = cur[ok] - ref
                sums[l, ok] += (df * df).sum(axis=(1, 2))
                cnts[l, ok] += 1
    return sums, cnts, seen, own


def choose(sums, cnts, min_refs):
    """R6 -> (l* [m], W [m], any eligible [m]); l* and W are 0 where nothing is eligible"""
    L, m = sums.shape
    elig = cnts >= min_refs
    best, worst = np.zeros(m, np.int64), np.zeros(m, np.int64)
    have = np.zeros(m, bool)
    bs, bc, ws, wc = (np.zeros(m, np.int64) for _ in range(4))
    for l in range(L):
        s, c, e = sums[l], cnts[l], elig[l]
        lower = e & (~have | (s * bc < bs * c))
        higher = e & (~have | (ws * c < s * wc))
        best, bs, bc = np.where(lower, l, best), np.where(lower, s, bs), np.where(lower, c, bc)
        worst, ws, wc = np.where(higher, l, worst), np.where(higher, s, ws), np.where(higher, c, wc)
        have |= e
    return best, worst, have


def value(d, p):
    """R9: float64 [m] -> float32 [m]"""
    out = d.astype(np.float32)
    up, down = np.nextafter(out, np.float32(np.inf)), np.nextafter(out, np.float32(-np.inf))
    wide = out.astype(np.float64)
    return np.where(wide < p["dsp_min"], up, np.where(wide > p["dsp_max"], down, out)).astype(np.float32)


def recover_frame(cams, G, f, p, mg, tables=None, only=None):
    """R3-R9 for frame f -> dict(out float32 [h, w], level int16, sum int32, cnt uint8, cand bool, sums, cnts, at = (vv, uu), ...).
    ``tables`` is the entry of that name of an earlier result for the same frame, levels, window and references: R5 is not run again.
    ``only`` (bool [h, w]) limits the work to some pixels; the others are reported as non-candidates"""
    n, h, w = G.shape
    N, L = p["ssd_win"], p["levels"]
    vv, uu = np.mgrid[0:h, 0:w]
    cand = (uu >= N) & (uu < w - N) & (vv >= N) & (vv < h - N)                                                      # R3
    if only is not None:
        cand &= only
    out = np.zeros((h, w), np.float32)
    ll, ss, cc = np.full((h, w), NONE, np.int16), np.full((h, w), -1, np.int32), np.zeros((h, w), np.uint8)
    vv, uu = vv[cand], uu[cand]
    dls, step = level_values(p)
    if tables is None:
        own_mg = Margins()
        tables = costs_at(cams, G, f, uu, vv, dls, N, p["ref_frm_count"], own_mg) + (own_mg,)
    sums, cnts, seen, own, own_mg = tables
    for kind, least in own_mg.items():
        mg.see(kind, least)
    best, worst, any_l = choose(sums, cnts, p["min_refs"])
    idx = np.arange(len(uu))
    bs, bc, ws, wc = sums[best, idx], cnts[best, idx], sums[worst, idx], cnts[worst, idx]
    with np.errstate(all="ignore"):
        m = bs.astype(np.float64) / bc.astype(np.float64)
        mw = ws.astype(np.float64) / wc.astype(np.float64)
        rms = np.sqrt(m / float((2 * N + 1) * (2 * N + 1)))
        if p["ssd_err"] > 0:
            mg.see("accept", (np.abs(rms - p["ssd_err"]) / p["ssd_err"])[any_l])
        bar = p["peak"] * mw
        mg.see("peak", (np.abs(m - bar) / bar)[any_l & (ws > 0)])
        acc = any_l & (rms <= p["ssd_err"]) & (m < bar)                                                             # R7
        d = np.asarray(dls)[best]
        if p["flags"] & SUBSTEP:                                                                                    # R8
            lo, hi = np.clip(best - 1, 0, L - 1), np.clip(best + 1, 0, L - 1)
            both = any_l & (best - 1 >= 0) & (best + 1 <= L - 1) & (cnts[lo, idx] >= p["min_refs"]) & (cnts[hi, idx] >= p["min_refs"])
            cm = sums[lo, idx].astype(np.float64) / cnts[lo, idx].astype(np.float64)
            cp = sums[hi, idx].astype(np.float64) / cnts[hi, idx].astype(np.float64)
            den = (cm - 2.0 * m) + cp
            o = 0.5 * ((cm - cp) / den)
            ds = p["dsp_min"] + (best.astype(np.float64) + o) * step
            tried = both & (den > 0.0)
            mg.see("range", np.minimum(np.abs(ds - p["dsp_min"]), np.abs(ds - p["dsp_max"]))[tried & acc])
            use = tried & (ds >= p["dsp_min"]) & (ds <= p["dsp_max"])
            d = np.where(use, ds, d)
            offset = np.where(use, o, 0.0)
        else:
            offset = np.zeros(len(uu))
        inner = acc & (d != p["dsp_min"]) & (d != p["dsp_max"])
        mg.see("nudge", np.minimum(np.abs(d - p["dsp_min"]), np.abs(d - p["dsp_max"]))[inner])
        val = value(d, p)                                                                                           # R9
    out[cand] = np.where(acc, val, np.float32(0.0))
    ll[cand] = np.where(acc, best, NONE).astype(np.int16)
    ss[cand] = np.where(any_l, bs, -1).astype(np.int32)
    cc[cand] = np.where(any_l, bc, 0).astype(np.uint8)
    return dict(out=out, level=ll, sum=ss, cnt=cc, cand=cand, sums=sums, cnts=cnts, at=(vv, uu), best=best, worst=worst, any=any_l, offset=offset,
                accepted=acc, seen=seen, own=own, d=d, tables=tables)


def recover_sequence(cams, imgs, p, earlier=None):
    """one sequence: cams[n], imgs [n, h, w, 3] uint8 -> dict(out, level, sum, cnt [n, h, w], frames, margins); ``earlier`` is a result
    for the same sequence whose parameters differ only in flags, peak, ssd_err or min_refs: its cost tables are used again"""
    n = len(cams)
    mg = Margins()
    shape = tuple(np.asarray(imgs).shape[:3])
    if n == 0:
        return dict(out=np.zeros(shape, np.float32), level=np.zeros(shape, np.int16), sum=np.zeros(shape, np.int32), cnt=np.zeros(shape, np.uint8),
                    frames=[], margins=mg)
    G = grey(imgs)                                                                                                 # R1
    frames = [recover_frame(cams, G, f, p, mg, earlier["frames"][f]["tables"] if earlier else None) for f in range(n)]
    res = {key: np.stack([fr[key] for fr in frames]) for key in ("out", "level", "sum", "cnt")}
    res.update(frames=frames, margins=mg)
    return res


def recover(cameras, imgs, p, earlier=None):
    """``cameras[k]`` / ``imgs[k]`` per sequence -> a list of recover_sequence results: a sequence does not see another"""
    return [recover_sequence(c, i, p, earlier[k] if earlier else None) for k, (c, i) in enumerate(zip(cameras, imgs))]
