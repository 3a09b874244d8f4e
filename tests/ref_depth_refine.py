"""numpy restatement of mvs_refine_depth_maps (include/mvs.h), written from its nine rules: every floating-point operation is an fp64
+ - * / sqrt on numpy arrays in the order the rules state, every sum of squared grey differences an exact int64.  The camera maps are those
of tests/ref_pointsample.py (explicit sums and products).  Rule 6 is stated here as a walk over the hypotheses in the order of preference
(0, -1, 1, -2, 2, ...) in which a later one replaces the best only when it is strictly better — not the single ascending pass of
csrc/depth_refine_rules.h.  Besides the result ``refine`` returns the cost tables of every hypothesis and the smallest margin of every
kind of decision an fp64 operation feeds: ``coord`` (a projected coordinate against the next integer), ``z`` (|Xc.z|), ``bound`` (a
hypothesis d_k, k != 0, against dsp_min and dsp_max) and ``accept`` (rule 7's root mean square against ssd_err, relative)."""
import numpy as np

from tests.ref_pointsample import Margins, cam_from_world, cvt_i32, world_from_img

SUBSTEP = 1
NONE = -128


def params(dsp_min=0.0025, dsp_max=0.3, rel_range=0.04, ssd_err=40.0, ssd_win=7, ref_frm_count=5, steps=8, flags=SUBSTEP):
    return dict(dsp_min=dsp_min, dsp_max=dsp_max, rel_range=rel_range, ssd_err=ssd_err, ssd_win=ssd_win, ref_frm_count=ref_frm_count,
                steps=steps, flags=flags)


def grey(img):
    """rule 1: [..., 3] uint8 -> [...] uint8"""
    p = np.asarray(img, np.uint8).astype(np.int64)
    return ((4899 * p[..., 0] + 9617 * p[..., 1] + 1868 * p[..., 2] + 8192) >> 14).astype(np.uint8)


def references(f, n, count):
    """rule 2"""
    return [g for g in (f - count // 2 + i for i in range(count)) if 0 <= g < n and g != f]


def hypothesis(d0, k, step):
    """rule 4"""
    return d0 * (1.0 + float(k) * step)


def costs(cams, G, f, uu, vv, d0, p, mg):
    """rules 4 and 5 for the pixels (uu, vv) of frame f with input disparities d0 -> (sums [2K + 1, m] int64, cnts [2K + 1, m] int64,
    how often a hypothesis was not live (``dead``), a live one had Xc.z <= 0 (``behind``) or landed outside the interior (``outside``))"""
    n, h, w = G.shape
    N, K = p["ssd_win"], p["steps"]
    step = p["rel_range"] / float(K)
    sums, cnts = np.zeros((2 * K + 1, len(uu)), np.int64), np.zeros((2 * K + 1, len(uu)), np.int64)
    Gi = G.astype(np.int64)
    seen = dict(dead=0, behind=0, outside=0)
    with np.errstate(all="ignore"):
        for k in range(-K, K + 1):
            dk = hypothesis(d0, k, step)
            live = (dk >= p["dsp_min"]) & (dk <= p["dsp_max"])
            seen["dead"] += int((~live).sum())
            if k != 0:
                mg.see("bound", np.minimum(np.abs(dk - p["dsp_min"]), np.abs(dk - p["dsp_max"])))
            P = world_from_img(cams[f], uu, vv, 1.0 / dk)
            for g in references(f, n, p["ref_frm_count"]):
                c = cams[g]
                xc = cam_from_world(c, P)
                zpos = live & (xc[2] > 0.0)
                mg.see("z", np.abs(xc[2][live]))
                fu, fv = c.fx * xc[0] / xc[2] + c.cx + 0.5, c.fy * xc[1] / xc[2] + c.cy + 0.5
                for q in (fu[zpos], fv[zpos]):
                    mg.see("coord", np.abs(q - np.round(q)))
                u2, v2 = cvt_i32(fu), cvt_i32(fv)
                ok = zpos & (u2 >= N) & (u2 < w - N) & (v2 >= N) & (v2 < h - N)
                seen["behind"] += int((live & ~zpos).sum())
                seen["outside"] += int((zpos & ~ok).sum())
                s = np.zeros(int(ok.sum()), np.int64)
                for a in range(-N, N + 1):
                    for b in range(-N, N + 1):
                        df = Gi[f, vv[ok] + a, uu[ok] + b] - Gi[g, v2[ok] + a, u2[ok] + b]
                        s += df * df
                sums[k + K, ok] += s
                cnts[k + K, ok] += 1
    return sums, cnts, seen


def choose(sums, cnts, K):
    """rule 6 -> (k* [m], eligible-any [m])"""
    m = sums.shape[1]
    best = np.full(m, NONE, np.int64)
    bs, bc = np.zeros(m, np.int64), np.zeros(m, np.int64)
    order = [0] + [s * j for j in range(1, K + 1) for s in (-1, 1)]
    for k in order:
        s, c = sums[k + K], cnts[k + K]
        better = (c > 0) & ((best == NONE) | (s * bc < bs * c))
        best, bs, bc = np.where(better, k, best), np.where(better, s, bs), np.where(better, c, bc)
    return best, best != NONE


def refine_frame(cams, G, depths, f, p, mg):
    """rules 3-8 for frame f -> dict(out float32 [h, w], k int8, sum int32, cnt uint8, cand bool, sums, cnts, at = (vv, uu))"""
    n, h, w = G.shape
    N, K = p["ssd_win"], p["steps"]
    raster = np.asarray(depths[f], np.float32)
    d = raster.astype(np.float64)
    vv, uu = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore"):
        cand = (d >= p["dsp_min"]) & (d <= p["dsp_max"]) & (uu >= N) & (uu < w - N) & (vv >= N) & (vv < h - N)       # rule 3
    out = raster.copy()
    kk, ss, cc = np.full((h, w), NONE, np.int8), np.full((h, w), -1, np.int32), np.zeros((h, w), np.uint8)
    vv, uu = vv[cand], uu[cand]
    d0 = d[cand]
    sums, cnts, seen = costs(cams, G, f, uu, vv, d0, p, mg)
    best, any_k = choose(sums, cnts, K)
    step = p["rel_range"] / float(K)
    idx = np.arange(len(d0))
    bi = np.where(any_k, best, 0) + K
    bs, bc = sums[bi, idx], cnts[bi, idx]
    with np.errstate(all="ignore"):
        m = bs.astype(np.float64) / bc.astype(np.float64)
        rms = np.sqrt(m / float((2 * N + 1) * (2 * N + 1)))
        if p["ssd_err"] > 0:
            mg.see("accept", (np.abs(rms - p["ssd_err"]) / p["ssd_err"])[any_k])
        acc = any_k & (rms <= p["ssd_err"])                                                                         # rule 7
        dnew = d0 * (1.0 + best.astype(np.float64) * step)                                                         # d_k*; unused without a k*
        if p["flags"] & SUBSTEP:                                                                                    # rule 8
            lo, hi = np.clip(bi - 1, 0, 2 * K), np.clip(bi + 1, 0, 2 * K)
            both = any_k & (bi - 1 >= 0) & (bi + 1 <= 2 * K) & (cnts[lo, idx] > 0) & (cnts[hi, idx] > 0)
            cm = sums[lo, idx].astype(np.float64) / cnts[lo, idx].astype(np.float64)
            cp = sums[hi, idx].astype(np.float64) / cnts[hi, idx].astype(np.float64)
            den = (cm - 2.0 * m) + cp
            o = 0.5 * ((cm - cp) / den)
            ds = d0 * (1.0 + (best.astype(np.float64) + o) * step)
            use = both & (den > 0.0) & (ds >= p["dsp_min"]) & (ds <= p["dsp_max"])
            dnew = np.where(use, ds, dnew)
            offset = np.where(use, o, 0.0)
        else:
            offset = np.zeros(len(d0))
    res_out = out[cand]
    res_out[acc] = dnew[acc].astype(np.float32)
    out[cand] = res_out
    kk[cand] = np.where(acc, best, NONE).astype(np.int8)
    ss[cand] = np.where(any_k, bs, -1).astype(np.int32)
    cc[cand] = np.where(any_k, bc, 0).astype(np.uint8)
    return dict(out=out, k=kk, sum=ss, cnt=cc, cand=cand, sums=sums, cnts=cnts, at=(vv, uu), best=best, offset=offset, accepted=acc, seen=seen)


def refine_sequence(cams, imgs, depths, p):
    """one sequence: cams[n], imgs [n, h, w, 3] uint8, depths [n, h, w] float32 -> dict(out, k, sum, cnt [n, h, w], frames, margins)"""
    n = len(cams)
    mg = Margins()
    depths = np.asarray(depths, np.float32)
    if n == 0:
        return dict(out=depths.copy(), k=np.zeros(depths.shape, np.int8), sum=np.zeros(depths.shape, np.int32), cnt=np.zeros(depths.shape, np.uint8),
                    frames=[], margins=mg)
    G = grey(imgs)
    frames = [refine_frame(cams, G, depths, f, p, mg) for f in range(n)]                                           # rule 9: the original inputs
    res = {key: np.stack([fr[key] for fr in frames]) for key in ("out", "k", "sum", "cnt")}
    res.update(frames=frames, margins=mg)
    return res


def refine(cameras, imgs, depths, p):
    """``cameras[k]`` / ``imgs[k]`` / ``depths[k]`` per sequence -> a list of refine_sequence results: a sequence does not see another"""
    return [refine_sequence(c, i, d, p) for c, i, d in zip(cameras, imgs, depths)]
