"""The images and the tolerances the SIFT tests share (tests/test_sift_host.py, tests/test_gpu_sift.py).  Content: seeded Gaussian
blobs, rectangles and one L-shaped corner over low noise.  The EPS_* constants are the float32-against-float64 noise of the numpy
restatement (tests/ref_sift.py noise()), its largest value over SCENARIOS; tests/test_sift_host.py measures them again on every run and
fails when one is exceeded.  They are never taken from the kernel.  The GPU test allows FACTOR times each: the factor covers a device
libm that rounds differently from numpy's."""
import functools

import numpy as np

from tests import ref_sift as R

FACTOR = 4.0
EPS_O = 3.0e-5       # orientation, radians (cyclic)
EPS_D = 2.0e-5       # one descriptor entry
EPS_S = 2.0e-5       # scale, relative
EPS_H = 5.0e-5       # a bin of the smoothed orientation histogram, relative to the largest bin: the noise of every orientation decision
MAX_UNCLEAR = 0.02   # share of a scenario's candidates whose orientation margin may fall below FACTOR * EPS_H

# (name, w, h, first_octave, seed)
SCENARIOS = [("64x48_up", 64, 48, -1, 7), ("64x48", 64, 48, 0, 7), ("67x45_up", 67, 45, -1, 2), ("67x45", 67, 45, 0, 2), ("20x12_up", 20, 12, -1, 2),
             ("20x12", 20, 12, 0, 2)]
# the seeds were chosen on the CPU (restatement only): every orientation margin of every scenario clears 2 * FACTOR * EPS_H, the 64 x 48
# image (its L-shaped corner among others) has candidates with two orientations, and 20 x 12 has a key at all.  20 x 12 without the doubling is the case whose blur radius (13 for sigma 3.09) exceeds the image's
# height: whole tiles of the column pass read nothing but the replicated border


def scene(w, h, seed, black=False):
    """[h, w, 3] uint8"""
    if black:
        return np.zeros((h, w, 3), np.uint8)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.full((h, w), 0.45)
    for _ in range(max(3, w * h // 300)):
        cx, cy = rng.uniform(3, w - 3), rng.uniform(3, h - 3)
        s = rng.uniform(1.2, 4.0)
        a += rng.uniform(0.25, 0.5) * rng.choice([-1, 1]) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    if w >= 40:
        for _ in range(3):
            x0, y0 = int(rng.integers(4, w - 12)), int(rng.integers(4, h - 12))
            a[y0:y0 + int(rng.integers(5, 10)), x0:x0 + int(rng.integers(5, 10))] += rng.uniform(0.2, 0.4)
        x0, y0 = w // 2 - 6, h // 2 - 6                                   # the L-shaped corner
        a[y0:y0 + 12, x0:x0 + 3] += 0.35
        a[y0 + 9:y0 + 12, x0:x0 + 12] += 0.35
    a += rng.normal(0, 0.004, (h, w))
    g = np.clip(a * 255, 0, 255).astype(np.uint8)
    return np.stack([g, np.clip(g.astype(int) + 3, 0, 255).astype(np.uint8), g], -1)


def oriented_scene(w, h, seed, n=8):
    """[h, w, 3] uint8: n elongated Gaussian ridges at random angles over low noise.  A round blob has no direction, so its orientation
    histogram is flat and its peaks are decided by noise; these have one, and the chain scenario needs every such decision clear"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.full((h, w), 0.45)
    for _ in range(n):
        cx, cy = rng.uniform(10, w - 10), rng.uniform(10, h - 10)
        s1 = rng.uniform(1.5, 3.5)
        s2, th = s1 * rng.uniform(1.8, 3.0), rng.uniform(0, np.pi)
        u, v = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th), (yy - cy) * np.cos(th) - (xx - cx) * np.sin(th)
        a += rng.uniform(0.25, 0.5) * rng.choice([-1, 1]) * np.exp(-(u * u / (2 * s1 * s1) + v * v / (2 * s2 * s2)))
    a += rng.normal(0, 0.004, (h, w))
    g = np.clip(a * 255, 0, 255).astype(np.uint8)
    return np.stack([g, np.clip(g.astype(int) + 3, 0, 255).astype(np.uint8), g], -1)


def params_of(fo, **kw):
    return R.default_params(first_octave=fo, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float32 restatement of a scenario, computed once: (img, params, pyramid, detect())"""
    _, w, h, fo, seed = next(s for s in SCENARIOS if s[0] == name)
    img, p = scene(w, h, seed), params_of(fo)
    pyr = R.pyramid(img, p, np.float32)
    return img, p, pyr, R.detect(img, p, np.float32, pyr=pyr)


# ------------------------------------------------------------------ the chain ----
# Images to matches on the 96 x 72 three-frame cull scenario (tests/test_views_host.py: cameras and depths): the views of
# ref_views, the keys of ref_sift, the cull of ref_views, the matches of ref_match.  The same three frames are loaded twice, as sequence
# A with views 10 degrees apart and as sequence B with views 6 degrees apart, so every list pair of one frame is a view change of 0 to
# 16 degrees and list pairs of different frames show different content.
CHAIN_SEEDS = (76, 77, 78)
CHAIN_ROT = (10.0, 6.0)
CHAIN_SIFT = dict(hl=0.05, vr=0.05, max_features=12)
CHAIN_EPS_D = 5.0e-5       # the restatement's noise on the chain's 18 views (test_sift_host measures it again): a descriptor entry
CHAIN_EPS_H = 1.6e-4       # and a bin of the orientation histogram relative to the largest
CHAIN_MIN_MATCHES = 8       # view-change matches a list pair of the property test must have


def _decisions(slo, shi, distmax, ratiomax):
    """for a score matrix known only to lie in [slo, shi], entry by entry: (certain [na, nb]: row i accepts j whatever the scores are,
    possible [na, nb]: row i accepts j for some scores), by the rule of ref_match.decide"""
    na, nb = slo.shape
    if na == 0 or nb == 0:
        return np.zeros((na, nb), bool), np.zeros((na, nb), bool)
    dist = lambda s: np.arccos(np.minimum(s / 262144.0, 1.0))
    r = np.arange(na)
    idx = np.argmax(slo, axis=1)
    t = shi.copy()
    t[r, idx] = 0
    oth_hi = t.max(axis=1)                                              # the largest the second score can be (0 without another j)
    best_lo = slo[r, idx]
    certain = np.zeros((na, nb), bool)
    certain[r, idx] = (best_lo > oth_hi) & (best_lo > 0) & (dist(best_lo) < distmax) & (dist(best_lo) < ratiomax * dist(oth_hi))
    t = slo.copy()
    t[r, idx] = 0
    oth_lo = np.where(np.arange(nb)[None] == idx[:, None], t.max(axis=1)[:, None], best_lo[:, None])    # the smallest the best other score can be
    possible = (shi >= oth_lo) & (shi > 0) & (dist(shi) < distmax) & (dist(shi) < ratiomax * dist(oth_lo))
    return certain, possible


def match_unclear(d1, d2, eps, distmax=0.7, ratiomax=0.8):
    """how many pairs (i, j) ref_match.match_pair(d1, d2) could gain or lose for descriptors within eps of d1 and d2, entry by entry.
    Quantisation is monotonic and the quantised entries are not negative, so every score lies between the product of the lower and
    the product of the upper quantisations.  A pair is certain when each of the two accepts the other under the worst of these scores,
    possible when each can accept the other under some; the result is decided when the two sets are the same."""
    from tests import ref_match as RM
    e = np.float32(eps)
    d1, d2 = np.asarray(d1, np.float32).reshape(-1, 128), np.asarray(d2, np.float32).reshape(-1, 128)
    lo1, hi1, lo2, hi2 = RM.quantise(d1 - e), RM.quantise(d1 + e), RM.quantise(d2 - e), RM.quantise(d2 + e)
    slo, shi = lo1 @ lo2.T, hi1 @ hi2.T
    c12, p12 = _decisions(slo, shi, distmax, ratiomax)
    c21, p21 = _decisions(slo.T, shi.T, distmax, ratiomax)
    return int(((p12 & p21.T) != (c12 & c21.T)).sum())


@functools.lru_cache(maxsize=1)
def chain_reference(seeds=CHAIN_SEEDS, eps_d=None, eps_h=None, **sift):
    """-> dict(cameras, depths, imgs, sift (parameters), seqs = per sequence dict(views, tex, refs = detect() per list, keys, descs after
    the cull), raw = ref_match.match_feature of A against B, unclear = match decisions within FACTOR * EPS_D of flipping)"""
    from multiviewstitch_amd import scene as S
    from tests import ref_match as RM, ref_views as RV
    from tests.test_views_host import CFRAMES, CH, CVIEWS, CW
    cams, depths = S.make_sequence(CFRAMES, CW, CH, 25.0, f=2.2)
    imgs = np.stack([oriented_scene(CW, CH, s) for s in seeds])
    p = params_of(-1, **dict(CHAIN_SIFT, **sift))
    seqs = []
    for rot in CHAIN_ROT:
        views, tex, _ = RV.gen_new_views(cams, imgs, CVIEWS, 0, rot)
        refs = [R.detect(v, p) for v in views.reshape(-1, CH, CW, 3)]
        _, keys, descs = RV.keypoint_cull(cams, CVIEWS, [r["keys"] for r in refs], [r["descs"] for r in refs], tex, depths, S.MIN_DSP, S.MAX_DSP)
        seqs.append(dict(rot=rot, views=views, tex=tex, refs=refs, keys=keys, descs=descs))
    a, b = seqs
    raw, counts = RM.match_feature(a["keys"], a["descs"], b["keys"], b["descs"], CVIEWS)
    unclear = sum(match_unclear(d1, d2, FACTOR * (eps_d or CHAIN_EPS_D)) for d1 in a["descs"] for d2 in b["descs"])
    # an orientation decision matters when its candidate starts before the max_features cut: a change there moves every later key
    ori = [r["margins"]["ori"][r["first"] < p["max_features"]] for q in seqs for r in q["refs"]]
    ori_unclear = int(sum((m <= FACTOR * (eps_h or CHAIN_EPS_H)).sum() for m in ori))
    return dict(cameras=cams, depths=depths, imgs=imgs, sift=p, seqs=seqs, raw=raw, counts=counts, unclear=unclear, ori_unclear=ori_unclear)
