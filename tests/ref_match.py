"""numpy restatement of the SiftMatchGPU rules of include/mvs.h (mvs_sift_match_lists, rules 1-7): the expected values of
tests/test_gpu_match_feature.py.  Scores by an int64 matmul; `loops_*` are the same rules as plain Python loops, for the check of the
restatement itself on a small case (tests/test_match_feature_host.py)."""
import math

import numpy as np

INT_MIN = -2 ** 31


def quantise(descs):
    """rule 1: q = (int)(512 d + 0.5) in float32, truncating; d <= 0 or NaN -> 0; above 255 -> 255"""
    d = np.asarray(descs, np.float32).reshape(-1, 128)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.float32(512.0) * d + np.float32(0.5)
        q = np.where(d > 0, np.minimum(np.trunc(t), np.float32(255.0)), np.float32(0.0))
    return q.astype(np.int64)


def scores(q1, q2):
    """rule 3"""
    return q1 @ q2.T


def direction(s):
    """rule 4 without the thresholds, for the rows of s [na, nb]: best, bestidx (lowest j), second (0 without another j); with
    nb == 0: best = 0, bestidx = -1, second = 0"""
    na, nb = s.shape
    if nb == 0:
        return np.zeros(na, np.int64), np.full(na, -1, np.int64), np.zeros(na, np.int64)
    idx = np.argmax(s, axis=1)                                          # the first maximum
    best = s[np.arange(na), idx]
    if nb == 1:
        return best, idx, np.zeros(na, np.int64)
    t = s.copy()
    t[np.arange(na), idx] = -1
    return best, idx, t.max(axis=1)


def distances(best, second):
    with np.errstate(invalid="ignore"):
        return np.arccos(np.minimum(best / 262144.0, 1.0)), np.arccos(np.minimum(second / 262144.0, 1.0))


def decide(best, idx, second, distmax, ratiomax):
    """rule 4's thresholds -> m(i)"""
    dist, dist2 = distances(best, second)
    ok = (best > 0) & (dist < distmax) & (dist < ratiomax * dist2)
    return np.where(ok, idx, -1)


def match_pair(descs1, descs2, distmax=0.7, ratiomax=0.8, max_sift=4096, signed_bytes=False):
    """rules 1-5 for one list pair -> [m, 2] int32 (i, j).  signed_bytes: the WRONG rule a kernel that forgot the bias would follow
    (bytes above 127 read as negative), for the scenario checks."""
    q1, q2 = quantise(descs1)[:max_sift], quantise(descs2)[:max_sift]
    if signed_bytes:
        q1, q2 = np.where(q1 > 127, q1 - 256, q1), np.where(q2 > 127, q2 - 256, q2)
    s = scores(q1, q2)
    m12 = decide(*direction(s), distmax, ratiomax)
    m21 = decide(*direction(s.T), distmax, ratiomax)
    out = [(i, j) for i, j in enumerate(m12) if j >= 0 and m21[j] == i]
    return np.array(out, np.int32).reshape(-1, 2)


def margins(descs1, descs2, distmax=0.7, ratiomax=0.8, max_sift=4096):
    """the smallest |dist - distmax| and |dist - ratiomax dist2| over the descriptors with best > 0, both directions"""
    q1, q2 = quantise(descs1)[:max_sift], quantise(descs2)[:max_sift]
    s = scores(q1, q2)
    a = b = math.inf
    for t in (s, s.T):
        best, _, second = direction(t)
        dist, dist2 = distances(best, second)
        ok = best > 0
        if ok.any():
            a = min(a, float(np.abs(dist[ok] - distmax).min()))
            b = min(b, float(np.abs(dist[ok] - ratiomax * dist2[ok]).min()))
    return a, b


def cvt_i32(x):
    """the double -> int rule of the library (csrc/camera_dev.h)"""
    x = float(x)
    return int(x) if -2147483649.0 < x < 2147483648.0 else INT_MIN


def raw_row(l1, key1, l2, key2, view_count):
    """rule 6: keys are float32 {x, y, s, o}; the sum is in double"""
    return (l1 % view_count, cvt_i32(float(np.float32(key1[0])) + 0.5), cvt_i32(float(np.float32(key1[1])) + 0.5),
            l2 % view_count, cvt_i32(float(np.float32(key2[0])) + 0.5), cvt_i32(float(np.float32(key2[1])) + 0.5))


def match_feature(keys1, descs1, keys2, descs2, view_count, distmax=0.7, ratiomax=0.8, max_sift=4096):
    """rules 1-7 for two sequences given as per-list arrays -> (raw[f1][f2] = [n, 6] int32, pair_counts [L1, L2])"""
    L1, L2 = len(keys1), len(keys2)
    n1, n2 = L1 // view_count, L2 // view_count
    rows = [[[] for _ in range(n2)] for _ in range(n1)]
    counts = np.zeros((L1, L2), np.int64)
    for l1 in range(L1):                                                # the reference's loop order (Processor.cpp:652-664)
        for l2 in range(L2):
            m = match_pair(descs1[l1], descs2[l2], distmax, ratiomax, max_sift)
            counts[l1, l2] = len(m)
            rows[l1 // view_count][l2 // view_count] += [raw_row(l1, keys1[l1][i], l2, keys2[l2][j], view_count) for i, j in m]
    return [[np.array(r, np.int32).reshape(-1, 6) for r in row] for row in rows], counts


# ------------------------------------------------------------------ plain loops ----
def loops_quantise(descs):
    out = []
    for row in np.asarray(descs, np.float32).reshape(-1, 128):
        q = []
        for d in row:
            if not (d > 0):
                q.append(0)
                continue
            t = np.float32(np.float32(512.0) * d) + np.float32(0.5)
            q.append(255 if t >= 256 else int(t))
        out.append(q)
    return out


def loops_direction(qa, qb):
    """best, bestidx, second per descriptor of qa against qb, by the letter of rule 4"""
    out = []
    for a in qa:
        s = [sum(x * y for x, y in zip(a, b)) for b in qb]
        if not s:
            out.append((0, -1, 0))
            continue
        best = max(s)
        idx = s.index(best)
        rest = [v for j, v in enumerate(s) if j != idx]
        out.append((best, idx, max(rest) if rest else 0))
    return out


def loops_match_pair(descs1, descs2, distmax, ratiomax, max_sift):
    q1, q2 = loops_quantise(descs1)[:max_sift], loops_quantise(descs2)[:max_sift]

    def m(qa, qb):
        r = []
        for best, idx, second in loops_direction(qa, qb):
            if best == 0:
                r.append(-1)
                continue
            dist, dist2 = math.acos(min(best / 262144.0, 1.0)), math.acos(min(second / 262144.0, 1.0))
            r.append(idx if dist < distmax and dist < ratiomax * dist2 else -1)
        return r
    m12, m21 = m(q1, q2), m(q2, q1)
    return [(i, j) for i, j in enumerate(m12) if j >= 0 and m21[j] == i]
