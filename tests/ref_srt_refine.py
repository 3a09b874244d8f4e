"""numpy restatement of mvs_srt_refine (include/mvs.h, rules I1-I9): brute-force nearest points in float32 with d2f's operation order,
Python-int sums, the same Cholesky loop.  Every fp64 expression is written operation for operation as csrc/srt_refine_rules.h and
csrc/srt_refine.hip write it (no np.dot, no np.cross), so the 121 sums of a pair are the library's integers and the step differs only
by libm's sin, cos and exp."""
import math

import numpy as np

TERMS, JJ, JR, RR = 121, 1, 106, 120
Q = 68719476736.0                       # 2^36
FLT_MAX = 3.4028234663852886e38
FIX_SCALE = 1


def params(**kw):
    p = dict(rel_dist=0.02, min_cos=0.7, damping=1e-9, tol=1e-9, iters=20, stride=1, fixed_seq=-1, min_pairs=64, flags=0)
    for k in kw:
        if k not in p:
            raise KeyError(k)
    p.update(kw)
    return p


def _mv(M, P):
    """mulMv of dev_common.h for the rows of P; M is 3x3"""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([(M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z for i in range(3)], axis=1)


def _dot(A, B):
    return (A[:, 0] * B[:, 0] + A[:, 1] * B[:, 1]) + A[:, 2] * B[:, 2]


def _cross(A, B):
    return np.stack([A[:, 1] * B[:, 2] - A[:, 2] * B[:, 1], A[:, 2] * B[:, 0] - A[:, 0] * B[:, 2], A[:, 0] * B[:, 1] - A[:, 1] * B[:, 0]], axis=1)


def seq_apply(s, R, t, P):
    """I1: y = M p + t with M = s * R element by element"""
    return _mv(s * np.asarray(R, np.float64).reshape(3, 3), P) + np.asarray(t, np.float64).reshape(1, 3)


def relative(sb, Rb, tb, sa, Ra, ta):
    """mvs_srt_relative(b, a): the map of a's points into b's own frame"""
    Rb, Ra = np.asarray(Rb, np.float64).reshape(3, 3), np.asarray(Ra, np.float64).reshape(3, 3)
    tb, ta = np.asarray(tb, np.float64).reshape(3), np.asarray(ta, np.float64).reshape(3)
    Rt = Rb.T
    s = 1.0 / sb * sa
    R = np.array([[(Rt[i, 0] * Ra[0, j] + Rt[i, 1] * Ra[1, j]) + Rt[i, 2] * Ra[2, j] for j in range(3)] for i in range(3)])
    M = (1.0 / sb) * Rt
    t = _mv(M, (ta - tb).reshape(1, 3))[0]
    return s, R, t


def usable(P):
    with np.errstate(invalid="ignore"):
        return (np.isfinite(P) & (np.abs(P) <= FLT_MAX)).all(axis=1)


def unit(N):
    with np.errstate(all="ignore"):
        l2 = _dot(N, N)
        ok = (l2 > 0.0) & np.isfinite(l2)
        return N / np.sqrt(l2)[:, None], ok


def frame(points, scales, Rs, ts):
    """I2 -> (c [3], D); None when there is no box"""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for k, P in enumerate(points):
        P = np.asarray(P, np.float64).reshape(-1, 3)
        P = P[usable(P)]
        if len(P):
            with np.errstate(all="ignore"):
                Y = seq_apply(scales[k], Rs[k], ts[k], P)
            lo, hi = np.fmin(lo, np.fmin.reduce(Y, axis=0)), np.fmax(hi, np.fmax.reduce(Y, axis=0))
    if not (lo[0] <= hi[0]):
        return None
    e = hi - lo
    c = (lo + hi) / 2.0
    D = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) / 2.0
    return (c, D) if D > 0.0 and math.isfinite(D) else None


def nearest(Qf, Tf, chunk=512):
    """I3: for the float32 queries Qf [m, 3] the index of the nearest row of Tf [n, 3] by d2f, ties to the lower index; -1 without one
    (a query that is not finite, or no finite target).  -> (index [m], tie [m]: more than one row at the least distance)"""
    idx, tie = np.full(len(Qf), -1, np.int64), np.zeros(len(Qf), bool)
    Qf, Tf = np.asarray(Qf, np.float32), np.asarray(Tf, np.float32)
    if len(Tf) == 0:
        return idx, tie
    for a in range(0, len(Qf), chunk):
        q = Qf[a:a + chunk]
        with np.errstate(all="ignore"):
            dx, dy, dz = (q[:, None, c] - Tf[None, :, c] for c in range(3))
            r = dx * dx
            r = r + dy * dy
            r = r + dz * dz
        assert r.dtype == np.float32
        r = np.where(np.isnan(r), np.float32(np.inf), r)
        j = np.argmin(r, axis=1)                                   # the first of the least: the lower index
        best = r[np.arange(len(q)), j]
        ok = np.isfinite(q).all(axis=1) & (best < np.inf)
        idx[a:a + chunk] = np.where(ok, j, -1)
        tie[a:a + chunk] = ok & ((r == best[:, None]).sum(axis=1) > 1)
    return idx, tie


def pair_matches(points, normals, scales, Rs, ts, a, b, c, D, p):
    """I3-I5 for the ordered pair (a, b) -> dict(query, target: indices of the accepted matches, r [m], J [m, 14], tie [m], searched:
    queries that found a nearest point, at_cap: accepted matches with |x_a - x_b|^2 == cap^2)"""
    Pa, Na = np.asarray(points[a], np.float64).reshape(-1, 3), np.asarray(normals[a], np.float64).reshape(-1, 3)
    Pb, Nb = np.asarray(points[b], np.float64).reshape(-1, 3), np.asarray(normals[b], np.float64).reshape(-1, 3)
    qi = np.arange(0, len(Pa), p["stride"])
    qi = qi[usable(Pa[qi])] if len(qi) else qi
    s, R, t = relative(scales[b], Rs[b], ts[b], scales[a], Rs[a], ts[a])
    with np.errstate(all="ignore"):
        Yb = seq_apply(s, R, t, Pa[qi]).astype(np.float32)
        Tf = np.where(usable(Pb)[:, None], Pb, np.nan).astype(np.float32)
    j, tie = nearest(Yb, Tf)
    found = j >= 0
    qi, j, tie = qi[found], j[found], tie[found]
    searched = len(qi)
    cap = 2.0 * p["rel_dist"]
    with np.errstate(all="ignore"):
        ua, oka = unit(Na[qi])
        ub, okb = unit(Nb[j])
        xa = (seq_apply(scales[a], Rs[a], ts[a], Pa[qi]) - c.reshape(1, 3)) / D
        xb = (seq_apply(scales[b], Rs[b], ts[b], Pb[j]) - c.reshape(1, 3)) / D
        d = xa - xb
        d2 = _dot(d, d)
        n = _mv(np.asarray(Rs[b], np.float64).reshape(3, 3), ub)
        cosv = _dot(_mv(np.asarray(Rs[a], np.float64).reshape(3, 3), ua), n)
        acc = oka & okb & (d2 <= cap * cap) & (cosv >= p["min_cos"])
    qi, j, tie, xa, xb, d, n, d2, cosv = (v[acc] for v in (qi, j, tie, xa, xb, d, n, d2, cosv))
    r = _dot(n, d)
    J = np.concatenate([_cross(xa, n), n, _dot(n, xa)[:, None], -_cross(xb, n), -n, -_dot(n, xb)[:, None]], axis=1)
    return dict(query=qi, target=j, r=r, J=J, tie=tie, searched=searched, at_cap=int((d2 == cap * cap).sum()), cos=cosv)


def _q(v):
    return np.rint(v * Q).astype(np.int64).tolist()                # llrint: to nearest, ties to even


def pair_sums(m, exact=False):
    """I6: the 121 Python ints of one pair's matches; exact: the same sums unquantised, each the correctly rounded sum (math.fsum)"""
    r, J = m["r"], m["J"]
    red = (lambda v: math.fsum(v.tolist())) if exact else (lambda v: sum(_q(v)))
    out = [float(len(r)) if exact else len(r)]
    for i in range(14):
        for j in range(i, 14):
            out.append(red(J[:, i] * J[:, j]))
    for i in range(14):
        out.append(red(J[:, i] * r))
    out.append(red(r * r))
    return out


def all_sums(points, normals, scales, Rs, ts, p, fr=None, exact=False, details=None):
    """-> sums [n][n][121] (Python ints; zeros on the diagonal), c, D.  details: a dict that receives pair_matches of every pair"""
    n = len(points)
    fr = fr if fr is not None else frame(points, scales, Rs, ts)
    c, D = fr
    S = [[[0.0 if exact else 0] * TERMS for _ in range(n)] for _ in range(n)]
    for a in range(n):
        for b in range(n):
            if a == b or len(points[a]) == 0 or len(points[b]) == 0:
                continue
            m = pair_matches(points, normals, scales, Rs, ts, a, b, c, D, p)
            if details is not None:
                details[(a, b)] = m
            S[a][b] = pair_sums(m, exact)
    return S, c, D


def solve(S, free, fix_scale, damping):
    """I7 -> the step [7 n] (0 where nothing moves); raises ArithmeticError on a pivot <= 0"""
    n = len(S)
    N = 7 * n
    H = [[0.0] * N for _ in range(N)]
    g = [0.0] * N
    at = lambda a, b, i: 7 * a + i if i < 7 else 7 * b + i - 7
    for a in range(n):
        for b in range(n):
            if a == b or S[a][b][0] == 0:
                continue
            k = JJ
            for i in range(14):
                for j in range(i, 14):
                    v = float(S[a][b][k]) * (1.0 / Q)
                    k += 1
                    gi, gj = at(a, b, i), at(a, b, j)
                    H[gi][gj] += v
                    if gi != gj:
                        H[gj][gi] += v
            for i in range(14):
                g[at(a, b, i)] += float(S[a][b][JR + i]) * (1.0 / Q)
    idx = [7 * k + i for k in range(n) if free[k] for i in range(6 if fix_scale else 7)]
    m = len(idx)
    A = [[H[idx[i]][idx[j]] for j in range(m)] for i in range(m)]
    max_diag = 0.0
    for i in range(m):
        if A[i][i] > max_diag:
            max_diag = A[i][i]
    for i in range(m):
        A[i][i] += damping * max_diag
    Lm = [[0.0] * m for _ in range(m)]
    for i in range(m):
        for j in range(i + 1):
            s = A[i][j]
            for k in range(j):
                s -= Lm[i][k] * Lm[j][k]
            if i == j:
                if not s > 0.0:
                    raise ArithmeticError(f"pivot {i}")
                Lm[i][i] = math.sqrt(s)
            else:
                Lm[i][j] = s / Lm[j][j]
    y, x = [0.0] * m, [0.0] * m
    for i in range(m):
        s = -g[idx[i]]
        for k in range(i):
            s -= Lm[i][k] * y[k]
        y[i] = s / Lm[i][i]
    for i in range(m - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, m):
            s -= Lm[k][i] * x[k]
        x[i] = s / Lm[i][i]
    step = [0.0] * N
    for i in range(m):
        step[idx[i]] = x[i]
    return step


def apply_step(st, c, D, s, R, t):
    """I8 -> (s', R', t')"""
    wx, wy, wz = st[0], st[1], st[2]
    th2 = (wx * wx + wy * wy) + wz * wz
    th = math.sqrt(th2)
    dR = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if th > 0.0:
        ka, kb = math.sin(th) / th, (1.0 - math.cos(th)) / th2
        K = [[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]]
        for i in range(3):
            for j in range(3):
                k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j]
                dR[i][j] = (dR[i][j] + ka * K[i][j]) + kb * k2
    g = math.exp(st[6])
    R = np.asarray(R, np.float64).reshape(3, 3)
    Rn = np.array([[(dR[i][0] * R[0, j] + dR[i][1] * R[1, j]) + dR[i][2] * R[2, j] for j in range(3)] for i in range(3)])
    gdR = g * np.array(dR)
    c = np.asarray(c, np.float64).reshape(1, 3)
    tn = _mv(gdR, np.asarray(t, np.float64).reshape(1, 3)) + ((c - _mv(gdR, c)) + D * np.array([[st[3], st[4], st[5]]]))
    return g * s, Rn, tn[0]


def refine(points, normals, scales, Rs, ts, p=None):
    """the whole call -> dict(scales, Rs, ts, iters_done, history [iters_done, 2], pair_count [n, n], trace: per iteration whose search
    ran (chain before, sums, chain after or None when no step followed), c, D)"""
    p = p if p is not None else params()
    n = len(points)
    s = [float(v) for v in scales]
    R = [np.array(v, np.float64).reshape(3, 3) for v in Rs]
    t = [np.array(v, np.float64).reshape(3) for v in ts]
    fr = frame(points, s, R, t)
    if fr is None:
        raise ArithmeticError("no box")
    c, D = fr
    fixed = n - 1 if p["fixed_seq"] < 0 else p["fixed_seq"]
    hist, trace, done = [], [], 0
    pc = np.zeros((n, n), np.int64)
    for it in range(p["iters"]):
        before = (list(s), [v.copy() for v in R], [v.copy() for v in t])
        S, _, _ = all_sums(points, normals, s, R, t, p, fr)
        per, total, rr = [0] * n, 0, 0.0
        for a in range(n):
            for b in range(n):
                cnt = S[a][b][0]
                pc[a, b] = cnt
                total += cnt
                per[a] += cnt
                per[b] += cnt
                rr += float(S[a][b][RR]) * (1.0 / Q)
        free = [k != fixed and per[k] >= p["min_pairs"] and per[k] > 0 for k in range(n)]
        if not any(free):
            trace.append((before, S, None))
            break
        step = solve(S, free, bool(p["flags"] & FIX_SCALE), p["damping"])
        hist.append((float(total), D * math.sqrt(rr / float(total))))
        big = 0.0
        for k in range(n):
            if free[k]:
                s[k], R[k], t[k] = apply_step(step[7 * k:7 * k + 7], c, D, s[k], R[k], t[k])
                big = max(big, max(abs(v) for v in step[7 * k:7 * k + 7]))
        done = it + 1
        trace.append((before, S, (list(s), [v.copy() for v in R], [v.copy() for v in t])))
        if big < p["tol"]:
            break
    return dict(scales=np.array(s), Rs=np.array(R), ts=np.array(t), iters_done=done, history=np.array(hist).reshape(-1, 2), pair_count=pc,
                trace=trace, c=c, D=D)
