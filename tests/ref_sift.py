"""numpy restatement of mvs_sift_detect (include/mvs.h, rules 1-9; csrc/sift.hip, csrc/sift_rules.h), operation for operation.
``dtype=np.float32`` is the pin: rules 1-6 are then the library's float32 operations in the library's order, so Gaussian levels and
the stage-6 candidates are bit-equal to the device's; rules 7-8 go through numpy's float32 exp / atan2 / sqrt / sin / cos, which the
device's libm only approximates.  ``dtype=np.float64`` evaluates the same formulas in double (taps and parameters stay the float32
values the library is given): the difference between the two runs is the rounding noise the GPU tolerances are derived from.

Every key also carries its decision margins (``detect(...)["margins"]``): how far each accept / reject decision was from flipping."""
import math

import numpy as np

Q = 16777216.0
SMOOTH = 6


def default_params(**kw):
    p = dict(first_octave=-1, dog_levels=3, max_orient=2, max_features=2 ** 31 - 1, dog_threshold=0.02, edge_threshold=10.0, sigma0=1.6,
             sigma_in=0.5, hl=0.0, hr=0.0, vl=0.0, vr=0.0)
    p.update(kw)
    return p


def grey8(img):
    a = img.astype(np.int64)
    return (4899 * a[..., 0] + 9617 * a[..., 1] + 1868 * a[..., 2] + 8192) >> 14


def octaves(W0, H0):
    return max(1, int(math.floor(math.log2(min(W0, H0)))) - 3)


def taps(sigma):
    """rule 3: (r, float32 taps); libm's exp in double, as the library's host code"""
    r = int(math.ceil(4.0 * sigma))
    t = [math.exp(-(float(i) * float(i)) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)]
    s = 0.0
    for v in t:
        s += v
    return r, np.array([v / s for v in t], np.float64).astype(np.float32)


def level_sigma(l, p):
    s0, sin_ = float(np.float32(p["sigma0"])), float(np.float32(p["sigma_in"]))
    S = p["dog_levels"]
    if l == 0:
        sb = sin_ * (2.0 if p["first_octave"] < 0 else 1.0)
        return math.sqrt(s0 * s0 - sb * sb)
    a, b = s0 * math.pow(2.0, l / S), s0 * math.pow(2.0, (l - 1) / S)
    return math.sqrt(a * a - b * b)


def margins_px(w, h, p):
    """(left, right, top, bottom): pixels outside [left, right) x [top, bottom) are black; the key filter uses the same numbers"""
    return int(w * p["hl"]), w - int(w * p["hr"]), int(h * p["vl"]), h - int(h * p["vr"])


def grey(img, p, dt):
    h, w = img.shape[:2]
    I = grey8(img).astype(dt) / dt(255.0)
    l, r, t, b = margins_px(w, h, p)
    I[:t] = 0; I[b:] = 0; I[:, :l] = 0; I[:, r:] = 0
    return I


def base(I, p, dt):
    if p["first_octave"] == 0:
        return I
    h, w = I.shape
    R = np.empty((h, 2 * w), dt)
    R[:, 0::2] = I
    R[:, 1::2] = dt(0.5) * (I + I[:, np.minimum(np.arange(w) + 1, w - 1)])
    U = np.empty((2 * h, 2 * w), dt)
    U[0::2] = R
    U[1::2] = dt(0.5) * (R + R[np.minimum(np.arange(h) + 1, h - 1)])
    return U


def blur(a, sigma, dt):
    r, k = taps(sigma)
    k = k.astype(dt)
    H, W = a.shape
    P = np.pad(a, ((0, 0), (r, r)), mode="edge")
    acc = k[0] * P[:, 0:W]
    for i in range(1, 2 * r + 1):
        acc = acc + k[i] * P[:, i:i + W]
    P = np.pad(acc, ((r, r), (0, 0)), mode="edge")
    acc = k[0] * P[0:H]
    for i in range(1, 2 * r + 1):
        acc = acc + k[i] * P[i:i + H]
    return acc


def pyramid(img, p, dt=np.float32):
    """-> list over octaves of [S + 3, H, W]"""
    S = p["dog_levels"]
    U = base(grey(img, p, dt), p, dt)
    out = []
    for o in range(octaves(U.shape[1], U.shape[0])):
        g = [blur(U, level_sigma(0, p), dt) if o == 0 else out[-1][S][0::2, 0::2][:out[-1].shape[1] // 2, :out[-1].shape[2] // 2]]
        for l in range(1, S + 3):
            g.append(blur(g[-1], level_sigma(l, p), dt))
        out.append(np.stack(g))
    return out


def step_of(o, p):
    return 0.5 * 2 ** o if p["first_octave"] < 0 else float(2 ** o)


def refine(D, T, e, dt):
    """sift_refine on D [n, 3, 3, 3] -> (keep, dx, dy, ds, vr, slack dict); the order of operations is csrc/sift_rules.h's"""
    c = lambda x: dt(x)
    v = D[:, 1, 1, 1]
    gx = c(0.5) * (D[:, 1, 1, 2] - D[:, 1, 1, 0]); gy = c(0.5) * (D[:, 1, 2, 1] - D[:, 1, 0, 1]); gs = c(0.5) * (D[:, 2, 1, 1] - D[:, 0, 1, 1])
    dxx = (D[:, 1, 1, 2] + D[:, 1, 1, 0]) - c(2.0) * v
    dyy = (D[:, 1, 2, 1] + D[:, 1, 0, 1]) - c(2.0) * v
    dss = (D[:, 2, 1, 1] + D[:, 0, 1, 1]) - c(2.0) * v
    dxy = c(0.25) * ((D[:, 1, 2, 2] - D[:, 1, 2, 0]) - (D[:, 1, 0, 2] - D[:, 1, 0, 0]))
    dxs = c(0.25) * ((D[:, 2, 1, 2] - D[:, 2, 1, 0]) - (D[:, 0, 1, 2] - D[:, 0, 1, 0]))
    dys = c(0.25) * ((D[:, 2, 2, 1] - D[:, 2, 0, 1]) - (D[:, 0, 2, 1] - D[:, 0, 0, 1]))
    tr = dxx + dyy
    det2 = dxx * dyy - dxy * dxy
    lhs, rhs = (tr * tr) * e, ((e + c(1.0)) * (e + c(1.0))) * det2
    with np.errstate(all="ignore"):
        keep = (det2 > 0) & (lhs < rhs)
        b0, b1, b2 = -gx, -gy, -gs
        det = (dxx * (dyy * dss - dys * dys) - dxy * (dxy * dss - dys * dxs)) + dxs * (dxy * dys - dyy * dxs)
        keep &= det != 0
        dx = ((b0 * (dyy * dss - dys * dys) - dxy * (b1 * dss - dys * b2)) + dxs * (b1 * dys - dyy * b2)) / det
        dy = ((dxx * (b1 * dss - dys * b2) - b0 * (dxy * dss - dys * dxs)) + dxs * (dxy * b2 - b1 * dxs)) / det
        ds = ((dxx * (dyy * b2 - b1 * dys) - dxy * (dxy * b2 - b1 * dxs)) + b0 * (dxy * dys - dyy * dxs)) / det
        keep &= (np.abs(dx) < 1) & (np.abs(dy) < 1) & (np.abs(ds) < 1)
        vr = v + c(0.5) * ((gx * dx + gy * dy) + gs * ds)
        keep &= np.abs(vr) > T
        slack = dict(contrast=np.minimum(np.abs(v), np.abs(vr)).astype(np.float64) - float(T),
                     edge=np.minimum(det2, (rhs - lhs) / ((e + c(1.0)) * (e + c(1.0)))).astype(np.float64),
                     delta=1.0 - np.maximum(np.maximum(np.abs(dx), np.abs(dy)), np.abs(ds)).astype(np.float64))
    return keep, dx, dy, ds, vr, slack


def candidates(pyr, w, h, p, dt=np.float32):
    """rules 5-6 -> dict of arrays in the order of rule 9: o, l, xi, yi (int), x, y, s, so, dx, dy (dt), margins"""
    S = p["dog_levels"]
    T = dt(np.float32(p["dog_threshold"]) / np.float32(S))
    e = dt(np.float32(p["edge_threshold"]))
    left, right, top, bottom = margins_px(w, h, p)
    rows = {k: [] for k in ("o", "l", "xi", "yi", "x", "y", "s", "so", "dx", "dy", "m_contrast", "m_edge", "m_delta", "m_gap", "m_xy")}
    for o, g in enumerate(pyr):
        d = g[1:] - g[:-1]
        H, W = d.shape[1:]
        step = dt(step_of(o, p))
        for l in range(1, S + 1):
            v = d[l, 1:-1, 1:-1]
            nb = [d[l + a, 1 + b:H - 1 + b, 1 + c:W - 1 + c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
            nmax, nmin = np.maximum.reduce(nb), np.minimum.reduce(nb)
            yi, xi = np.nonzero((np.abs(v) > T) & ((v > nmax) | (v < nmin)))
            if len(yi) == 0:
                continue
            gap = np.where(v[yi, xi] > nmax[yi, xi], v[yi, xi] - nmax[yi, xi], nmin[yi, xi] - v[yi, xi]).astype(np.float64)
            yi, xi = yi + 1, xi + 1
            D = np.stack([d[l - 1 + a, yi + b, xi + c] for a in range(3) for b in (-1, 0, 1) for c in (-1, 0, 1)], axis=1).reshape(-1, 3, 3, 3)
            keep, dx, dy, ds, vr, slack = refine(D, T, e, dt)
            x = ((xi.astype(dt) + dx) + dt(0.5)) * step
            y = ((yi.astype(dt) + dy) + dt(0.5)) * step
            with np.errstate(all="ignore"):
                keep &= ~((x < left) | (x > right) | (y < top) | (y > bottom))
                so = dt(np.float32(p["sigma0"])) * np.exp2((dt(l) + ds) / dt(S))
                mxy = np.minimum(np.minimum(x - left, right - x), np.minimum(y - top, bottom - y)).astype(np.float64)
            for k, a in (("o", np.full(len(xi), o)), ("l", np.full(len(xi), l)), ("xi", xi), ("yi", yi), ("x", x), ("y", y), ("s", so * step), ("so", so),
                         ("dx", dx), ("dy", dy), ("m_contrast", slack["contrast"]), ("m_edge", slack["edge"]), ("m_delta", slack["delta"]),
                         ("m_gap", gap), ("m_xy", mxy)):
                rows[k].append(np.asarray(a)[keep])
    ints = ("o", "l", "xi", "yi")
    return {k: (np.concatenate(v) if v else np.zeros(0, np.int64 if k in ints else (np.float64 if k.startswith("m_") else dt))) for k, v in rows.items()}


def _quant(v, dt):
    return np.floor(v * dt(Q) + dt(0.5)).astype(np.int64)


def orientation(g, xi, yi, dx, dy, so, max_orient, dt=np.float32):
    """rule 7 for one candidate on its level g [H, W] -> (angles, h [36] smoothed, margin relative to the largest bin)"""
    H, W = g.shape
    f32 = dt == np.float32
    two_pi = dt(np.float32(2 * math.pi)) if f32 else dt(2 * math.pi)
    bin36 = dt(np.float32(36.0 / (2 * math.pi))) if f32 else dt(36.0 / (2 * math.pi))
    ostep = dt(np.float32(2 * math.pi / 36.0)) if f32 else dt(2 * math.pi / 36.0)
    sw = dt(1.5) * so
    R = int(dt(3.0) * sw + dt(0.5))
    oy, ox = np.mgrid[-R:R + 1, -R:R + 1]
    oy, ox = oy.reshape(-1), ox.reshape(-1)
    px, py = xi + ox, yi + oy
    ok = (px >= 1) & (px <= W - 2) & (py >= 1) & (py <= H - 2)
    px, py, ox, oy = px[ok], py[ok], ox[ok], oy[ok]
    gx = g[py, px + 1] - g[py, px - 1]
    gy = g[py + 1, px] - g[py - 1, px]
    fx, fy = ox.astype(dt) - dx, oy.astype(dt) - dy
    v = np.exp(-(fx * fx + fy * fy) / (dt(2.0) * sw * sw)) * np.sqrt(gx * gx + gy * gy)
    ang = np.arctan2(gy, gx)
    ang = np.where(ang < 0, ang + two_pi, ang)
    fb = ang * bin36 - dt(0.5)
    b0 = np.floor(fb)
    rb = fb - b0
    b0 = b0.astype(np.int64)
    hist = np.zeros(36, np.int64)
    np.add.at(hist, (b0 + 36) % 36, _quant((dt(1.0) - rb) * v, dt))
    np.add.at(hist, (b0 + 37) % 36, _quant(rb * v, dt))
    hcur = hist.astype(dt) / dt(Q)
    for _ in range(SMOOTH):
        hcur = ((np.roll(hcur, 1) + hcur) + np.roll(hcur, -1)) / dt(3.0)
    hm, hp = np.roll(hcur, 1), np.roll(hcur, -1)
    mx = hcur.max()
    if not mx > 0:
        return np.zeros(0, dt), hcur, 0.0
    peak = (hcur > hm) & (hcur > hp) & (hcur >= dt(0.8) * mx)
    order = sorted(np.nonzero(peak)[0], key=lambda b: (-hcur[b], b))
    out = []
    for b in order[:max_orient]:
        dd = dt(0.5) * (hm[b] - hp[b]) / ((hm[b] - dt(2.0) * hcur[b]) + hp[b])
        th = ((dt(b) + dd) + dt(0.5)) * ostep
        if th < 0:
            th = th + two_pi
        if th >= two_pi:
            th = th - two_pi
        out.append(th)
    # how far any of these decisions is from flipping, in units of the largest bin
    h64, m64 = hcur.astype(np.float64), float(mx)
    near = h64 >= 0.7 * m64
    locmax = (h64 >= np.roll(h64, 1)) & (h64 >= np.roll(h64, -1))
    cands = [np.abs(h64[near & locmax] - 0.8 * m64).min(initial=np.inf),
             np.minimum(np.abs(h64 - np.roll(h64, 1)), np.abs(h64 - np.roll(h64, -1)))[near].min(initial=np.inf)]
    pv = np.sort(h64[peak])[::-1]
    if len(pv) > 1:
        cands.append(np.abs(np.diff(pv)).min())
    return np.array(out, dt), hcur, float(min(cands)) / m64


def descriptor(g, xi, yi, dx, dy, so, th, dt=np.float32):
    """rule 8 for one key -> [128]"""
    H, W = g.shape
    f32 = dt == np.float32
    two_pi = dt(np.float32(2 * math.pi)) if f32 else dt(2 * math.pi)
    bin8 = dt(np.float32(8.0 / (2 * math.pi))) if f32 else dt(8.0 / (2 * math.pi))
    m = dt(3.0) * so
    ct, st = np.cos(th), np.sin(th)
    R = int(m * dt(np.float32(3.5355339))) + 2
    oy, ox = np.mgrid[-R:R + 1, -R:R + 1]
    oy, ox = oy.reshape(-1), ox.reshape(-1)
    px, py = xi + ox, yi + oy
    ok = (px >= 1) & (px <= W - 2) & (py >= 1) & (py <= H - 2)
    px, py, ox, oy = px[ok], py[ok], ox[ok], oy[ok]
    ddx, ddy = ox.astype(dt) - dx, oy.astype(dt) - dy
    nx, ny = (ct * ddx + st * ddy) / m, (ct * ddy - st * ddx) / m
    fx, fy = nx + dt(1.5), ny + dt(1.5)
    ok = (fx > -1) & (fx < 4) & (fy > -1) & (fy < 4)
    px, py, nx, ny, fx, fy = px[ok], py[ok], nx[ok], ny[ok], fx[ok], fy[ok]
    gx = dt(0.5) * (g[py, px + 1] - g[py, px - 1])
    gy = dt(0.5) * (g[py + 1, px] - g[py - 1, px])
    v = np.sqrt(gx * gx + gy * gy) * np.exp(-(nx * nx + ny * ny) / dt(8.0))
    dth = np.arctan2(gy, gx) - th
    dth = np.where(dth < 0, dth + two_pi, dth)
    dth = np.where(dth < 0, dth + two_pi, dth)
    dth = np.where(dth >= two_pi, dth - two_pi, dth)
    ft = dth * bin8
    ix, iy, it = np.floor(fx), np.floor(fy), np.floor(ft)
    rx, ry, rt = fx - ix, fy - iy, ft - it
    ix, iy, it = ix.astype(np.int64), iy.astype(np.int64), it.astype(np.int64)
    acc = np.zeros(128, np.int64)
    for a in (0, 1):
        for b in (0, 1):
            cx, cy = ix + a, iy + b
            inside = (cx >= 0) & (cx <= 3) & (cy >= 0) & (cy <= 3)
            wxy = (v * (rx if a else dt(1.0) - rx)) * (ry if b else dt(1.0) - ry)
            cell = (cy * 4 + cx) * 8
            np.add.at(acc, (cell + (it & 7))[inside], _quant(wxy * (dt(1.0) - rt), dt)[inside])
            np.add.at(acc, (cell + ((it + 1) & 7))[inside], _quant(wxy * rt, dt)[inside])
    d = acc.astype(dt) / dt(Q)
    for k in range(2):
        s = 0.0
        for u in d.astype(np.float64):
            s += u * u
        nrm = dt(math.sqrt(s))
        if nrm > 0:
            d = d / nrm
        if k == 0:
            d = np.minimum(d, dt(0.2))
    return d


def detect(img, p=None, dt=np.float32, pyr=None):
    """mvs_sift_detect for one image [h, w, 3] uint8 -> dict(keys [n, 4], descs [n, 128], cand = candidates(), n_or [n_cand], first
    [n_cand] = row of each candidate's first key (before max_features), margins = per-candidate dict, h = smoothed histograms)"""
    p = default_params() if p is None else p
    h, w = img.shape[:2]
    pyr = pyramid(img, p, dt) if pyr is None else pyr
    c = candidates(pyr, w, h, p, dt)
    keys, descs, n_or, first, m_ori, hs = [], [], [], [], [], []
    for i in range(len(c["o"])):
        g = pyr[c["o"][i]][c["l"][i]]
        th, hcur, mo = orientation(g, int(c["xi"][i]), int(c["yi"][i]), c["dx"][i], c["dy"][i], c["so"][i], p["max_orient"], dt)
        n_or.append(len(th)); first.append(len(keys)); m_ori.append(mo); hs.append(hcur)
        for t in th:
            keys.append([c["x"][i], c["y"][i], c["s"][i], t])
            descs.append(descriptor(g, int(c["xi"][i]), int(c["yi"][i]), c["dx"][i], c["dy"][i], c["so"][i], t, dt))
    n = min(len(keys), p["max_features"])
    margins = {k[2:]: v for k, v in c.items() if k.startswith("m_")}
    margins["ori"] = np.array(m_ori, np.float64)
    return dict(keys=np.array(keys[:n], dt).reshape(-1, 4), descs=np.array(descs[:n], dt).reshape(-1, 128), cand=c, n_or=np.array(n_or, np.int64),
                first=np.array(first, np.int64), margins=margins, h=np.array(hs, dt).reshape(-1, 36))


def noise(img, p=None):
    """float32 against float64 over the candidates present in both -> dict(eps_o, eps_d, eps_s, eps_h (histogram / largest bin), n, n32,
    n64): the rounding noise of the restatement, the source of the GPU test's tolerances"""
    a, b = detect(img, p, np.float32), detect(img, p, np.float64)
    ka = {tuple(int(a["cand"][k][i]) for k in ("o", "l", "xi", "yi")): i for i in range(len(a["n_or"]))}
    kb = {tuple(int(b["cand"][k][i]) for k in ("o", "l", "xi", "yi")): i for i in range(len(b["n_or"]))}
    eo = ed = es = eh = 0.0
    n = 0
    for key, i in ka.items():
        j = kb.get(key)
        if j is None:
            continue
        n += 1
        es = max(es, abs(float(a["cand"]["s"][i]) - float(b["cand"]["s"][j])) / float(b["cand"]["s"][j]))
        eh = max(eh, float(np.abs(a["h"][i].astype(np.float64) - b["h"][j]).max() / b["h"][j].max()))
        if a["n_or"][i] != b["n_or"][j]:
            continue
        for t in range(int(a["n_or"][i])):
            ra, rb = a["first"][i] + t, b["first"][j] + t
            if ra >= len(a["keys"]) or rb >= len(b["keys"]):
                continue
            do = abs(float(a["keys"][ra, 3]) - float(b["keys"][rb, 3]))
            eo = max(eo, min(do, 2 * math.pi - do))
            ed = max(ed, float(np.abs(a["descs"][ra].astype(np.float64) - b["descs"][rb]).max()))
    return dict(eps_o=eo, eps_d=ed, eps_s=es, eps_h=eh, n=n, n32=len(ka), n64=len(kb))
