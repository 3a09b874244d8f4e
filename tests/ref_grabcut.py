"""numpy / scipy restatement of mvs_grid_mincut and mvs_grabcut_masks (include/mvs.h), rule for rule and, for the double arithmetic,
operation for operation in the order of csrc/grabcut_rules.h.  Rule G1 is scipy.sparse.csgraph.maximum_flow on int32 with an explicit
source and sink, then a backward breadth-first search from the sink on capacity - flow."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import breadth_first_order, maximum_flow

K = 5
DX = (-1, -1, 0, 1, 1, 1, 0, -1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)
PAIR = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # p00 p01 p02 p11 p12 p22
AT = ((4, 5, 6), (5, 7, 8), (6, 8, 9))
EPS = float(np.finfo(np.float64).eps)


# ---------------------------------------------------------------- rule G1 ----
def neighbour(gw, gh, d):
    """(valid [gh, gw] bool, neighbour node index [gh, gw]) of direction d"""
    y, x = np.mgrid[0:gh, 0:gw]
    nx, ny = x + DX[d], y + DY[d]
    ok = (nx >= 0) & (nx < gw) & (ny >= 0) & (ny < gh)
    return ok, np.where(ok, ny * gw + nx, 0)


def g1_cut(excess, cap):
    """excess [gh, gw] int32, cap [8, gh, gw] int32 -> source_side [gh, gw] uint8: the nodes that cannot reach the sink in the residual
    graph of a maximum flow"""
    gh, gw = excess.shape
    N = gw * gh
    src, snk = N, N + 1
    e = excess.reshape(-1).astype(np.int64)
    rows, cols, vals = [], [], []
    for d in range(8):
        ok, nb = neighbour(gw, gh, d)
        c = cap[d].astype(np.int64)
        m = ok & (c > 0)
        rows.append(np.nonzero(m.reshape(-1))[0]); cols.append(nb[m]); vals.append(c[m])
    pos, neg = np.nonzero(e > 0)[0], np.nonzero(e < 0)[0]
    rows += [np.full(len(pos), src), neg]; cols += [pos, np.full(len(neg), snk)]; vals += [e[pos], -e[neg]]
    rows, cols, vals = (np.concatenate(a) for a in (rows, cols, vals))
    assert e[pos].sum() < 2 ** 31 and vals.max(initial=0) < 2 ** 31
    g = sp.csr_matrix((vals.astype(np.int32), (rows, cols)), shape=(N + 2, N + 2))
    if g.nnz == 0:
        return (e >= 0).astype(np.uint8).reshape(gh, gw)
    res = (g - maximum_flow(g, src, snk).flow).tocsr()
    res.data[res.data < 0] = 0
    res.eliminate_zeros()
    reach = breadth_first_order(res.T.tocsr(), snk, directed=True, return_predecessors=False)
    side = np.ones(N + 2, np.uint8)
    side[reach] = 0
    return side[:N].reshape(gh, gw)


# ---------------------------------------------------------------- the rules ----
def half_image(img):
    """rule 1: [h, w, 3] uint8 -> [hh, hw, 3] uint8"""
    h, w = img.shape[:2]
    hh, hw = h // 2, w // 2
    a = img[:2 * hh, :2 * hw].astype(np.int32)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def rect(hw, hh, hl, hr, vl, vr):
    """rule 2 -> (x0, y0, x1, y1)"""
    return int(hw * hl), int(hh * vl), hw - int(hw * hr), hh - int(hh * vr)


def inside_mask(hw, hh, r):
    m = np.zeros((hh, hw), bool)
    m[r[1]:r[3], r[0]:r[2]] = True
    return m


def luma_components(half, model):
    """rule 4 for the pixels where ``model`` is set -> component per pixel of the model (others 0)"""
    luma = half.astype(np.int32).sum(axis=2)
    out = np.zeros(luma.shape, np.uint8)
    m = int(model.sum())
    cum = np.cumsum(np.bincount(luma[model], minlength=766))
    t = [int(np.argmax(cum >= (k * m + 4) // 5)) for k in range(1, 5)]
    out[model] = sum((tk < luma[model]).astype(np.uint8) for tk in t)
    return out


def start_labels(half, fg):
    return np.where(fg, luma_components(half, fg), luma_components(half, ~fg)).astype(np.uint8)


def learn_sums(half, fg, labels):
    """rule 5's sums: [2][5][10] int64, model 0 = foreground"""
    c = half.astype(np.int64)
    s = np.zeros((2, K, 10), np.int64)
    for mi, model in enumerate((fg, ~fg)):
        for k in range(K):
            px = c[model & (labels == k)]
            s[mi, k, 0] = len(px)
            s[mi, k, 1:4] = px.sum(axis=0)
            for j, (a, b) in enumerate(PAIR):
                s[mi, k, 4 + j] = (px[:, a] * px[:, b]).sum()
    return s


def fit(s, m):
    """rule 5: a component from its sums (python floats are IEEE doubles; the order is grabcut_rules.h's) -> dict or None"""
    cnt = int(s[0])
    if cnt <= 0:
        return None
    n = float(cnt)
    mean = [float(int(s[1 + a])) / n for a in range(3)]
    c = [[float(int(s[AT[a][b]])) / n - mean[a] * mean[b] for b in range(3)] for a in range(3)]

    def dtm():
        return c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0]) + \
            c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0])
    det = dtm()
    if det <= EPS:
        for a in range(3):
            c[a][a] += 0.01
        det = dtm()
    inv = [0.0] * 9
    inv[0] = (c[1][1] * c[2][2] - c[1][2] * c[2][1]) / det
    inv[3] = -(c[1][0] * c[2][2] - c[1][2] * c[2][0]) / det
    inv[6] = (c[1][0] * c[2][1] - c[1][1] * c[2][0]) / det
    inv[1] = -(c[0][1] * c[2][2] - c[0][2] * c[2][1]) / det
    inv[4] = (c[0][0] * c[2][2] - c[0][2] * c[2][0]) / det
    inv[7] = -(c[0][0] * c[2][1] - c[0][1] * c[2][0]) / det
    inv[2] = (c[0][1] * c[1][2] - c[0][2] * c[1][1]) / det
    inv[5] = -(c[0][0] * c[1][2] - c[0][2] * c[1][0]) / det
    inv[8] = (c[0][0] * c[1][1] - c[0][1] * c[1][0]) / det
    weight = n / float(m)
    return dict(mean=mean, inv=inv, det=det, weight=weight, lw=float(np.log(weight)) - 0.5 * float(np.log(det)))


def fit_models(sums):
    """[2][5][10] -> [2][5] components (None: empty)"""
    return [[fit(sums[mi, k], int(sums[mi, :, 0].sum())) for k in range(K)] for mi in range(2)]


def score(g, half):
    """rule 6: a_k of every pixel [hh, hw] under component g"""
    c = half.astype(np.float64)
    d0, d1, d2 = c[..., 0] - g["mean"][0], c[..., 1] - g["mean"][1], c[..., 2] - g["mean"][2]
    i = g["inv"]
    q = d0 * (d0 * i[0] + d1 * i[3] + d2 * i[6]) + d1 * (d0 * i[1] + d1 * i[4] + d2 * i[7]) + d2 * (d0 * i[2] + d1 * i[5] + d2 * i[8])
    return g["lw"] - 0.5 * q


def model_scores(model, half):
    """[5][hh, hw], -inf for an empty component"""
    return np.stack([score(g, half) if g is not None else np.full(half.shape[:2], -np.inf) for g in model])


def assign(models, half, fg):
    """rule 6 -> labels; also the relative gap between the two best scores of every pixel in its own model"""
    a = np.where(fg[None], model_scores(models[0], half), model_scores(models[1], half))
    lab = np.argmax(a, axis=0).astype(np.uint8)                  # the first maximum: the lowest index on ties
    top = np.sort(a, axis=0)[::-1]
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(top[1]), (top[0] - top[1]) / np.maximum(np.abs(top[0]), 1e-300), np.inf)
    return lab, gap


def big_l(model, half, gamma):
    """rule 9's L per pixel"""
    used = [g for g in model if g is not None]
    if not used:
        return np.full(half.shape[:2], 9.0 * gamma)
    a = np.stack([score(g, half) for g in used])
    mx = a.max(axis=0)
    tot = np.zeros_like(mx)
    for k in range(len(used)):
        tot = tot + np.exp(a[k] - mx)
    return -(mx + np.log(tot))


def tlink_max(gamma):
    return int(np.rint(1024.0 * 9.0 * gamma))


def excess_of(models, half, inside, gamma):
    """rule 9 -> (excess int32, the unrounded value 1024 (Lb - Lf))"""
    kk = tlink_max(gamma)
    v = 1024.0 * (big_l(models[1], half, gamma) - big_l(models[0], half, gamma))
    e = np.where(~(v < kk), kk, np.where(v <= -kk, -kk, np.rint(np.clip(v, -kk, kk)))).astype(np.int64)
    return np.where(inside, e, -kk).astype(np.int32), v


def d2_dir(half, d):
    """squared colour difference to the neighbour in direction d (0 where there is none)"""
    hh, hw = half.shape[:2]
    ok, nb = neighbour(hw, hh, d)
    c = half.reshape(-1, 3).astype(np.int64)
    return np.where(ok, ((c.reshape(hh, hw, 3) - c[nb]) ** 2).sum(axis=2), 0), ok


def beta_sum(half):
    return int(sum(int(d2_dir(half, d)[0].sum()) for d in range(4)))


def beta_of(S, hw, hh):
    return 0.0 if S == 0 else 1.0 / (2.0 * (float(S) / float(4 * hw * hh - 3 * hw - 3 * hh + 2)))


def ncap_of(half, gamma):
    """rule 8 -> (cap [8][hh, hw] int32, the unrounded values)"""
    hh, hw = half.shape[:2]
    beta = beta_of(beta_sum(half), hw, hh)
    raw = np.zeros((8, hh, hw))
    for d in range(8):
        d2, ok = d2_dir(half, d)
        g = gamma / float(np.sqrt(2.0)) if d & 1 else gamma
        raw[d] = np.where(ok, 1024.0 * g * np.exp(-beta * d2.astype(np.float64)), 0.0)
    return np.rint(raw).astype(np.int32), raw


def full_mask(half_mask, w, h):
    """rule 12: [hh, hw] non-zero = foreground -> [h, w] uint8 255 / 0"""
    hh, hw = half_mask.shape

    def foot(n, hn):
        x = np.arange(n)
        x0 = np.where(x & 1, (x - 1) // 2, x // 2 - 1)
        return np.clip(x0, 0, hn - 1), np.clip(x0 + 1, 0, hn - 1)
    xa, xb = foot(w, hw)
    ya, yb = foot(h, hh)
    m = half_mask != 0
    f = m[np.ix_(ya, xa)] | m[np.ix_(ya, xb)] | m[np.ix_(yb, xa)] | m[np.ix_(yb, xb)]
    return np.where(f, 255, 0).astype(np.uint8)


def iteration(half, fg, models, inside, cap, gamma):
    """rules 6, 5, 9, 10 from the mask ``fg`` and the models learnt before -> dict(labels, gap, sums, models, excess, raw, mask)"""
    lab, gap = assign(models, half, fg)
    sums = learn_sums(half, fg, lab)
    new = fit_models(sums)
    e, raw = excess_of(new, half, inside, gamma)
    return dict(labels=lab, gap=gap, sums=sums, models=new, excess=e, raw=raw, mask=(inside & (g1_cut(e, cap) != 0)))


def grabcut(img, hl, hr, vl, vr, gamma=50.0, iters=3):
    """one frame [h, w, 3] uint8 -> dict(half, rect, inside, S, cap, cap_raw, labels0, sums0, its [iters], half_mask, mask)"""
    h, w = img.shape[:2]
    half = half_image(img)
    hh, hw = half.shape[:2]
    r = rect(hw, hh, hl, hr, vl, vr)
    inside = inside_mask(hw, hh, r)
    cap, cap_raw = ncap_of(half, gamma)
    fg = inside.copy()
    lab0 = start_labels(half, fg)
    sums0 = learn_sums(half, fg, lab0)
    models = fit_models(sums0)
    its = []
    for _ in range(iters):
        it = iteration(half, fg, models, inside, cap, gamma)
        fg, models = it["mask"], it["models"]
        its.append(it)
    return dict(half=half, rect=r, inside=inside, S=beta_sum(half), cap=cap, cap_raw=cap_raw, labels0=lab0, sums0=sums0, its=its,
                half_mask=fg.astype(np.uint8), mask=full_mask(fg, w, h))
