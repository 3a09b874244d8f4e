"""Rules O1-O6 of include/mvs.h (the match and SIFT overlay pictures) restated in numpy and Python integers.  The canvas is painted
primitive after primitive in list order, each one over the pixels it covers: sequential painting, the formulation the reference has, and
not the kernel's gather from the highest index down.  Nothing here is shared with csrc/overlay_rules.h.

A primitive is the record of ``processor.draw_prim``: (x0, y0, x1, y1, kind, size, (c0, c1, c2), (0, 0, 0))."""
import math

import numpy as np

DISC, RING, SEGMENT = 0, 1, 2
RNG_DEFAULT = 0xFFFFFFFF
INT_MIN = -2 ** 31
RING_COLOUR = (255, 255, 0)          # cv::Scalar(255, 255, 0), B G R
MARK_COLOUR = (0, 255, 0)


def prim(kind, x0, y0, x1=0, y1=0, size=1, colour=(0, 0, 0)):
    return (int(x0), int(y0), int(x1), int(y1), int(kind), int(size), tuple(int(c) for c in colour), (0, 0, 0))


def covers(p, x, y):
    """O3 for one pixel, in Python integers"""
    x0, y0, x1, y1, kind, size = p[:6]
    ex, ey = x - x0, y - y0
    d2 = ex * ex + ey * ey
    if kind == DISC:
        return d2 <= size * size
    if kind == RING:
        return d2 == 0 if size == 0 else (size - 1) ** 2 < d2 <= size * size
    dx, dy = x1 - x0, y1 - y0
    L2, s = dx * dx + dy * dy, ex * dx + ey * dy
    if s <= 0:
        return 4 * d2 <= size * size
    if s >= L2:
        return 4 * ((x - x1) ** 2 + (y - y1) ** 2) <= size * size
    return 4 * (ex * dy - ey * dx) ** 2 <= size * size * L2


def mask(p, w, h, exact=False):
    """-> (y slice, x slice, bool array): the pixels of a w x h canvas that p covers, inside the clipped box that can hold them.
    ``exact``: Python integers (object arrays) in place of int64"""
    x0, y0, x1, y1, kind, size = p[:6]
    xs = (x0, x1) if kind == SEGMENT else (x0, x0)
    ys = (y0, y1) if kind == SEGMENT else (y0, y0)
    xa, xb = max(0, min(xs) - size), min(w, max(xs) + size + 1)
    ya, yb = max(0, min(ys) - size), min(h, max(ys) + size + 1)
    if xa >= xb or ya >= yb:
        return slice(0, 0), slice(0, 0), np.zeros((0, 0), bool)
    dt = object if exact else np.int64
    X = np.arange(xa, xb).astype(dt)[None, :]
    Y = np.arange(ya, yb).astype(dt)[:, None]
    ex, ey = X - x0, Y - y0
    d2 = ex * ex + ey * ey
    T2 = size * size
    if kind == DISC:
        m = d2 <= T2
    elif kind == RING:
        m = (d2 == 0) if size == 0 else ((d2 > (size - 1) ** 2) & (d2 <= T2))
    else:
        dx, dy = x1 - x0, y1 - y0
        L2 = dx * dx + dy * dy
        s = ex * dx + ey * dy
        fx, fy = X - x1, Y - y1
        cr = ex * dy - ey * dx
        m = np.where(s <= 0, 4 * d2 <= T2, np.where(s >= L2, 4 * (fx * fx + fy * fy) <= T2, 4 * cr * cr <= T2 * L2))
    return slice(ya, yb), slice(xa, xb), np.asarray(m, bool)


def draw(canvas, prims, exact=False):
    """O4: ``canvas`` [h, w, 3] with ``prims`` painted one after the other -> a new array"""
    out = np.array(canvas, np.uint8, copy=True)
    h, w = out.shape[:2]
    for p in prims:
        ys, xs, m = mask(p, w, h, exact)
        out[ys, xs][m] = p[6]
    return out


def cv_round(f):
    """cvRound of a float32: half to even; NaN and values outside int32 -> INT_MIN"""
    x = float(np.float32(f))
    if math.isnan(x) or not (-2147483649.0 < x < 2147483648.0):
        return INT_MIN
    return round(x)


class Rng:
    """cv::RNG as O6 recalls it, in Python integers"""

    def __init__(self, state=RNG_DEFAULT):
        self.state = int(state)

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def double(self):
        hi = self.next()
        return float((hi << 32) | self.next()) * 5.4210108624275221700372640043497e-20

    def colour(self):
        """the line colour of one match: r, g, b in this order -> (b, g, r)"""
        r, g, b = (int(self.double() * 255) for _ in range(3))
        return (b, g, r)


def match_prims(matches, h, rng, swap=False):
    """Processor.cpp:783-785: ring, ring, segment per match (u1, v1, u2, v2) on the stacked canvas"""
    out = []
    ring = RING_COLOUR[::-1] if swap else RING_COLOUR
    for u1, v1, u2, v2 in np.asarray(matches, np.int64).reshape(-1, 4).tolist():
        c = rng.colour()
        out += [prim(RING, u1, v1, size=1, colour=ring), prim(RING, u2, h + v2, size=1, colour=ring),
                prim(SEGMENT, u1, v1, u2, h + v2, 2, c[::-1] if swap else c)]
    return out


def match_canvases(imgs1, imgs2, matches, state=RNG_DEFAULT, swap=False):
    """-> ([n1 * n2, 2 h, w, 3], the advanced state): one generator through all pairs in row-major order"""
    rng = Rng(state)
    h = imgs1.shape[1]
    out = [draw(np.concatenate([imgs1[i], imgs2[j]], axis=0), match_prims(matches[i][j], h, rng, swap))
           for i in range(len(imgs1)) for j in range(len(imgs2))]
    return np.stack(out), rng.state


def sift_prims(keys):
    return [prim(DISC, cv_round(k[0]), cv_round(k[1]), size=1, colour=MARK_COLOUR) for k in np.asarray(keys, np.float32).reshape(-1, 4)]


def sift_canvases(views, keys):
    """a mark whose centre is INT_MIN (or anywhere off the canvas) paints nothing: ``mask`` clips it"""
    return np.stack([draw(v, [p for p in sift_prims(k) if abs(p[0]) <= 2 ** 20 and abs(p[1]) <= 2 ** 20]) for v, k in zip(views, keys)])
