"""Scenes of the chain refinement tests (mvs_srt_refine): H, the three overlapping patches of one bumpy surface under a perturbed chain;
T, ties and exact thresholds on coordinates that every step represents exactly; E, the edges.  The restatement's results are computed
once per process and shared (reference())."""
import functools
import math

import numpy as np

from tests import ref_srt_refine as R

NAMES = ("H", "T", "E")


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def surface(x, y):
    """z = 0.15 sin 3x cos 2y + 0.1 x y + 0.05 cos 5y and its unit normal"""
    z = 0.15 * np.sin(3 * x) * np.cos(2 * y) + 0.1 * x * y + 0.05 * np.cos(5 * y)
    zx = 0.45 * np.cos(3 * x) * np.cos(2 * y) + 0.1 * y
    zy = -0.3 * np.sin(3 * x) * np.sin(2 * y) + 0.1 * x - 0.25 * np.sin(5 * y)
    n = np.stack([-zx, -zy, np.ones_like(z)], axis=-1)
    return np.stack([x, y, z], axis=-1), n / np.linalg.norm(n, axis=-1, keepdims=True)


def _patch(x0, x1, y0, y1, nx, ny, seed):
    rng = np.random.default_rng(seed)
    cx, cy = (x1 - x0) / nx, (y1 - y0) / ny
    gx, gy = np.meshgrid(x0 + (np.arange(nx) + 0.5) * cx, y0 + (np.arange(ny) + 0.5) * cy, indexing="ij")
    gx = gx + rng.uniform(-0.4, 0.4, gx.shape) * cx
    gy = gy + rng.uniform(-0.4, 0.4, gy.shape) * cy
    P, N = surface(gx.reshape(-1), gy.reshape(-1))
    return P, N


def _own(P, N, s, Rm, t):
    """world -> the own frame of the sequence whose chain entry is (s, R, t)"""
    return (P - t) @ Rm / s, N @ Rm


def mapped(sc, scales, Rs, ts):
    return [R.seq_apply(scales[k], Rs[k], ts[k], np.asarray(sc["points"][k], np.float64)) for k in range(len(sc["points"]))]


def rms_to_truth(sc, scales, Rs, ts):
    """rms distance of the mapped points of all sequences to where the true chain maps them"""
    d = np.concatenate(mapped(sc, scales, Rs, ts)) - np.concatenate(sc["world"])
    return float(np.sqrt((d * d).sum(axis=1).mean()))


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "H":
        ranges = ((-1.0, 0.2), (-0.5, 0.7), (-0.2, 1.0))
        true_s = [1.3, 0.8, 1.0]
        true_R = [_rot((1, 2, 3), 25.0), _rot((-2, 1, 0.5), -40.0), np.eye(3)]
        true_t = [np.array([0.3, -0.2, 0.5]), np.array([-0.4, 0.1, -0.3]), np.zeros(3)]
        world, pts, nrm = [], [], []
        for k, (x0, x1) in enumerate(ranges):
            P, N = _patch(x0, x1, -1.0, 1.0, 24, 24, 100 + k)
            world.append(P)
            p, n = _own(P, N, true_s[k], true_R[k], true_t[k])
            pts.append(np.ascontiguousarray(p))
            nrm.append(np.ascontiguousarray(n))
        # the input chain: the truth perturbed by about 2 degrees, 0.02 and 2 % per moving sequence
        dR = [_rot((0.3, 1, -0.5), 2.0), _rot((1, -0.4, 0.8), -2.0), np.eye(3)]
        dt = [np.array([0.012, -0.011, 0.012]), np.array([-0.011, 0.012, 0.011]), np.zeros(3)]
        dg = [1.02, 0.98, 1.0]
        s = [dg[k] * true_s[k] for k in range(3)]
        Rs = [dR[k] @ true_R[k] for k in range(3)]
        ts = [dg[k] * dR[k] @ true_t[k] + dt[k] for k in range(3)]
        return dict(points=pts, normals=nrm, scales=np.array(s), Rs=np.array(Rs), ts=np.array(ts), world=world,
                    true=(np.array(true_s), np.array(true_R), np.array(true_t)), params=R.params(rel_dist=0.05, min_cos=0.7))
    if name == "T":
        # World box (-8, -8, -4) .. (8, 8, 4): c = 0, D = 12.  Every designed point sits on the lattice u = 3/32, so x = y / 12 is a
        # multiple of 1/128; sequence 0 has scale 2 (own = world / 2), sequence 1 is the identity: both relative maps are exact.
        # cap = 2 rel_dist = 1/32 = 4 u.
        u = 3.0 / 32.0
        Z, Y, X, nX = (0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, -1)
        seq1 = [((0, 0, 0), Z), ((2, 0, 0), Z),                                          # 0, 1: the query at (1, 0, 0) is equidistant
                ((10, 1, 0), Z), ((12, 1, 0), Z), ((10, 3, 0), Z), ((12, 3, 0), Z),      # 2-5: (11, 2, 0) is equidistant from four
                ((20, 0, 0), Z), ((20, 0, 0), Z),                                        # 6, 7: coincident, and the query coincides too
                ((30, 0, 0), Y),                                                         # 8: the query at exactly the cap
                ((40, 0, 0), Y),                                                         # 9: the query just beyond it
                ((50, 0, 0), Z),                                                         # 10: normals at a right angle: the dot product is 0
                ((60, 0, 0), Z),                                                         # 11: opposite normals
                ((71, 0, 0), Z)]                                                         # 12: equidistant from two points of sequence 0
        seq0 = [((1, 0, 0), Z), ((11, 2, 0), Z), ((20, 0, 0), Z), ((30, 4, 0), Y), ((40, 4, 1), Y), ((50, 1, 0), X), ((60, 1, 0), nX),
                ((70, 0, 0), Z), ((72, 0, 0), Z)]
        w1 = np.array([p for p, _ in seq1], np.float64) * u
        w0 = np.array([p for p, _ in seq0], np.float64) * u
        w1 = np.concatenate([w1, [[-8.0, -8.0, -4.0], [8.0, 8.0, 4.0]]])                 # the corners of the box, far from everything
        n1 = np.array([n for _, n in seq1] + [Z, Z], np.float64)
        n0 = np.array([n for _, n in seq0], np.float64)
        return dict(points=[w0 / 2.0, w1], normals=[n0, n1], scales=np.array([2.0, 1.0]), Rs=np.array([np.eye(3), np.eye(3)]),
                    ts=np.zeros((2, 3)), world=[w0, w1], params=R.params(rel_dist=1.0 / 64.0, min_cos=0.0))
    if name == "E":
        # sequence 0: 130 points of the surface (fixed); sequence 1: 65 points over its middle, a little off; sequence 2: one point far
        # from both.  NaN and Inf coordinates and zero normals in both; points of sequence 1 far outside sequence 0's box.
        P0, N0 = _patch(-0.6, 0.6, -0.5, 0.5, 13, 10, 7)
        P1, N1 = _patch(-0.45, 0.45, -0.4, 0.4, 13, 5, 8)
        P0, N0, P1, N1 = P0.copy(), N0.copy(), P1.copy(), N1.copy()
        P0[5, 0] = np.nan
        P0[17] = np.inf
        P0[40, 2] = -np.inf
        N0[8] = 0.0
        N0[33] = 0.0
        N0[60, 1] = np.nan
        P1[3, 1] = np.nan                                       # a query (3 % 3 == 0)
        P1[9] = np.inf                                          # a query
        P1[10, 0] = -np.inf                                     # a target only
        P1[12] = (6.0, 5.0, 4.0)                                # queries far outside sequence 0's box
        P1[21] = (-7.0, 2.0, -3.0)
        N1[6] = 0.0                                            # a query whose match is rejected
        N1[7] = 0.0
        P2, N2 = np.array([[-6.0, -6.0, 5.0]]), np.array([[0.0, 0.0, 1.0]])
        true_s = [1.0, 1.25, 0.9]
        true_R = [np.eye(3), _rot((1, 1, 0), 30.0), _rot((0, 1, 1), 10.0)]
        true_t = [np.zeros(3), np.array([0.2, 0.1, -0.3]), np.array([0.5, 0.5, 0.5])]
        pts, nrm = [], []
        with np.errstate(all="ignore"):
            for k, (P, N) in enumerate(((P0, N0), (P1, N1), (P2, N2))):
                p, n = _own(P, N, true_s[k], true_R[k], true_t[k])
                bad = ~np.isfinite(P).all(axis=1)
                p[bad] = P[bad]                                  # (the map would smear one bad coordinate over all three)
                pts.append(np.ascontiguousarray(p))
                nrm.append(np.ascontiguousarray(n))
        pts[1][30] = (1e39, 0.0, 0.0)                            # a query: finite as fp64, not as float32
        pts[0][51, 1] = -3.5e38                                  # a target of the same kind
        s = [1.0, 1.25 * 1.01, 0.9]
        Rs = [np.eye(3), _rot((0.2, -1, 0.4), 1.0) @ true_R[1], true_R[2]]
        ts = [np.zeros(3), true_t[1] + np.array([0.01, -0.008, 0.012]), true_t[2]]
        return dict(points=pts, normals=nrm, scales=np.array(s), Rs=np.array(Rs), ts=np.array(ts), world=[P0, P1, P2],
                    params=R.params(rel_dist=0.02, min_cos=0.7, stride=3, fixed_seq=0, min_pairs=8))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's whole call on the scene with the scene's parameters (do not modify the result)"""
    sc = scene(name)
    return R.refine(sc["points"], sc["normals"], sc["scales"], sc["Rs"], sc["ts"], sc["params"])


@functools.lru_cache(maxsize=None)
def first_search(name, exact=False):
    """the restatement's sums for the scene's input chain -> (sums, c, D, details per pair)"""
    sc = scene(name)
    det = {}
    S, c, D = R.all_sums(sc["points"], sc["normals"], sc["scales"], sc["Rs"], sc["ts"], sc["params"], exact=exact, details=det)
    return S, c, D, det


def flat(S):
    """sums [n][n][121] of Python ints -> int64 [n, n, 121]"""
    return np.array(S, dtype=np.int64)
