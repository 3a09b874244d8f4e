"""numpy restatement of rules 14-18 of include/mvs.h (mvs_poisson_reconstruct_density, mvs_mesh_trim_by_value) on top of
tests/ref_poisson.py, which holds rules 1-13.  No code shared with the library: the node sums of rule 14 and the sum behind rho_mean
with np.add.at on int64, the trim in plain numpy.  Arrays over the nodes of the density grid are flat, in node order
(iz * (Gd + 1) + iy) * (Gd + 1) + ix."""
import math

import numpy as np

from tests import ref_poisson as R

Q = 2.0 ** 36
QR = 2.0 ** 16
DEFAULTS = dict(max_gain=4.0, weight=False, density_drop=1)


def density_grid(side, D, drop):
    """rule 14 -> (Dd, Gd, hd)"""
    Dd = max(D - drop, 2)
    Gd = 2 ** Dd
    return Dd, Gd, side / Gd


def node_of(i0, c, n1):
    return ((i0[:, 2] + (c >> 2 & 1)) * n1 + i0[:, 1] + (c >> 1 & 1)) * n1 + i0[:, 0] + (c & 1)


def density_sums(P, o, hd, Gd):
    """rule 14 -> int64 node sums [(Gd + 1)^3]"""
    n1 = Gd + 1
    i0, w = R.corners_weights(P, o, hd, Gd)
    S = np.zeros(n1 * n1 * n1, np.int64)
    for c in range(8):
        np.add.at(S, node_of(i0, c, n1), np.rint(w[c] * Q).astype(np.int64))
    return S


def density_at(X, S, o, hd, Gd):
    """rules 15 and 17: the trilinear W at the rows of X, added in corner order"""
    n1 = Gd + 1
    W = S.astype(np.float64) * (1.0 / Q)
    i0, w = R.corners_weights(X, o, hd, Gd)
    val = np.zeros(len(X))
    for c in range(8):
        val = val + w[c] * W[node_of(i0, c, n1)]
    return val


def mean_density(rho):
    """rule 15: the order-free mean"""
    q = np.zeros(1, np.int64)
    np.add.at(q, np.zeros(len(rho), np.int64), np.rint(rho * QR).astype(np.int64))
    return float(q[0]) * (1.0 / QR) / float(len(rho))


def gains(rho, rho_mean, max_gain):
    """rule 16 -> (s_p, n_clamped)"""
    with np.errstate(divide="ignore"):
        ratio = rho_mean / rho                                            # rho = 0: infinity, cut at max_gain
    return np.minimum(ratio, max_gain), int((ratio > max_gain).sum())


def trim(n_vertices, faces, values, threshold):
    """rule 18 -> (indices of the kept vertices, ascending; the kept faces, renumbered, int32)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    passes = np.asarray(values, np.float64) >= threshold                 # NaN does not pass
    keep_f = passes[faces].all(1) if len(faces) else np.zeros(0, bool)
    ref = np.zeros(n_vertices, bool)
    ref[faces[keep_f].reshape(-1)] = True
    kept = np.nonzero(ref)[0]
    renum = np.full(n_vertices, -1, np.int64)
    renum[kept] = np.arange(len(kept))
    return kept, renum[faces[keep_f]].astype(np.int32).reshape(-1, 3)


def reconstruct(points, normals, max_gain=4.0, weight=False, density_drop=1, **kw):
    """mvs_poisson_reconstruct_density -> the dict of ref_poisson.reconstruct plus density_depth, Gd, hd, node_sums, rho, rho_mean, gain,
    n_clamped and vertex_density"""
    prm = dict(R.DEFAULTS, **kw)
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    assert prm["depth_min"] >= 3 and prm["scale"] > 1.0 + 4.0 / 2 ** prm["depth_min"]
    assert 1.0 <= max_gain <= 16.0 and 0 <= density_drop <= 8 and (not weight or len(points) <= 2 ** 22)
    use = R.used_rows(points, normals)
    P, Nn = points[use], normals[use]
    if len(P) < 2 or not (P.max(0) - P.min(0)).max() > 0.0:
        raise R.Degenerate()
    o, side = R.cube_of(P, prm["scale"])
    D = R.pick_depth(P, o, side, prm)
    G = 2 ** D
    h = side / G
    Dd, Gd, hd = density_grid(side, D, density_drop)
    S = density_sums(P, o, hd, Gd)
    rho = density_at(P, S, o, hd, Gd)
    rho_mean = mean_density(rho)
    s, n_clamped = gains(rho, rho_mean, max_gain)
    b = R.rhs_of(R.splat(P, Nn * s[:, None] if weight else Nn, o, h, G), h)       # rule 16: x = w * (n_a * s_p)
    chi, rel = R.solve(b, G)
    iso = R.iso_of(P, chi, o, h, G)                                                # unweighted point values
    verts, faces, gap = R.extract(chi, iso, o, h, G)
    dv = density_at(verts, S, o, hd, Gd) if len(verts) else np.zeros(0)
    return dict(n_used=len(P), origin=o, side=side, h=h, depth=D, G=G, rhs=b, chi=chi, rel_residual=rel, iso=iso, vertices=verts, faces=faces,
                gap=gap, P=P, density_depth=Dd, Gd=Gd, hd=hd, node_sums=S, rho=rho, rho_mean=rho_mean, gain=s, n_clamped=n_clamped,
                vertex_density=dv)


# ------------------------------------------------------------------ what the tests measure ----
def radial_rms(verts, centre, radius, h):
    """rms and max of | |v - centre| - radius |, in cells"""
    e = np.abs(np.sqrt(((verts - np.asarray(centre)) ** 2).sum(1)) - radius) / h
    return float(np.sqrt((e ** 2).mean())), float(e.max())


def boundary_loops(faces):
    """-> (loops of unpaired directed edges, True when every unpaired edge lies on a simple loop and no edge is used twice in one
    direction)"""
    f = np.asarray(faces, np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    m = int(f.max()) + 1 if len(f) else 1
    code, rev = de[:, 0] * m + de[:, 1], de[:, 1] * m + de[:, 0]
    if len(np.unique(code)) != len(code):
        return 0, False
    open_e = de[~np.isin(code, rev)]
    nxt = {}
    for a, b in open_e.tolist():
        if a in nxt:
            return 0, False
        nxt[a] = b
    loops, seen = 0, set()
    for start in nxt:
        if start in seen:
            continue
        at = start
        while at not in seen:
            seen.add(at)
            if at not in nxt:
                return 0, False
            at = nxt[at]
        if at != start:
            return 0, False
        loops += 1
    return loops, True


def max_density(S):
    return float(S.max()) / Q


def vertex_density_bound(B, hd, S):
    """what a vertex displacement of at most B moves d_v by: the displacement times the density's largest slope.  W is trilinear, so
    along an axis it changes by (the difference of two node values) / hd per unit length, a convex combination of four such differences;
    node values lie in [0, max W], which bounds the slope by max(W) / hd.  -> B / hd * max(W)"""
    return B / hd * max_density(S)
