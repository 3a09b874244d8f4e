"""numpy / scipy restatement of mvs_poisson_reconstruct (include/mvs.h, rules 1-13).  No code shared with the library: rules 1-7 with
np.add.at on int64, rule 8 by a sparse direct solve of the Kronecker-sum Laplacian, rules 9-12 as plain loops over the cubes the
surface crosses.  Arrays over the nodes are indexed [iz, iy, ix]; the flat order of a node is (iz * (G + 1) + iy) * (G + 1) + ix."""
import math

import numpy as np

MAX_DEPTH = 9
Q = 2.0 ** 36
DEFAULTS = dict(scale=1.1, samples_per_node=1.5, solve_tol=1e-8, depth_max=10, depth_min=7, max_cycles=64)
ETYPE = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]           # (dx, dy, dz) of edge types 0..6
TYPE_OF = {d: t for t, d in enumerate(ETYPE)}
TETS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]                       # xyz, xzy, yxz, yzx, zxy, zyx


class Degenerate(Exception):
    pass


def tet_corners(k):
    """the four corners of tetrahedron k as (dx, dy, dz) offsets from the cube origin"""
    q = [[0, 0, 0]]
    for axis in TETS[k]:
        nxt = list(q[-1])
        nxt[axis] += 1
        q.append(nxt)
    return [tuple(c) for c in q]


def used_rows(points, normals):
    return np.isfinite(points).all(1) & np.isfinite(normals).all(1)


def cube_of(P, scale):
    """rule 2 -> (o[3], side)"""
    lo, hi = P.min(0), P.max(0)
    c = 0.5 * (lo + hi)
    side = scale * (hi - lo).max()
    return c - 0.5 * side, side


def cells_at(P, o, side, d):
    """rule 3: the cell of every point at depth d, [N, 3] int64 (x, y, z)"""
    n = 2 ** d
    return np.clip(np.floor((P - o) / (side / n)), 0, n - 1).astype(np.int64)


def occupied(P, o, side, d):
    c = cells_at(P, o, side, d)
    n = 2 ** d
    return len(np.unique((c[:, 2] * n + c[:, 1]) * n + c[:, 0]))


def pick_depth(P, o, side, prm):
    dmax = min(prm["depth_max"], MAX_DEPTH)
    D = prm["depth_min"]
    for d in range(prm["depth_min"], dmax + 1):
        if float(len(P)) >= prm["samples_per_node"] * float(occupied(P, o, side, d)):
            D = d
    return D


def corners_weights(P, o, h, G):
    """rule 5 per point: i0 [N, 3] and, for corner c = bx + 2 by + 4 bz, its weight w[c] [N] = (wx * wy) * wz"""
    g = (P - o) / h
    i0 = np.clip(np.floor(g), 0, G - 1)
    f = g - i0
    i0 = i0.astype(np.int64)
    w = []
    for c in range(8):
        wx = f[:, 0] if c & 1 else 1.0 - f[:, 0]
        wy = f[:, 1] if c & 2 else 1.0 - f[:, 1]
        wz = f[:, 2] if c & 4 else 1.0 - f[:, 2]
        w.append((wx * wy) * wz)
    return i0, w


def splat(P, Nn, o, h, G):
    """rule 5 -> int64 sums [3][n1, n1, n1]"""
    n1 = G + 1
    i0, w = corners_weights(P, o, h, G)
    S = np.zeros((3, n1 * n1 * n1), np.int64)
    for c in range(8):
        node = ((i0[:, 2] + (c >> 2 & 1)) * n1 + i0[:, 1] + (c >> 1 & 1)) * n1 + i0[:, 0] + (c & 1)
        for a in range(3):
            np.add.at(S[a], node, np.rint((w[c] * Nn[:, a]) * Q).astype(np.int64))
    return S.reshape(3, n1, n1, n1)


def rhs_of(S, h):
    """rule 6 -> b [n1, n1, n1], zero on the boundary"""
    V = S.astype(np.float64) * (1.0 / Q)
    b = np.zeros(V.shape[1:])
    b[1:-1, 1:-1, 1:-1] = (((V[0][1:-1, 1:-1, 2:] - V[0][1:-1, 1:-1, :-2]) + (V[1][1:-1, 2:, 1:-1] - V[1][1:-1, :-2, 1:-1])) +
                           (V[2][2:, 1:-1, 1:-1] - V[2][:-2, 1:-1, 1:-1])) * (0.5 * h)
    return b


def laplacian(G):
    import scipy.sparse as sp
    m = G - 1
    T = sp.diags([np.ones(m - 1), -2.0 * np.ones(m), np.ones(m - 1)], [-1, 0, 1], format="csr")
    I = sp.identity(m, format="csr")
    return (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsc()


def solve(b, G):
    """rules 7-8 -> (chi [n1, n1, n1], relative residual of the direct solve)"""
    from scipy.sparse.linalg import spsolve
    A = laplacian(G)
    rhs = b[1:-1, 1:-1, 1:-1].reshape(-1)
    x = spsolve(A, rhs, permc_spec="MMD_AT_PLUS_A") if G > 2 else rhs / -6.0
    x = np.atleast_1d(x)
    bn = float(np.linalg.norm(rhs))
    rel = float(np.linalg.norm(rhs - A @ x)) / bn if bn > 0.0 else 0.0
    chi = np.zeros_like(b)
    chi[1:-1, 1:-1, 1:-1] = x.reshape(G - 1, G - 1, G - 1)
    return chi, rel


def iso_of(P, chi, o, h, G):
    """rule 9"""
    i0, w = corners_weights(P, o, h, G)
    val = np.zeros(len(P))
    for c in range(8):
        val = val + w[c] * chi[i0[:, 2] + (c >> 2 & 1), i0[:, 1] + (c >> 1 & 1), i0[:, 0] + (c & 1)]
    return float(val.sum() / float(len(P)))


def polygon(idx, pos, d):
    """rule 12 for one cycle of vertex indices idx with positions pos (a triangle or the quad AC, AD, BD, BC) and d = mean(O) - mean(I):
    the oriented, rotated cycle"""
    def cross(a, b):
        return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])

    def sub(a, b):
        return (a[0] - b[0], a[1] - b[1], a[2] - b[2])

    n = cross(sub(pos[1], pos[0]), sub(pos[2], pos[0]))
    if len(idx) == 4:
        m = cross(sub(pos[2], pos[0]), sub(pos[3], pos[0]))
        n = (n[0] + m[0], n[1] + m[1], n[2] + m[2])
    if (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2] < 0.0:
        idx = idx[::-1]
    k = idx.index(min(idx))
    return idx[k:] + idx[:k]


def tet_cycle(corners, inside):
    """the I-O edges of a tetrahedron as (corner, corner) pairs, in the listed order, and d = mean(O) - mean(I) in cell units"""
    I = [i for i in range(4) if inside[i]]
    O = [i for i in range(4) if not inside[i]]
    if not I or not O:
        return [], None
    if len(I) == 1:
        cyc = [(I[0], j) for j in O]
    elif len(I) == 3:
        cyc = [(i, O[0]) for i in I]
    else:
        cyc = [(I[0], O[0]), (I[0], O[1]), (I[1], O[1]), (I[1], O[0])]
    d = tuple(sum(corners[j][a] for j in O) / float(len(O)) - sum(corners[i][a] for i in I) / float(len(I)) for a in range(3))
    return cyc, d


def edge_key(origin, corners, i, j, n1):
    """(node index, type) of the edge between corners i and j of a tetrahedron of the cube at `origin` (ix, iy, iz)"""
    lo, hi = (i, j) if i < j else (j, i)
    a, b = corners[lo], corners[hi]
    node = ((origin[2] + a[2]) * n1 + origin[1] + a[1]) * n1 + origin[0] + a[0]
    return node * 7 + TYPE_OF[(b[0] - a[0], b[1] - a[1], b[2] - a[2])]


def extract(chi, iso, o, h, G):
    """rules 10-13 -> (vertices [V, 3], faces [F, 3] int32, gap = min |chi_b - chi_a| over the crossed edges)"""
    n1 = G + 1
    inside = chi < iso
    keys, va, vb, pa, pb = [], [], [], [], []
    for t, (dx, dy, dz) in enumerate(ETYPE):
        lo_in, hi_in = inside[:n1 - dz, :n1 - dy, :n1 - dx], inside[dz:, dy:, dx:]
        iz, iy, ix = np.nonzero(lo_in != hi_in)
        lo_v, hi_v = chi[iz, iy, ix], chi[iz + dz, iy + dy, ix + dx]
        lo_p = np.stack([o[0] + h * ix.astype(np.float64), o[1] + h * iy.astype(np.float64), o[2] + h * iz.astype(np.float64)], 1)
        hi_p = np.stack([o[0] + h * (ix + dx).astype(np.float64), o[1] + h * (iy + dy).astype(np.float64), o[2] + h * (iz + dz).astype(np.float64)], 1)
        lo_is_in = lo_in[iz, iy, ix]
        keys.append(((iz * n1 + iy) * n1 + ix) * 7 + t)
        va.append(np.where(lo_is_in, lo_v, hi_v))
        vb.append(np.where(lo_is_in, hi_v, lo_v))
        pa.append(np.where(lo_is_in[:, None], lo_p, hi_p))
        pb.append(np.where(lo_is_in[:, None], hi_p, lo_p))
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    keys, va, vb = keys[order], np.concatenate(va)[order], np.concatenate(vb)[order]
    pa, pb = np.concatenate(pa)[order], np.concatenate(pb)[order]
    if len(keys) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int32), math.inf
    t = (iso - va) / (vb - va)
    verts = pa + t[:, None] * (pb - pa)
    index = {int(k): i for i, k in enumerate(keys)}
    vl = verts.tolist()
    cin = inside[:-1, :-1, :-1].astype(np.int32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                if dx or dy or dz:
                    cin = cin + inside[dz:G + dz, dy:G + dy, dx:G + dx]
    corner_sets = [tet_corners(k) for k in range(6)]
    faces = []
    for cube in np.nonzero(((cin > 0) & (cin < 8)).reshape(-1))[0].tolist():
        origin = (cube % G, cube // G % G, cube // (G * G))
        for k in range(6):
            corners = corner_sets[k]
            ins = [bool(inside[origin[2] + c[2], origin[1] + c[1], origin[0] + c[0]]) for c in corners]
            cyc, d = tet_cycle(corners, ins)
            if not cyc:
                continue
            idx = [index[edge_key(origin, corners, i, j, n1)] for i, j in cyc]
            idx = polygon(idx, [vl[i] for i in idx], d)
            faces.append((idx[0], idx[1], idx[2]))
            if len(idx) == 4:
                faces.append((idx[0], idx[2], idx[3]))
    return verts, np.asarray(faces, np.int32).reshape(-1, 3), float(np.abs(vb - va).min())


def reconstruct(points, normals, **kw):
    """the whole call -> dict(n_used, origin, h, depth, G, rhs, chi, rel_residual (of the direct solve), iso, vertices, faces, gap)"""
    prm = dict(DEFAULTS, **kw)
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    assert prm["depth_min"] >= 3 and prm["scale"] > 1.0 + 4.0 / 2 ** prm["depth_min"]          # what the library refuses
    use = used_rows(points, normals)
    P, Nn = points[use], normals[use]
    if len(P) < 2 or not (P.max(0) - P.min(0)).max() > 0.0:
        raise Degenerate()
    o, side = cube_of(P, prm["scale"])
    D = pick_depth(P, o, side, prm)
    G = 2 ** D
    h = side / G
    b = rhs_of(splat(P, Nn, o, h, G), h)
    chi, rel = solve(b, G)
    iso = iso_of(P, chi, o, h, G)
    verts, faces, gap = extract(chi, iso, o, h, G)
    return dict(n_used=len(P), origin=o, side=side, h=h, depth=D, G=G, rhs=b, chi=chi, rel_residual=rel, iso=iso, vertices=verts, faces=faces,
                gap=gap, P=P)


# ------------------------------------------------------------------ what the tests measure ----
def lambda_min(D):
    """the smallest eigenvalue (in magnitude) of rule 7's matrix"""
    return 12.0 * math.sin(math.pi / 2 ** (D + 1)) ** 2


def stop_bound(rel, b, D):
    """E: what a relative residual `rel` can move any chi value, and iso, by"""
    return rel * float(np.linalg.norm(b)) / lambda_min(D)


def mesh_properties(verts, faces):
    """-> (every directed edge once with its reverse once, V - E + F, components, signed volume)"""
    f = np.asarray(faces, np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    code = de[:, 0] * (len(verts) + 1) + de[:, 1]
    rev = de[:, 1] * (len(verts) + 1) + de[:, 0]
    closed = len(np.unique(code)) == len(code) and np.array_equal(np.sort(code), np.sort(rev))
    parent = list(range(len(verts)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b in de.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    used = np.unique(f)
    comps = len({find(int(i)) for i in used})
    euler = len(used) - len(code) // 2 + len(f)
    p0, p1, p2 = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    vol = float((p0 * np.cross(p1, p2)).sum() / 6.0)
    return closed, euler, comps, vol
