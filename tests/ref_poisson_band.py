"""numpy / scipy restatement of the band levels of the Poisson stage (rules 24-31, csrc/poisson_band_rules.h) over tests/ref_poisson.py
(rules 1-13).  No code shared with the library: every level is a dense array over all nodes of its grid with NaN where a node has no value, the blocks are the
Chebyshev balls written as slices, every level is solved on its free nodes by scipy's conjugate gradients down to 1e-14 (a sparse
factorisation of the 125 000 free nodes of a level 6 takes minutes) with the residual it really reached entering every bound, and rule 31
is counted face by face.  Arrays over the nodes are indexed [iz, iy, ix], arrays over cells and blocks likewise."""
import math

import numpy as np

from tests import ref_poisson as R

BAND_MAX_DEPTH = 10
BLOCK = 4
NONE, FIXED, FREE = 0, 1, 2
BAND_DEFAULTS = dict(base_depth=8, band=2)


def pick_depth(P, o, side, prm):
    """rule 24: rule 3 with Dmax = min(depth_max, 10)"""
    D = prm["depth_min"]
    for d in range(prm["depth_min"], min(prm["depth_max"], BAND_MAX_DEPTH) + 1):
        if float(len(P)) >= prm["samples_per_node"] * float(R.occupied(P, o, side, d)):
            D = d
    return D


def active_blocks(P, o, side, l, band):
    """rule 26 -> bool [Gb, Gb, Gb]: the blocks within Chebyshev distance `band` of the block of some point"""
    Gb = 2 ** l // BLOCK
    act = np.zeros((Gb, Gb, Gb), bool)
    for bx, by, bz in np.unique(R.cells_at(P, o, side, l) // BLOCK, axis=0).tolist():
        act[max(bz - band, 0):bz + band + 1, max(by - band, 0):by + band + 1, max(bx - band, 0):bx + band + 1] = True
    return act


def cells_of(act):
    return act.repeat(BLOCK, 0).repeat(BLOCK, 1).repeat(BLOCK, 2)


def node_classes(cell):
    """rule 26 -> uint8 [n1, n1, n1]: FREE when the eight cells around a node are active, FIXED when some are, else NONE"""
    G = cell.shape[0]
    pad = np.pad(cell, 1).astype(np.int32)                  # cells outside the grid are not active
    cnt = np.zeros((G + 1,) * 3, np.int32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cnt += pad[dz:dz + G + 1, dy:dy + G + 1, dx:dx + G + 1]
    return np.where(cnt == 8, FREE, np.where(cnt > 0, FIXED, NONE)).astype(np.uint8)


def start_values(chi_below):
    """rule 27: 1/8 of the trilinear prolongation, along x, then y, then z; NaN spreads from the coarse nodes without a value"""
    c = chi_below
    m = c.shape[0]
    n1 = 2 * (m - 1) + 1
    a = np.empty((m, m, n1))
    a[:, :, ::2] = c
    a[:, :, 1::2] = 0.5 * (c[:, :, :-1] + c[:, :, 1:])
    b = np.empty((m, n1, n1))
    b[:, ::2] = a
    b[:, 1::2] = 0.5 * (a[:, :-1] + a[:, 1:])
    z = np.empty((n1, n1, n1))
    z[::2] = b
    z[1::2] = 0.5 * (b[:-1] + b[1:])
    return 0.125 * z


def laplacian_all(n1):
    """rule 7's stencil over all n1^3 nodes (rows of boundary nodes are never used)"""
    import scipy.sparse as sp
    T = sp.diags([np.ones(n1 - 1), -2.0 * np.ones(n1), np.ones(n1 - 1)], [-1, 0, 1], format="csr")
    I = sp.identity(n1, format="csr")
    return (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T)).tocsr()


def solve_level(P, Nn, o, side, l, band, chi_below):
    """rules 26-28 for level l -> dict(l, G, h, act, cell, cls, b, chi, rel, bnorm, n_active, n_free)"""
    from scipy.sparse.linalg import cg
    G = 2 ** l
    h = side / G
    act = active_blocks(P, o, side, l, band)
    cell = cells_of(act)
    cls = node_classes(cell)
    start = start_values(chi_below)
    assert start.shape == cls.shape and not np.isnan(start[cls != NONE]).any()          # rule 26's nesting
    b_all = R.rhs_of(R.splat(P, Nn, o, h, G), h)
    free = np.flatnonzero(cls.reshape(-1) == FREE)
    fixed = np.flatnonzero(cls.reshape(-1) == FIXED)
    rows = laplacian_all(G + 1)[free]
    A_ff, A_fc = rows[:, free].tocsc(), rows[:, fixed]
    assert A_ff.nnz + A_fc.nnz == rows.nnz                                                # every neighbour of a free node has a value
    bp = b_all.reshape(-1)[free] - A_fc @ start.reshape(-1)[fixed]
    bn = float(np.linalg.norm(bp))
    x = cg(-A_ff, -bp, rtol=1e-14, atol=0.0, maxiter=20000)[0] if bn > 0.0 else np.zeros(len(free))
    rel = float(np.linalg.norm(bp - A_ff @ x)) / bn if bn > 0.0 else 0.0
    chi = np.full(cls.size, np.nan)
    chi[fixed] = start.reshape(-1)[fixed]
    chi[free] = x
    b = np.full(cls.size, np.nan)
    b[fixed] = 0.0
    b[free] = b_all.reshape(-1)[free]
    return dict(l=l, G=G, h=h, act=act, cell=cell, cls=cls, b=b.reshape(cls.shape), chi=chi.reshape(cls.shape), rel=rel, bnorm=bn,
                n_active=int(act.sum()), n_free=len(free))


def edge_cells(pad, n1, d):
    """for the edges of direction d = (dx, dy, dz) at every lower node [n1 - dz, n1 - dy, n1 - dx]: -> (exists, open).  Rule 31 face
    by face: a face that contains the edge is normal to an axis the edge does not run along, lies in the node's plane on that axis and
    spans, along each other axis, the edge's own step or one of the two cells beside the node; the edge is open when such a face has an
    active cell on one side only.  pad: the cells with a layer of inactive ones around the grid."""
    shape = (n1 - d[2], n1 - d[1], n1 - d[0])

    def cell_at(off):                                       # the cell whose origin is the node minus off (x, y, z)
        return pad[1 - off[2]:1 - off[2] + shape[0], 1 - off[1]:1 - off[1] + shape[1], 1 - off[0]:1 - off[0] + shape[2]]

    if d == (1, 1, 1):
        return cell_at((0, 0, 0)).copy(), np.zeros(shape, bool)
    exists, opened = np.zeros(shape, bool), np.zeros(shape, bool)
    for a in range(3):
        if d[a]:
            continue
        u, v = [q for q in range(3) if q != a]
        for ou in ((0,) if d[u] else (0, 1)):
            for ov in ((0,) if d[v] else (0, 1)):
                if not d[u] and not d[v]:
                    continue
                lo, hi = [0, 0, 0], [0, 0, 0]
                lo[u] = hi[u] = ou
                lo[v] = hi[v] = ov
                lo[a], hi[a] = 1, 0
                exists |= cell_at(lo) | cell_at(hi)
                opened |= cell_at(lo) != cell_at(hi)
    return exists, opened


def extract(chi, iso, o, h, G, cell):
    """rules 30-31 -> (vertices, faces, gap, n_open_edges, open_vertex [V] bool): R.extract over the active cubes only"""
    n1 = G + 1
    inside = chi < iso                                      # NaN: False, and never looked at
    pad = np.pad(cell, 1)
    keys, va, vb, pa, pb, op = [], [], [], [], [], []
    for t, (dx, dy, dz) in enumerate(R.ETYPE):
        exists, opened = edge_cells(pad, n1, (dx, dy, dz))
        lo_in, hi_in = inside[:n1 - dz, :n1 - dy, :n1 - dx], inside[dz:, dy:, dx:]
        iz, iy, ix = np.nonzero(exists & (lo_in != hi_in))
        lo_v, hi_v = chi[iz, iy, ix], chi[iz + dz, iy + dy, ix + dx]
        assert not np.isnan(lo_v).any() and not np.isnan(hi_v).any()
        lo_p = np.stack([o[0] + h * ix.astype(np.float64), o[1] + h * iy.astype(np.float64), o[2] + h * iz.astype(np.float64)], 1)
        hi_p = np.stack([o[0] + h * (ix + dx).astype(np.float64), o[1] + h * (iy + dy).astype(np.float64), o[2] + h * (iz + dz).astype(np.float64)], 1)
        lo_is_in = lo_in[iz, iy, ix]
        keys.append(((iz * n1 + iy) * n1 + ix) * 7 + t)
        va.append(np.where(lo_is_in, lo_v, hi_v))
        vb.append(np.where(lo_is_in, hi_v, lo_v))
        pa.append(np.where(lo_is_in[:, None], lo_p, hi_p))
        pb.append(np.where(lo_is_in[:, None], hi_p, lo_p))
        op.append(opened[iz, iy, ix])
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    keys, va, vb, op = keys[order], np.concatenate(va)[order], np.concatenate(vb)[order], np.concatenate(op)[order]
    pa, pb = np.concatenate(pa)[order], np.concatenate(pb)[order]
    if len(keys) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int32), math.inf, 0, np.zeros(0, bool)
    verts = pa + ((iso - va) / (vb - va))[:, None] * (pb - pa)
    index = {int(k): i for i, k in enumerate(keys)}
    vl = verts.tolist()
    cin = np.zeros((G, G, G), np.int32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cin = cin + inside[dz:G + dz, dy:G + dy, dx:G + dx]
    corner_sets = [R.tet_corners(k) for k in range(6)]
    faces = []
    for cube in np.nonzero((cell & (cin > 0) & (cin < 8)).reshape(-1))[0].tolist():
        origin = (cube % G, cube // G % G, cube // (G * G))
        for k in range(6):
            corners = corner_sets[k]
            ins = [bool(inside[origin[2] + c[2], origin[1] + c[1], origin[0] + c[0]]) for c in corners]
            cyc, d = R.tet_cycle(corners, ins)
            if not cyc:
                continue
            idx = [index[R.edge_key(origin, corners, i, j, n1)] for i, j in cyc]
            idx = R.polygon(idx, [vl[i] for i in idx], d)
            faces.append((idx[0], idx[1], idx[2]))
            if len(idx) == 4:
                faces.append((idx[0], idx[2], idx[3]))
    return verts, np.asarray(faces, np.int32).reshape(-1, 3), float(np.abs(vb - va).min()), int(op.sum()), op


def reconstruct(points, normals, base_depth=8, band=2, **kw):
    """the whole call.  D <= base_depth: R.reconstruct's result, unchanged.  Otherwise dict(n_used, origin, side, h, depth, G,
    base_depth, base (R.reconstruct at depth B), levels {l: solve_level's dict}, chi (level D), iso, vertices, faces, gap,
    n_open_edges, open_vertex, P)"""
    prm = dict(R.DEFAULTS, **kw)
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    assert 3 <= base_depth <= R.MAX_DEPTH and 1 <= band <= 64 and 3 <= prm["depth_min"] <= BAND_MAX_DEPTH
    use = R.used_rows(points, normals)
    P, Nn = points[use], normals[use]
    if len(P) < 2 or not (P.max(0) - P.min(0)).max() > 0.0:
        raise R.Degenerate()
    o, side = R.cube_of(P, prm["scale"])
    D = pick_depth(P, o, side, prm)
    if D <= base_depth:
        return R.reconstruct(points, normals, **kw)
    B = base_depth
    G = 2 ** B
    hb = side / G
    rhs_b = R.rhs_of(R.splat(P, Nn, o, hb, G), hb)
    chi_b, rel_b = R.solve(rhs_b, G)
    base = dict(depth=B, G=G, h=hb, rhs=rhs_b, chi=chi_b, rel_residual=rel_b)
    levels, chi, cover = {}, chi_b, None
    for l in range(B + 1, D + 1):
        lv = solve_level(P, Nn, o, side, l, band, chi)
        if cover is not None:                               # rule 26: the level below covers this one
            assert cover.repeat(2, 0).repeat(2, 1).repeat(2, 2)[lv["act"]].all()
        levels[l], chi, cover = lv, lv["chi"], lv["act"]
    top = levels[D]
    iso = R.iso_of(P, top["chi"], o, top["h"], top["G"])
    verts, faces, gap, n_open, open_vertex = extract(top["chi"], iso, o, top["h"], top["G"], top["cell"])
    return dict(n_used=len(P), origin=o, side=side, h=top["h"], depth=D, G=top["G"], base_depth=B, base=base, levels=levels, chi=top["chi"],
                iso=iso, vertices=verts, faces=faces, gap=gap, n_open_edges=n_open, open_vertex=open_vertex, P=P)


# ------------------------------------------------------------------ what the tests measure ----
def accumulated_bound(ref, rel_of):
    """E_D: what stopping every solve at a relative residual can move any chi value of level D, and iso, by.  rel_of(l, level or base
    dict) is the relative residual of level l's solve.  A_ff is a principal submatrix of rule 7's matrix, so its smallest eigenvalue is
    not smaller (R.lambda_min); a change of the fixed values by at most e moves the solution by at most e (the maximum principle), and
    rule 27 hands an eighth of the level below's error on."""
    E = R.stop_bound(rel_of(ref["base_depth"], ref["base"]), ref["base"]["rhs"], ref["base_depth"])
    for l in sorted(ref["levels"]):
        lv = ref["levels"][l]
        E = rel_of(l, lv) * lv["bnorm"] / R.lambda_min(l) + 0.125 * E
    return E
