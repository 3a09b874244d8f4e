"""numpy / scipy restatement of rules 19-23 of include/mvs.h (mvs_poisson_reconstruct_screened) on top of tests/ref_poisson.py (rules
1-13) and tests/ref_poisson_density.py (rules 14-17).  No code shared with the library: the stencil of rule 20 with np.add.at on int64,
the operator of rule 21 as a scipy sparse matrix over the interior nodes, rule 22 by a sparse direct solve (up to D = 4) or by conjugate
gradients to 1e-13 (from D = 5 on, where a direct factorisation of the 3-D operator takes a test too long).  The stencil is dense,
[(G + 1)^3, 27] int64 in node order and the offset order (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1).

The target T of rule 21 is the iso value of the FIRST solve, so it carries that solve's stopping error and two solvers cannot agree on
its bits; everything downstream of T (f, chi, the mesh) is therefore a function of T here: `screened(ref, T)` evaluates rules 21-23 for
any T on the matrix kept in the reference, so a test can hand in the device's T and compare the rest exactly or to the bound."""
import math

import numpy as np

from tests import ref_poisson as R, ref_poisson_density as RD

QS = 2.0 ** 30
DEFAULTS = dict(alpha=4.0)
CG_FROM_DEPTH = 5                 # from this depth on both solves run by conjugate gradients


def offset_index(dx, dy, dz):
    return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)


def screen_lambda(alpha, N, occ):
    """rule 19"""
    return alpha / max(1.0, float(N) / float(occ))


def stencil_sums(P, o, h, G, lam):
    """rule 20 -> int64 [(G + 1)^3, 27]"""
    n1 = G + 1
    i0, w = R.corners_weights(P, o, h, G)
    S = np.zeros(n1 * n1 * n1 * 27, np.int64)
    node = [RD.node_of(i0, c, n1) for c in range(8)]
    for c1 in range(8):
        for c2 in range(c1, 8):
            d = ((c2 & 1) - (c1 & 1), (c2 >> 1 & 1) - (c1 >> 1 & 1), (c2 >> 2 & 1) - (c1 >> 2 & 1))
            q = np.rint(((lam * w[c1]) * w[c2]) * QS).astype(np.int64)
            np.add.at(S, node[c1] * 27 + offset_index(*d), q)
            if c1 != c2:
                np.add.at(S, node[c2] * 27 + offset_index(-d[0], -d[1], -d[2]), q)
    return S.reshape(-1, 27)


def row_sums(S):
    """rs of rule 20 -> (int64 sums [(G + 1)^3], the doubles)"""
    q = S.sum(1, dtype=np.int64)
    return q, q.astype(np.float64) * (1.0 / QS)


def touch_counts(P, o, h, G):
    """the used points that touch every node, [(G + 1)^3]"""
    n1 = G + 1
    i0, _ = R.corners_weights(P, o, h, G)
    cnt = np.zeros(n1 * n1 * n1, np.int64)
    for c in range(8):
        np.add.at(cnt, RD.node_of(i0, c, n1), 1)
    return cnt


def quantisation_norm(cnt):
    """a bound on the 2-norm of (quantised S - exact S): a point adds 8 entries to the row of a node it touches, each rounded by at most
    half a unit of 2^-30; the matrix is symmetric, so its 2-norm is at most its largest absolute row sum"""
    return float(cnt.max()) * 8.0 * 0.5 / QS


def screen_matrix(S, G):
    """the S part of rule 21 over the interior nodes (a column at a boundary node multiplies chi = 0 and is dropped), csr"""
    import scipy.sparse as sp
    n1, m = G + 1, G - 1
    Sv = S.reshape(n1, n1, n1, 27)[1:-1, 1:-1, 1:-1].astype(np.float64) * (1.0 / QS)
    iz, iy, ix = np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij")
    rows, cols, vals = [], [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                v = Sv[..., offset_index(dx, dy, dz)]
                jz, jy, jx = iz + dz, iy + dy, ix + dx
                ok = (v != 0.0) & (jz >= 0) & (jz < m) & (jy >= 0) & (jy < m) & (jx >= 0) & (jx < m)
                rows.append(((iz * m + iy) * m + ix)[ok])
                cols.append(((jz * m + jy) * m + jx)[ok])
                vals.append(v[ok])
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m ** 3, m ** 3))


def operator(S, G):
    """M of rule 21 over the interior nodes, csc"""
    return (R.laplacian(G) - screen_matrix(S, G)).tocsc()


def _cg(Mneg, rhs, x0):
    """conjugate gradients on the positive definite -M to a relative residual of 1e-13: the recurrence stops at half of that, the
    callers measure the true residual"""
    from scipy.sparse.linalg import cg
    x, flag = cg(Mneg, -rhs, x0=x0, rtol=5e-14, atol=0.0, maxiter=20000)
    assert flag == 0
    return x


def _embed(x, G):
    chi = np.zeros((G + 1, G + 1, G + 1))
    chi[1:-1, 1:-1, 1:-1] = x.reshape(G - 1, G - 1, G - 1)
    return chi


def first_solve(b, G):
    """rules 7-8 as ref_poisson.solve, by conjugate gradients from CG_FROM_DEPTH on -> (chi0, relative residual)"""
    if G < 2 ** CG_FROM_DEPTH:
        return R.solve(b, G)
    A = R.laplacian(G)
    rhs = b[1:-1, 1:-1, 1:-1].reshape(-1)
    x = _cg(-A, rhs, None)
    return _embed(x, G), float(np.linalg.norm(rhs - A @ x) / np.linalg.norm(rhs))


def rhs_screened(b, rs, T):
    """rule 21: f = b - T * rs at interior nodes (rs is zero elsewhere: the scale check keeps every touched node interior)"""
    return b - T * rs.reshape(b.shape)


def screened(ref, T):
    """rules 21-23 for the target T on the reference `ref` of reconstruct -> dict(f, chi, rel_residual, iso, vertices, faces, gap,
    vertex_density)"""
    G, M = ref["G"], ref["M"]
    f = rhs_screened(ref["rhs"], ref["rs"], T)
    rhs = f[1:-1, 1:-1, 1:-1].reshape(-1)
    fn = float(np.linalg.norm(rhs))
    if fn == 0.0:
        x = ref["chi0"][1:-1, 1:-1, 1:-1].reshape(-1)
    elif G < 2 ** CG_FROM_DEPTH:
        from scipy.sparse.linalg import spsolve
        x = spsolve(M, rhs, permc_spec="MMD_AT_PLUS_A")
    else:
        x = _cg(-M, rhs, ref["chi0"][1:-1, 1:-1, 1:-1].reshape(-1))
    rel = float(np.linalg.norm(rhs - M @ x)) / fn if fn > 0.0 else 0.0
    chi = _embed(x, G)
    iso = R.iso_of(ref["P"], chi, ref["origin"], ref["h"], G)
    verts, faces, gap = R.extract(chi, iso, ref["origin"], ref["h"], G)
    dv = RD.density_at(verts, ref["node_sums"], ref["origin"], ref["hd"], ref["Gd"]) if len(verts) else np.zeros(0)
    return dict(f=f, chi=chi, rel_residual=rel, iso=iso, vertices=verts, faces=faces, gap=gap, vertex_density=dv)


def reconstruct(points, normals, alpha=4.0, max_gain=4.0, weight=False, density_drop=1, **kw):
    """mvs_poisson_reconstruct_screened -> a dict: grid and density as ref_poisson_density.reconstruct (rhs = b, chi0, rel_residual0 and
    iso0 = T of the first solve), occupied, lam, stencil, rs_q / rs, touch, M, and
    the fields of screened(ref, T) for the restatement's own T.  alpha = 0: stencil and rs are zero and the result is the first solve's."""
    prm = dict(R.DEFAULTS, **kw)
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    assert prm["depth_min"] >= 3 and prm["scale"] > 1.0 + 4.0 / 2 ** prm["depth_min"] and 0.0 <= alpha <= 64.0
    use = R.used_rows(points, normals)
    P, Nn = points[use], normals[use]
    if len(P) < 2 or not (P.max(0) - P.min(0)).max() > 0.0:
        raise R.Degenerate()
    o, side = R.cube_of(P, prm["scale"])
    D = R.pick_depth(P, o, side, prm)
    G = 2 ** D
    h = side / G
    Dd, Gd, hd = RD.density_grid(side, D, density_drop)
    Sd = RD.density_sums(P, o, hd, Gd)
    rho = RD.density_at(P, Sd, o, hd, Gd)
    rho_mean = RD.mean_density(rho)
    s, n_clamped = RD.gains(rho, rho_mean, max_gain)
    b = R.rhs_of(R.splat(P, Nn * s[:, None] if weight else Nn, o, h, G), h)
    chi0, rel0 = first_solve(b, G)
    T = R.iso_of(P, chi0, o, h, G)
    occ = R.occupied(P, o, side, D)
    lam = screen_lambda(alpha, len(P), occ) if alpha > 0.0 else 0.0
    S = stencil_sums(P, o, h, G, lam) if alpha > 0.0 else np.zeros(((G + 1) ** 3, 27), np.int64)
    rs_q, rs = row_sums(S)
    M = operator(S, G)
    ref = dict(n_used=len(P), origin=o, side=side, h=h, depth=D, G=G, rhs=b, chi0=chi0, rel_residual0=rel0, iso0=T, P=P, density_depth=Dd, Gd=Gd, hd=hd,
               node_sums=Sd, rho=rho, rho_mean=rho_mean, gain=s, n_clamped=n_clamped, alpha=alpha, occupied=occ, lam=lam, stencil=S, rs_q=rs_q, rs=rs,
               touch=touch_counts(P, o, h, G), M=M)
    if alpha > 0.0:
        ref.update(screened(ref, T))
    else:
        verts, faces, gap = R.extract(chi0, T, o, h, G)
        dv = RD.density_at(verts, Sd, o, hd, Gd) if len(verts) else np.zeros(0)
        ref.update(f=b, chi=chi0, rel_residual=rel0, iso=T, vertices=verts, faces=faces, gap=gap, vertex_density=dv)
    return ref


# ------------------------------------------------------------------ what the tests measure ----
def lambda_min_screened(ref):
    """a lower bound on the smallest eigenvalue of -M: the exact S is a sum of lambda w w^T and positive semi-definite, so -M lies above
    the Laplacian's lambda_min less the norm of the quantisation"""
    return R.lambda_min(ref["depth"]) - quantisation_norm(ref["touch"])


def stop_bound(rel, f, ref):
    """E of ref_poisson.stop_bound for the screened solve: what a relative residual `rel` against |f| can move any chi value, and iso, by"""
    return rel * float(np.linalg.norm(f)) / lambda_min_screened(ref)


def smallest_eigenvalue(ref):
    """the smallest eigenvalue of -M by Lanczos: a Ritz value, so never below the true one, converged to a relative 1e-6"""
    from scipy.sparse.linalg import eigsh
    val = eigsh(-ref["M"], k=1, which="SA", return_eigenvectors=False, tol=1e-6, ncv=64, maxiter=100000, v0=np.ones(ref["M"].shape[0]))
    return float(val[0])
