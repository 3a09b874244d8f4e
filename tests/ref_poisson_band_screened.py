"""numpy / scipy restatement of rules 36-41 of include/mvs.h (mvs_poisson_reconstruct_band_screened): the band levels of
tests/ref_poisson_band.py and the sampling density of tests/ref_poisson_band_density.py with the screening of tests/ref_poisson_screened.py
on the base level and on every band level.  Composed from those and tests/ref_poisson.py without a line of theirs changed, and no code
shared with the library: every level is a dense array over all nodes of its grid, the stencil of a level is dense [(G + 1)^3, 27] int64,
the operator of rule 40 a scipy sparse matrix over the free nodes, and every solve runs by conjugate gradients with the residual it
really reached entering every bound.

accumulated_bound, derived.  Every error below is a 2-norm over the nodes of a level that have a value (so it bounds every single value).
 base     chi0 is off by e0 <= rel0 |b| / lmin(B) (ref_poisson.stop_bound).  T_B = g . chi0 with g = (1 / N) sum_p (the eight weights of
          p at its corners), so |dT_B| <= |g| e0.  The screened chi_B solves M chi = b - T_B rs, which does not depend on chi0
          otherwise, so it is off by at most E_B = (rel_s |f| + |g| |rs| e0) / lmin_s(B), lmin_s(B) = lmin(B) - |quantisation of S|
          <= the smallest eigenvalue of -M (ref_poisson_screened.lambda_min_screened: the exact S is a sum of lambda w w^T, positive
          semi-definite).
 level l  S has positive off-diagonal entries, so M is no M-matrix and the maximum principle of ref_poisson_band.accumulated_bound does
          not hold; errors are carried by norms.  M_ff is a principal submatrix of M, so lmin(-M_ff) >= lmin(-M) >= lmin(l) - |quantisation|;
          but that is the full grid's eigenvalue (0.0072 at level 6) while the free nodes form a band a few blocks wide, whose smallest
          eigenvalue is an order of magnitude larger, and a factor 1 / lmin is paid per level.  lmin_s(l) is therefore 0.99 times the
          smallest Ritz value of -M_ff itself, by Lanczos from the vector of ones, converged to a relative 1e-4 (a Ritz value is never
          below the smallest eigenvalue; the margin of 1 % covers its convergence), and never less than the full grid's bound.
          The start values are 1/8 of the trilinear prolongation of chi_(l-1).  Per axis the prolongation copies a value and puts
          half of each of two values on a midpoint: its 1-norm is 2 and its infinity norm 1, so its 2-norm is at most sqrt(2), and that
          of the three axes sqrt(8): the start values are off by es <= sqrt(8) / 8 E_(l-1).
          T_l = g . start with the g of level l, so |dT_l| <= |g| es.
          f' = b - T_l rs - A_fc chi_c, so |df'| <= |dT_l| |rs| + |A_fc| es with |A_fc| <= sqrt(|A_fc|_1 |A_fc|_inf), and with the
          stop at the relative residual rel_l against |f'|
              E_l = max(es, (rel_l |f'| + (|g| |rs| + sqrt(|A_fc|_1 |A_fc|_inf)) es) / lmin_s(l))
          (the fixed nodes carry es itself).  iso = g_D . chi_D with |g_D| <= 1 is off by at most E_D.
Arrays over the nodes are indexed [iz, iy, ix]."""
import math

import numpy as np

from tests import ref_poisson as R, ref_poisson_band as RB, ref_poisson_band_density as RBD, ref_poisson_density as RD, ref_poisson_screened as RS


def mean_weights(P, o, h, G):
    """g of the derivation above -> [(G + 1)^3]: T = g . chi is rule 29's mean (up to the order of the sums)"""
    n1 = G + 1
    i0, w = R.corners_weights(P, o, h, G)
    g = np.zeros(n1 ** 3)
    for c in range(8):
        np.add.at(g, RD.node_of(i0, c, n1), w[c])
    return g / float(len(P))


def solve_base(P, Nw, o, side, B, alpha):
    """rule 37 -> dict(depth, G, h, rhs, chi0, rel0, T, occupied, lam, stencil, rs, touch, f, chi, rel_residual (the screened solve's))"""
    G = 2 ** B
    h = side / G
    b = R.rhs_of(R.splat(P, Nw, o, h, G), h)
    chi0, rel0 = RS.first_solve(b, G)
    T = R.iso_of(P, chi0, o, h, G)
    occ = R.occupied(P, o, side, B)
    lam = RS.screen_lambda(alpha, len(P), occ)
    S = RS.stencil_sums(P, o, h, G, lam)
    rs_q, rs = RS.row_sums(S)
    touch = RS.touch_counts(P, o, h, G)                     # a row per touched node, whatever its sums
    M = RS.operator(S, G)
    f = RS.rhs_screened(b, rs, T)
    rhs = f[1:-1, 1:-1, 1:-1].reshape(-1)
    fn = float(np.linalg.norm(rhs))
    x0 = chi0[1:-1, 1:-1, 1:-1].reshape(-1)
    if fn == 0.0:
        x = x0
    elif G < 2 ** RS.CG_FROM_DEPTH:
        from scipy.sparse.linalg import spsolve
        x = spsolve(M, rhs, permc_spec="MMD_AT_PLUS_A")
    else:
        x = RS._cg(-M, rhs, x0)
    rel = float(np.linalg.norm(rhs - M @ x)) / fn if fn > 0.0 else 0.0
    chi = np.zeros_like(b)
    chi[1:-1, 1:-1, 1:-1] = x.reshape(G - 1, G - 1, G - 1)
    ref = dict(depth=B, G=G, h=h, rhs=b, chi0=chi0, rel0=rel0, T=T, occupied=occ, lam=lam, stencil=S, rs=rs, touch=touch,
               f=f, chi=chi, rel_residual=rel, active_nodes=int((touch > 0).sum()), g_norm=float(np.linalg.norm(mean_weights(P, o, h, G))),
               rs_norm=float(np.linalg.norm(rs)))
    return ref


def level_operator(S, cls):
    """rule 40 -> (M_ff csr over the free nodes, A_fc over the fixed ones, free, fixed); asserts rule 38: S has no entry outside the free nodes"""
    import scipy.sparse as sp
    n1 = cls.shape[0]
    flat = cls.reshape(-1)
    free, fixed = np.flatnonzero(flat == RB.FREE), np.flatnonzero(flat == RB.FIXED)
    rows = RB.laplacian_all(n1)[free]
    A_ff, A_fc = rows[:, free], rows[:, fixed]
    assert A_ff.nnz + A_fc.nnz == rows.nnz                  # every neighbour of a free node has a value
    number = np.full(n1 ** 3, -1, np.int64)
    number[free] = np.arange(len(free))
    node, off = np.nonzero(S)
    assert (flat[node] == RB.FREE).all()                    # rule 38: every touched node is FREE
    dz, dy, dx = off // 9 - 1, off // 3 % 3 - 1, off % 3 - 1
    col = node + (dz * n1 + dy) * n1 + dx
    assert (number[col] >= 0).all()
    Sm = sp.csr_matrix((S[node, off].astype(np.float64) * (1.0 / RS.QS), (number[node], number[col])), shape=(len(free), len(free)))
    return (A_ff - Sm).tocsr(), A_fc.tocsr(), free, fixed


def solve_level(P, Nw, o, side, l, band, chi_below, alpha):
    """rules 38-40 for level l -> RB.solve_level's dict (b: rule 28's; chi: the screened field; rel, bnorm: of M_ff chi_f = f') plus
    start, occupied, lam, stencil, rs, touch, T, f, active_nodes, afc_norm, g_norm, rs_norm"""
    from scipy.sparse.linalg import cg
    G = 2 ** l
    h = side / G
    act = RB.active_blocks(P, o, side, l, band)
    cell = RB.cells_of(act)
    cls = RB.node_classes(cell)
    start = RB.start_values(chi_below)
    assert start.shape == cls.shape and not np.isnan(start[cls != RB.NONE]).any()
    b_all = R.rhs_of(R.splat(P, Nw, o, h, G), h)
    occ = R.occupied(P, o, side, l)
    lam = RS.screen_lambda(alpha, len(P), occ)
    S = RS.stencil_sums(P, o, h, G, lam)
    rs_q, rs = RS.row_sums(S)
    T = R.iso_of(P, start, o, h, G)                         # rule 39: on the start values
    M_ff, A_fc, free, fixed = level_operator(S, cls)
    f_all = b_all - T * rs.reshape(b_all.shape)
    fp = f_all.reshape(-1)[free] - A_fc @ start.reshape(-1)[fixed]
    fn = float(np.linalg.norm(fp))
    x = cg(-M_ff, -fp, x0=start.reshape(-1)[free], rtol=1e-14, atol=0.0, maxiter=20000)[0] if fn > 0.0 else np.zeros(len(free))
    rel = float(np.linalg.norm(fp - M_ff @ x)) / fn if fn > 0.0 else 0.0
    chi = np.full(cls.size, np.nan)
    chi[fixed] = start.reshape(-1)[fixed]
    chi[free] = x
    b, f = np.full(cls.size, np.nan), np.full(cls.size, np.nan)
    b[fixed] = f[fixed] = 0.0
    b[free], f[free] = b_all.reshape(-1)[free], f_all.reshape(-1)[free]
    from scipy.sparse.linalg import eigsh
    ritz = float(eigsh(-M_ff, k=1, which="SA", return_eigenvectors=False, tol=1e-4, ncv=64, maxiter=100000, v0=np.ones(M_ff.shape[0]))[0])
    touch = RS.touch_counts(P, o, h, G)
    absA = abs(A_fc)
    afc = math.sqrt(float(absA.sum(0).max()) * float(absA.sum(1).max())) if A_fc.nnz else 0.0
    return dict(l=l, G=G, h=h, act=act, cell=cell, cls=cls, b=b.reshape(cls.shape), chi=chi.reshape(cls.shape), rel=rel, bnorm=fn,
                n_active=int(act.sum()), n_free=len(free), start=np.where(cls != RB.NONE, start, np.nan), occupied=occ, lam=lam, stencil=S, rs=rs,
                touch=touch, T=T, f=f.reshape(cls.shape), active_nodes=int((touch > 0).sum()), afc_norm=afc,
                lmin=max(0.99 * ritz, R.lambda_min(l) - RS.quantisation_norm(touch)),
                g_norm=float(np.linalg.norm(mean_weights(P, o, h, G))), rs_norm=float(np.linalg.norm(rs)))


def reconstruct(points, normals, base_depth=8, band=2, max_gain=4.0, weight=False, density_drop=1, alpha=4.0, **kw):
    """the whole call.  D <= base_depth (rule 36): RS.reconstruct's result at depth D, unchanged.  alpha = 0: RBD.reconstruct's result,
    unchanged.  Otherwise the dict of RBD.reconstruct with base = solve_base's dict and levels = solve_level's dicts, plus alpha"""
    prm = dict(R.DEFAULTS, **kw)
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    assert 3 <= base_depth <= R.MAX_DEPTH and 1 <= band <= 64 and 3 <= prm["depth_min"] <= RB.BAND_MAX_DEPTH and 0.0 <= alpha <= 64.0
    use = R.used_rows(points, normals)
    P, Nn = points[use], normals[use]
    if len(P) < 2 or not (P.max(0) - P.min(0)).max() > 0.0:
        raise R.Degenerate()
    o, side = R.cube_of(P, prm["scale"])
    D = RB.pick_depth(P, o, side, prm)
    if D <= base_depth:
        return RS.reconstruct(points, normals, alpha=alpha, max_gain=max_gain, weight=weight, density_drop=density_drop, **dict(kw, depth_min=D, depth_max=D))
    if alpha == 0.0:
        return RBD.reconstruct(points, normals, base_depth=base_depth, band=band, max_gain=max_gain, weight=weight, density_drop=density_drop, **kw)
    Dd, Gd, hd = RD.density_grid(side, D, density_drop)
    Sd = RD.density_sums(P, o, hd, Gd)
    rho = RD.density_at(P, Sd, o, hd, Gd)
    rho_mean = RD.mean_density(rho)
    s, n_clamped = RD.gains(rho, rho_mean, max_gain)
    Nw = Nn * s[:, None] if weight else Nn                  # rule 36: the flag keeps rule 33's meaning and changes no lambda
    base = solve_base(P, Nw, o, side, base_depth, alpha)
    levels, chi = {}, base["chi"]
    for l in range(base_depth + 1, D + 1):
        levels[l] = solve_level(P, Nw, o, side, l, band, chi, alpha)
        chi = levels[l]["chi"]
    top = levels[D]
    iso = R.iso_of(P, top["chi"], o, top["h"], top["G"])
    verts, faces, gap, n_open, open_vertex = RB.extract(top["chi"], iso, o, top["h"], top["G"], top["cell"])
    dv = RD.density_at(verts, Sd, o, hd, Gd) if len(verts) else np.zeros(0)
    return dict(n_used=len(P), origin=o, side=side, h=top["h"], depth=D, G=top["G"], base_depth=base_depth, base=base, levels=levels, chi=top["chi"],
                iso=iso, vertices=verts, faces=faces, gap=gap, n_open_edges=n_open, open_vertex=open_vertex, P=P, density_depth=Dd, Gd=Gd, hd=hd,
                node_sums=Sd, rho=rho, rho_mean=rho_mean, gain=s, n_clamped=n_clamped, vertex_density=dv, alpha=alpha)


# ------------------------------------------------------------------ what the tests measure ----
def accumulated_bound(ref, rel0, rel_base, rel_of, upto=None):
    """E of the chain (the module's docstring) up to level `upto` (the finest by default): what stopping the two solves of the base at
    the relative residuals rel0 and rel_base and the solve of level l at rel_of(l) can move any chi value of that level, its T and
    its f' entries' solution, and iso, by.  -> (E, {l: (es, E_l)})"""
    base = ref["base"]
    e0 = R.stop_bound(rel0, base["rhs"], base["depth"])
    E = (rel_base * float(np.linalg.norm(base["f"])) + base["g_norm"] * base["rs_norm"] * e0) / (R.lambda_min(base["depth"]) - RS.quantisation_norm(base["touch"]))
    steps = {}
    for l in sorted(ref["levels"]):
        if upto is not None and l > upto:
            break
        lv = ref["levels"][l]
        es = math.sqrt(8.0) / 8.0 * E
        E = max(es, (rel_of(l) * lv["bnorm"] + (lv["g_norm"] * lv["rs_norm"] + lv["afc_norm"]) * es) / lv["lmin"])
        steps[l] = (es, E)
    return E, steps


def target_bound(lv, es):
    """what start values off by es (2-norm) can move T_l by"""
    return lv["g_norm"] * es


def f_bound(lv, es):
    """... and any entry of f = b - T_l rs"""
    return lv["g_norm"] * es * float(np.abs(lv["rs"]).max())
