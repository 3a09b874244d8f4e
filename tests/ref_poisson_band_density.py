"""numpy / scipy restatement of rules 32-35 of include/mvs.h (mvs_poisson_reconstruct_band_density): the band levels of
tests/ref_poisson_band.py with the sampling density of tests/ref_poisson_density.py carried over every level.  Composed from those two
and tests/ref_poisson.py without a line of theirs changed, and no code shared with the library: the density grid is one dense array
over all (2^Dd + 1)^3 nodes, whatever the library stores."""
import numpy as np

from tests import ref_poisson as R, ref_poisson_band as RB, ref_poisson_density as RD


def reconstruct(points, normals, base_depth=8, band=2, max_gain=4.0, weight=False, density_drop=1, **kw):
    """the whole call.  D <= base_depth (rule 32): RD.reconstruct's result at depth D, unchanged.  Otherwise the dict of
    RB.reconstruct plus density_depth, Gd, hd, node_sums, rho, rho_mean, gain, n_clamped and vertex_density"""
    prm = dict(R.DEFAULTS, **kw)
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    assert 3 <= base_depth <= R.MAX_DEPTH and 1 <= band <= 64 and 3 <= prm["depth_min"] <= RB.BAND_MAX_DEPTH
    assert 1.0 <= max_gain <= 16.0 and 0 <= density_drop <= 8 and (not weight or len(points) <= 2 ** 22)
    use = R.used_rows(points, normals)
    P, Nn = points[use], normals[use]
    if len(P) < 2 or not (P.max(0) - P.min(0)).max() > 0.0:
        raise R.Degenerate()
    o, side = R.cube_of(P, prm["scale"])
    D = RB.pick_depth(P, o, side, prm)
    if D <= base_depth:
        return RD.reconstruct(points, normals, max_gain=max_gain, weight=weight, density_drop=density_drop, **dict(kw, depth_min=D, depth_max=D))
    # rule 32: rules 14-16 with this D
    Dd, Gd, hd = RD.density_grid(side, D, density_drop)
    S = RD.density_sums(P, o, hd, Gd)
    rho = RD.density_at(P, S, o, hd, Gd)
    rho_mean = RD.mean_density(rho)
    s, n_clamped = RD.gains(rho, rho_mean, max_gain)
    Nw = Nn * s[:, None] if weight else Nn                  # rule 33: x = w * (n_a * s_p), base and band levels alike
    B = base_depth
    G = 2 ** B
    hb = side / G
    rhs_b = R.rhs_of(R.splat(P, Nw, o, hb, G), hb)
    chi_b, rel_b = R.solve(rhs_b, G)
    base = dict(depth=B, G=G, h=hb, rhs=rhs_b, chi=chi_b, rel_residual=rel_b)
    levels, chi = {}, chi_b
    for l in range(B + 1, D + 1):
        levels[l] = RB.solve_level(P, Nw, o, side, l, band, chi)
        chi = levels[l]["chi"]
    top = levels[D]
    iso = R.iso_of(P, top["chi"], o, top["h"], top["G"])    # the unweighted mean over the used points
    verts, faces, gap, n_open, open_vertex = RB.extract(top["chi"], iso, o, top["h"], top["G"], top["cell"])
    dv = RD.density_at(verts, S, o, hd, Gd) if len(verts) else np.zeros(0)      # rule 34
    return dict(n_used=len(P), origin=o, side=side, h=top["h"], depth=D, G=top["G"], base_depth=B, base=base, levels=levels, chi=top["chi"],
                iso=iso, vertices=verts, faces=faces, gap=gap, n_open_edges=n_open, open_vertex=open_vertex, P=P, density_depth=Dd, Gd=Gd,
                hd=hd, node_sums=S, rho=rho, rho_mean=rho_mean, gain=s, n_clamped=n_clamped, vertex_density=dv)


def stored_nodes(P, o, side, Dd):
    """rule 32's storage for Dd > B -> bool [n1, n1, n1]: the nodes of the blocks of level Dd that hold a node of a cell of the block
    of some point (what the library keeps; every other node reads as 0)"""
    Gd = 2 ** Dd
    Gb, n1 = Gd // RB.BLOCK, Gd + 1
    marked = RB.active_blocks(P, o, side, Dd, 0)
    T = Gb + 1                                              # block index Gb holds the node plane Gd only
    stored = np.zeros((T, T, T), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                q = np.zeros((T, T, T), bool)
                q[dz:dz + Gb, dy:dy + Gb, dx:dx + Gb] = marked
                stored |= q
    return stored, stored.repeat(RB.BLOCK, 0).repeat(RB.BLOCK, 1).repeat(RB.BLOCK, 2)[:n1, :n1, :n1]


def corner_sums(X, S, o, hd, Gd):
    """the eight node sums around every row of X [len(X), 8], corner order bx + 2 by + 4 bz"""
    i0, _ = R.corners_weights(X, o, hd, Gd)
    return np.stack([S[RD.node_of(i0, c, Gd + 1)] for c in range(8)], 1)
