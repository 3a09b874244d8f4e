"""The generated high-valence meshes (tests/mesh_valence.py) are what they claim to be, and the two CPU references agree on them:
only then is a GPU result on them compared with anything (tests/test_gpu_valence.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import mesh_sheets as MS, mesh_valence as MV, ref_numpy


def _edge_weights(oracle, m):
    """the oracle's cotangent weights as a dense-able sparse matrix, and the adjacency of the REAL edges"""
    V = len(m.pts)
    rowptr, col, w = oracle.cot_weights(m.pts, m.faces)
    W = sp.csr_matrix((w, col, rowptr), shape=(V, V))
    return W, MV.adjacency(V, m.faces)


@pytest.mark.parametrize("name", MV.CASES)
def test_case_is_what_it_says(oracle, name):
    m = MV.case(name)
    V = len(m.pts)
    assert oracle.mesh_check(V, m.faces) == 0
    assert V <= 6000 and (V >= 2048) == (not name.startswith("small_"))
    deg = MV.degrees(V, m.faces)
    base = name.partition("_")[0] if not name.startswith("small_") else "small_d12"
    want_max = {"d9": 9, "d12": 12, "d13": 13, "d16": 16, "d17": 17, "d40": 40, "small_d12": 12}[base]
    assert deg.max() == want_max == m.max_valence
    assert deg[m.hubs].tolist() == list(m.valences) and len(set(m.hubs.tolist())) == len(m.hubs)
    n_hubs = (4 if base == "small_d12" else 6) + (MV.OPEN_BOUNDARY_HUBS if name.endswith("_open") else 0)
    assert len(m.hubs) == n_hubs
    # every vertex above valence 8 is a hub or the far vertex x of split edges (next to a hub's ring)
    ring2 = MV.within_rings(V, m.faces, 2)
    for i in np.flatnonzero(deg > 8):
        assert i in m.hubs or any(ring2[i, h] for h in m.hubs), i
    assert sum(v > 8 for v in m.valences) <= (deg > 8).sum()
    # hubs at least four rings apart
    near = MV.within_rings(V, m.faces, 3)
    for k, h in enumerate(m.hubs):
        assert all(near[h, g] == 0 for g in m.hubs[k + 1:]), h
    # rows within a group
    assert len(set((m.hubs & 7).tolist())) >= 4
    if name.endswith("_perm"):
        last = V // 8
        assert V % 8 != 0 and sum(h >> 3 == last for h in m.hubs) >= 2                      # hubs in the last, partial row group
        mids = np.flatnonzero(deg == 4)                                                      # the inserted vertices are spread
        assert mids.min() < V // 4 and mids.max() > 3 * V // 4
    else:
        groups = {}
        for h, v in zip(m.hubs, m.valences):
            groups.setdefault(int(h) >> 3, []).append(v)
        assert any(len(set(v)) >= 2 for v in groups.values())                                # two hubs of different valence in a group
        assert any(h & 7 == 7 and len(groups[int(h) >> 3]) == 1 for h in m.hubs)             # a hub in the last row of another
    expect = {"d9": ("patch", 12), "d12": ("patch", 12), "d13": ("patch", 16), "d16": ("patch", 16), "d17": ("cg", 0),
              "d40": ("cg", 0), "small_d12": ("cg", 0)}[base]
    assert m.expect == expect
    bnd = MV.boundary_vertices(m.faces)
    if name.endswith("_open"):
        # boundary edges (opp1 == -1) in rows of more than one pass
        assert sum(h in bnd for h in m.hubs) >= MV.OPEN_BOUNDARY_HUBS and all(deg[h] > 8 for h in m.hubs if h in bnd)
    else:
        assert len(bnd) == 0
    # ---- the oracle's cotangent weights
    W, A = _edge_weights(oracle, m)
    assert (np.asarray(W.sum(1)).ravel() > 0).all()
    Wd, Ad = W.toarray(), A.toarray()
    assert np.array_equal(Wd, Wd.T)
    zi, zj = np.nonzero((Wd == 0) & (Ad > 0))
    zero = {(int(i), int(j)) for i, j in zip(zi, zj) if i < j}
    if name == "d12_obtuse":
        assert zero == {(min(e), max(e)) for e in m.zero_edges} and len(zero) >= 3
        hub = m.zero_edges[0][0]
        row = np.flatnonzero(Ad[hub])                                                         # the hub's row, ascending as the ELL stores it
        assert any(int(np.searchsorted(row, mid)) >= 8 for _, mid in m.zero_edges)            # ... one of them in the second pass
        assert hub in m.hubs and deg[hub] == 12
    else:
        assert not zero and not m.zero_edges
        assert Wd[Ad > 0].min() > 1e-3                                                        # and none near the clamp either


@pytest.mark.parametrize("hubs_in", [True, False])
@pytest.mark.parametrize("name", MV.CASES)
def test_cpu_references_agree(oracle, name, hubs_in):
    """oracle.arap and ref_numpy.arap (scipy sparse LU, LAPACK SVD) on the deformation the GPU tests use: the case is well posed, and
    their disagreement is the number the GPU tolerance is set against (mesh_valence.tolerances)."""
    m = MV.case(name)
    nodes = MV.nodes_of(m, oracle, hubs_in)
    assert np.isin(m.hubs, nodes).all() if hubs_in else not np.isin(m.hubs, nodes).any()
    tg = MV.target_field(m.pts[nodes])
    a = oracle.arap(m.pts, m.faces, nodes, tg, 5, 1e-4)
    b = ref_numpy.arap(m.pts, m.faces, nodes, tg, 5, 1e-4)
    assert a["iters"] == b["iters"]
    e, dv, dr = MV.cpu_disagreement(m, a, b)
    print(f"[measured] {name} hubs_in={hubs_in}: CPU references differ by energy {e:.2e} vertex RMS/extent {dv:.2e} rotation RMS {dr:.2e}")
    be, bv, br = MV.CPU_DISAGREEMENT[(name, hubs_in)]
    assert e <= be and dv <= bv and dr <= br, (e, dv, dr)
    assert MV.tolerances(name, hubs_in) == (MV.E_RTOL, MV.RMS_TOL, MV.RMS_TOL)        # (ten times the disagreement is far below the project figures)


# ---- flat sheets (tests/mesh_sheets.py): every 1-ring covariance has rank 2 ----
@pytest.mark.parametrize("name", MS.CASES)
def test_sheet_is_what_it_says(oracle, name):
    m = MS.case(name)
    V = len(m.pts)
    size = name.split("_")[0]
    assert oracle.mesh_check(V, m.faces) == 0
    assert (V >= 2048) == (size == "large") and V <= 2300
    deg = MV.degrees(V, m.faces)
    assert deg.max() == 8 and len(MV.boundary_vertices(m.faces)) == 2 * sum(MS.SIZES[size]) - 4
    assert np.array_equal(m.nodes, np.arange(0, V, 13)) and len(m.nodes) >= 3
    off = m.pts @ m.n
    if name.endswith("_flat"):
        assert (m.pts[:, 2] == 0).all() and (m.targets[:, 2] == 0).all() and np.array_equal(m.n, [0, 0, 1])
    else:
        assert np.abs(off).max() <= 1e-15 and (off != 0).any() and np.abs(m.n).min() > 0.05      # off the plane by rounding only
    assert np.abs(m.targets @ m.n).max() <= 1e-15                                                 # the deformation stays in the plane
    W, A = _edge_weights(oracle, m)
    Wd, Ad = W.toarray(), A.toarray()
    assert (np.asarray(W.sum(1)).ravel() > 0.5).all() and (Wd >= 0).all()
    zero = int(((Wd == 0) & (Ad > 0)).sum())
    print(f"[measured] {name}: {zero} of {int(Ad.sum())} real edge weights are exactly 0.0")
    assert zero == MS.ZERO_WEIGHT_EDGES[size] and zero > Ad.sum() // 20                            # the kernels' padding sentinel


@pytest.mark.parametrize("name", MS.CASES)
def test_cpu_references_agree_on_sheets(oracle, name):
    """as test_cpu_references_agree; and the oracle's own rotations keep the plane's normal: the case is well posed"""
    m = MS.case(name)
    a = oracle.arap(m.pts, m.faces, m.nodes, m.targets, 5, 1e-4)
    b = ref_numpy.arap(m.pts, m.faces, m.nodes, m.targets, 5, 1e-4)
    assert a["iters"] == b["iters"] == 5
    e, dv, dr = MV.cpu_disagreement(m, a, b)
    rn = float(np.abs(a["rot"] @ m.n - m.n).max())
    print(f"[measured] {name}: CPU references differ by energy {e:.2e} vertex RMS/extent {dv:.2e} rotation RMS {dr:.2e}; oracle |R n - n| {rn:.2e}")
    be, bv, br = MS.CPU_DISAGREEMENT[name]
    assert e <= be and dv <= bv and dr <= br, (e, dv, dr)
    assert rn <= 1e-12
    assert (max(MV.E_RTOL, 10 * be), max(MV.RMS_TOL, 10 * bv), max(MV.RMS_TOL, 10 * br)) == (MV.E_RTOL, MV.RMS_TOL, MV.RMS_TOL)
