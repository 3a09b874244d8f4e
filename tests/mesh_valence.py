"""Generated meshes with vertices of valence 9 and above (tests/test_valence_meshes.py checks the builder on the CPU,
tests/test_gpu_valence.py runs the deformation solvers on them).

Every mesh the rest of the suite solves on has valence <= 8: one pass of the ELL-8 adjacency, patch tables of width 6 or 8.
Here a geodesic sphere, stretched and perturbed as ``tests.util.body_scene`` does it (no symmetry, nothing on a tie), gets
HUBS: chosen vertices whose valence is raised by splitting the edges of their ring.  Splitting the ring edge (a, b) of hub v
— opposite vertices v and x — inserts the midpoint m, pushed onto the surface, and replaces (a, b, v), (b, a, x) by (a, m, v), (m, b, v),
(b, m, x), (m, a, x): deg v and deg x rise by one, deg m = 4, the orientation stays.  The longest ring edge is split until the
hub has its valence; new vertices are appended, so a hub keeps its index.

Where the midpoint goes: onto the arc about v through the ends of the ORIGINAL ring edge (_Builder.arc), not onto its chord.  The
middle of the chord of a near-isoceles triangle is the foot of the hub's altitude: split there, the two angles opposite the spoke
(v, a) are 90 degrees to rounding, the spoke's weight is 0 or 1e-17 by chance, and any vertex between a and that foot makes them
obtuse — both cotangents clamped, a real edge of weight exactly 0.  On the arc the fan triangles of v are near-isoceles with
their apex at v: every spoke keeps a clearly positive weight.  Zero-weight real edges are left to the one case made for them.

Nothing is read from or written to disk: a case is built (in well under a second) when it is first asked for.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from multiviewstitch_amd import scene as S

STRETCH = np.array([0.85, 1.0, 1.2])     # mild: no triangle of the base mesh turns obtuse on both sides of an edge
_MIX = np.array([[1.3, 0.7, -0.4], [-0.9, 1.1, 0.5], [0.3, -0.6, 1.7]])

# case -> (sphere frequency, valence of every hub).  Hubs 0 and 1 share a row group of the ELL-8 adjacency (i >> 3) and differ
# in valence; hub 2 is the last row (i & 7 == 7) of another group; the others add further rows within a group.  The valences of
# d12 / d16 are chosen so that V is no multiple of 8: the permuted variants need a last, PARTIAL row group to put hubs into.
_SPEC = {
    "d9": (16, (9, 8, 9, 9, 9, 9)),
    "d12": (16, (12, 9, 12, 10, 11, 9)),
    "d13": (16, (13, 9, 13, 12, 10, 13)),
    "d16": (16, (16, 12, 16, 9, 13, 14)),
    "d17": (16, (17, 16, 17, 12, 9, 13)),
    "d40": (16, (40, 17, 24, 33, 9, 12)),
    "small_d12": (8, (12, 9, 12, 10)),
    "halves_d12": (22, (12, 9, 12, 10, 11, 9)),      # for two parts of >= 2048 vertices: only the hubs well inside y > 0 are raised
}
OPEN_BOUNDARY_HUBS = 2          # the open variants: this many hubs (of the case's maximum valence) ON the boundary, ahead of the others
CASES = ("d9", "d12", "d13", "d16", "d17", "d40", "small_d12", "d12_open", "d16_open", "d12_perm", "d16_perm", "d12_obtuse")
OBTUSE_EDGES = 4                # d12_obtuse: the last four midpoints of hub 2 are moved (row positions 8..11 of the hub)


@dataclasses.dataclass(frozen=True)
class ValenceMesh:
    name: str
    pts: np.ndarray             # (V, 3)
    normals: np.ndarray         # (V, 3)
    faces: np.ndarray           # (F, 3) int32
    hubs: np.ndarray            # vertex indices of the raised vertices
    valences: tuple             # ... and the valence each was raised to
    max_valence: int
    zero_edges: tuple           # (hub, midpoint) pairs built to have BOTH cotangents clamped (d12_obtuse), else ()

    @property
    def extent(self):
        return float(np.abs(self.pts).max())

    @property
    def expect(self):
        """what MVS_SOLVER_AUTO must choose: ("patch", width) or ("cg", 0)"""
        d = self.max_valence
        if len(self.pts) < 2048 or d > 16:
            return "cg", 0
        return "patch", 6 if d <= 6 else 8 if d <= 8 else 12 if d <= 12 else 16


def surface(dirs):
    """the smooth surface the vertices lie on, by direction: anisotropic stretch + a small perturbation"""
    p = np.asarray(dirs) * STRETCH
    return p + 0.02 * np.sin(p @ _MIX + [0.1, 0.5, 0.9])


def degrees(V, faces):
    return np.asarray(adjacency(V, faces).sum(1)).ravel().astype(np.int64)


def adjacency(V, faces):
    f = np.asarray(faces)
    r = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    c = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    A = sp.csr_matrix((np.ones(len(r), np.int8), (r, c)), shape=(V, V))
    A.data[:] = 1
    return A


def within_rings(V, faces, k):
    """boolean sparse matrix: j is at most k rings from i"""
    B = (adjacency(V, faces) + sp.identity(V, dtype=np.int8, format="csr")).astype(np.int32)
    M = B
    for _ in range(k - 1):
        M = M @ B
        M.data[:] = 1
    return M.tocsr()


def boundary_vertices(faces):
    f = np.asarray(faces, np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = int(f.max()) + 1
    key, twin = a * n + b, b * n + a
    lone = ~np.isin(key, twin)
    return np.unique(np.concatenate([a[lone], b[lone]]))


def _pick_hubs(V, faces, n_hubs, first=()):
    """Hubs at least four rings apart.  After ``first``: the lowest row group with two vertices far enough apart gives hubs 0 and 1,
    the lowest vertex with i & 7 == 7 of another group hub 2; the rest are taken from the middle of the index range upwards, each
    with a row i & 7 no hub has yet."""
    near = within_rings(V, faces, 3)
    hubs = list(first)

    def far(i):
        return all(near[i, h] == 0 for h in hubs)

    pair = None
    for g in range(V // 8):
        rows = [i for i in range(8 * g, 8 * g + 8) if far(i)]
        pair = next(((i, j) for i in rows for j in rows if i < j and near[i, j] == 0), None)
        if pair:
            break
    hubs += list(pair)
    hubs.append(next(i for i in range(7, V, 8) if i >> 3 != pair[0] >> 3 and far(i)))
    n_first = len(first)
    i = V // 2
    while len(hubs) - n_first < n_hubs:
        if far(i) and (i & 7) not in {h & 7 for h in hubs[n_first:]}:
            hubs.append(i)
        i += 1
    return hubs


class _Builder:
    def __init__(self, dirs, faces):
        self.dirs = [np.asarray(d, np.float64) for d in dirs]
        self.faces = [tuple(int(x) for x in f) for f in faces]
        self.par = {}                                        # inserted vertex -> (a0, b0, x0, s): see arc()
        self.mids = {}                                       # hub -> [(midpoint, a, b, x)] in the order of the splits

    def arc(self, v, a0, b0, x0, s):
        """the point at parameter s of the arc about v from a0 to b0: the point of the chord, moved towards x0 until it is as far
        from v as the ends are (by direction)"""
        dv, da, db, dx = (self.dirs[q] for q in (v, a0, b0, x0))
        chord = (1 - s) * da + s * db
        chord /= np.linalg.norm(chord)
        want = (1 - s) * np.linalg.norm(da - dv) + s * np.linalg.norm(db - dv)
        lo, hi = 0.0, 0.6
        for _ in range(60):
            t = 0.5 * (lo + hi)
            d = (1 - t) * chord + t * dx
            d /= np.linalg.norm(d)
            lo, hi = (t, hi) if np.linalg.norm(d - dv) < want else (lo, t)
        return d

    def pos(self, i):
        return surface(self.dirs[i])

    def ring(self, v):
        """[(face row, a, b)]: the faces (v, a, b) of v, rotated so that v comes first"""
        out = []
        for r, f in enumerate(self.faces):
            if v in f:
                k = f.index(v)
                out.append((r, f[(k + 1) % 3], f[(k + 2) % 3]))
        return out

    def degree(self, v):
        return len({j for _, a, b in self.ring(v) for j in (a, b)})

    def split_longest(self, v):
        twin = {}
        for r, f in enumerate(self.faces):
            for k in range(3):
                twin[(f[k], f[(k + 1) % 3])] = (r, f[(k + 2) % 3])
        best = None
        for r, a, b in self.ring(v):
            if (b, a) not in twin:                           # a ring edge on the boundary has no second face to split
                continue
            x = twin[(b, a)][1]
            if (x, a) not in twin or (b, x) not in twin:     # (b, a, x) lies on the boundary: its halves would face the boundary edge with
                continue                                     # an obtuse angle at m, the edge's one cotangent clamped
            key = (-float(np.linalg.norm(self.pos(a) - self.pos(b))), a, b)
            if best is None or key < best[0]:
                best = (key, r, a, b)
        _, r1, a, b = best
        r2, x = twin[(b, a)]
        m = len(self.dirs)
        # the original ring edge (a0, b0) this edge is a piece of, and where on it the new vertex lies
        a0, b0, x0, _ = self.par.get(a) or self.par.get(b) or (a, b, x, 0.0)
        s = 0.5 * sum(self.par[q][3] if q in self.par else float(q == b0) for q in (a, b))
        self.par[m] = (a0, b0, x0, s)
        self.dirs.append(self.arc(v, a0, b0, x0, s))
        self.faces[r1] = (a, m, v)
        self.faces[r2] = (b, m, x)
        self.faces += [(m, b, v), (m, a, x)]
        self.mids.setdefault(v, []).append((m, a, b, x))

    def raise_to(self, v, valence):
        while self.degree(v) < valence:
            self.split_longest(v)
        assert self.degree(v) == valence, (v, self.degree(v), valence)


def _cot(p, i, j, o):
    u, v = p[i] - p[o], p[j] - p[o]
    return float(u @ v) / float(np.linalg.norm(np.cross(u, v)))


def _open(dirs, faces):
    """remove a cap of faces (all three vertices inside a cone about an oblique axis), keep the largest component, renumber"""
    c = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    inside = dirs @ c > 0.93
    f = faces[~inside[faces].all(1)]
    pts = surface(dirs)
    while True:                                              # no boundary edge may face an obtuse angle: its one cotangent would be clamped
        a, b, o = (np.concatenate([f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]]) for k in range(3))
        n = len(dirs)
        lone = ~np.isin(a.astype(np.int64) * n + b, b.astype(np.int64) * n + a)
        bad = [r % len(f) for r in np.flatnonzero(lone) if _cot(pts, a[r], b[r], o[r]) < 0.1]
        if not bad:
            break
        f = np.delete(f, bad, axis=0)
    A = adjacency(len(dirs), f)
    _, comp = connected_components(A, directed=False)
    used = np.zeros(len(dirs), bool)
    used[np.unique(f)] = True
    big = np.argmax(np.bincount(comp[used]))
    f = f[comp[f[:, 0]] == big]
    vid = np.unique(f)
    return dirs[vid], np.searchsorted(vid, f).astype(np.int32)


def _boundary_hub_ok(dirs, faces, v, valence):
    """raised to ``valence``, do the two boundary edges of v still face an acute angle?  (each has ONE cotangent: clamped, the
    edge would have weight 0)"""
    b = _Builder(dirs, faces)
    b.raise_to(v, valence)
    pts = surface(np.array(b.dirs))
    have = {(f[k], f[(k + 1) % 3]) for f in b.faces for k in range(3)}
    return all(_cot(pts, f[k], f[(k + 1) % 3], f[(k + 2) % 3]) > 0.1
               for f in b.faces if v in f for k in range(3) if (f[(k + 1) % 3], f[k]) not in have)


@functools.lru_cache(maxsize=None)
def case(name: str) -> ValenceMesh:
    base, _, variant = name.partition("_") if not name.startswith(("small_", "halves_")) else (name, "", "")
    n, valences = _SPEC[base]
    dirs, faces = S.geodesic_sphere(n)
    first = []
    if variant == "open":
        dirs, faces = _open(dirs, faces)
        near = within_rings(len(dirs), faces, 3)
        for i in boundary_vertices(faces):                   # boundary hubs: multi-pass rows with opp1 == -1 entries
            if len(first) < OPEN_BOUNDARY_HUBS and all(near[i, h] == 0 for h in first) and _boundary_hub_ok(dirs, faces, int(i), max(valences)):
                first.append(int(i))
        valences = (max(valences),) * len(first) + valences
    hubs = _pick_hubs(len(dirs), faces, len(valences) - len(first), first)
    if base == "halves_d12":
        keep = [k for k, h in enumerate(hubs) if surface(dirs[h])[1] > 0.15]
        hubs, valences = [hubs[k] for k in keep], tuple(valences[k] for k in keep)
    b = _Builder(dirs, faces)
    for h, val in zip(hubs, valences):
        b.raise_to(h, val)
    dirs = np.array(b.dirs)
    faces = np.array(b.faces, np.int32)
    pts = surface(dirs)
    hubs = np.array(hubs, np.int64)
    zero_edges = ()
    if variant == "obtuse":
        # hub v, midpoint m of (a, b), x beyond: m moves towards x until the angles at a (face a, m, v) and at b (face m, b, v)
        # are clearly obtuse: both cotangents of the real edge (v, m) are clamped, its weight is exactly 0.0
        v = int(hubs[2])                                     # (a vertex of valence 6: its six midpoints are row positions 6..11)
        zero_edges = []
        for m, a, bb, x in b.mids[v][-OBTUSE_EDGES:]:
            mid = dirs[a] + dirs[bb]
            mid /= np.linalg.norm(mid)
            for t in np.arange(0.2, 0.65, 0.05):
                d = (1 - t) * mid + t * dirs[x]
                pts[m] = surface(d / np.linalg.norm(d))
                if _cot(pts, m, v, a) < -0.05 and _cot(pts, m, v, bb) < -0.05:
                    break
            else:
                raise AssertionError("no obtuse placement found")
            zero_edges.append((v, m))
        zero_edges = tuple(zero_edges)
    if variant == "perm":
        # a random vertex order spreads the inserted vertices over the rows; then two hubs are put into the last, partial row group
        V = len(pts)
        assert V % 8 >= 2, V
        new_of_old = np.random.default_rng(12).permutation(V)
        for h, slot in ((hubs[0], V - 1), (hubs[3], V - V % 8)):
            other = int(np.flatnonzero(new_of_old == slot)[0])
            new_of_old[other], new_of_old[h] = new_of_old[h], slot
        old_of_new = np.argsort(new_of_old)
        pts, faces, hubs = pts[old_of_new], new_of_old[faces].astype(np.int32), new_of_old[hubs]
    normals = S.vertex_normals_plyobj(pts, faces)
    deg = degrees(len(pts), faces)
    for a in (pts, normals, faces, hubs):
        a.setflags(write=False)
    return ValenceMesh(name, pts, normals, faces, hubs, tuple(valences), int(deg.max()), zero_edges)


def nodes_of(mesh: ValenceMesh, oracle, hubs_in: bool):
    """uniform_sampling(16) with every hub forced into the node set (its row is a Dirichlet row) or out of it (a free row)"""
    nodes = oracle.uniform_sampling(mesh.pts, 16)
    nodes = np.union1d(nodes, mesh.hubs) if hubs_in else np.setdiff1d(nodes, mesh.hubs)
    return nodes.astype(np.int32)


def target_field(p):
    """a smooth non-rigid target field for node positions ``p`` (as test_arap_on_an_open_irregular_mesh)"""
    A = np.eye(3) + 0.05 * np.random.default_rng(9).normal(size=(3, 3))
    return p @ A.T + 0.02 * np.sin(4 * p)


# Project figures (test_arap_matches_oracle_and_known_answers, test_arap_on_an_open_irregular_mesh): energies rtol 1e-6, vertex and
# rotation RMS 1e-7 x extent at cg_tol 1e-10.  A case whose two CPU references (oracle.arap: the C++ restatement, Jacobi SVD;
# ref_numpy.arap: SuperLU + LAPACK SVD) disagree by more than a tenth of a figure gets ten times their disagreement instead
# (profiles/r08/valence_tests.md holds the measurements; test_valence_meshes.py asserts that they still hold).
E_RTOL, RMS_TOL = 1e-6, 1e-7
# (case, hubs_in) -> (energy rel., vertex RMS / extent, rotation RMS) the CPU references were measured to differ by, rounded up
_BOUND = (5e-14, 2e-14, 5e-13)           # every case and both node sets measured below this (largest: 1.7e-14, 5.8e-15, 1.1e-13)
CPU_DISAGREEMENT = {(c, h): _BOUND for c in CASES for h in (True, False)}


def cpu_disagreement(mesh: ValenceMesh, a: dict, b: dict):
    it = a["iters"]
    e = float((np.abs(a["energies"][:it] - b["energies"][:it]) / np.abs(b["energies"][:it])).max())
    dv = float(np.sqrt(np.mean(np.sum((a["pts"] - b["pts"]) ** 2, axis=1)))) / mesh.extent
    dr = float(np.sqrt(np.mean(np.sum((a["rot"].reshape(-1, 9) - b["rot"].reshape(-1, 9)) ** 2, axis=1))))
    return e, dv, dr


def tolerances(name: str, hubs_in: bool):
    """-> (energy rtol, vertex RMS bound / extent, rotation RMS bound)"""
    e, dv, dr = CPU_DISAGREEMENT.get((name, hubs_in), (0.0, 0.0, 0.0))
    return max(E_RTOL, 10 * e), max(RMS_TOL, 10 * dv), max(RMS_TOL, 10 * dr)
