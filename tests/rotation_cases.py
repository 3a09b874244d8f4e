"""3x3 matrices at the edges of the rotation code (svd3_dev.h on the device, orc_geom.cpp in the oracle), a 60-digit reference for
them, and the assertions that hold for ANY correct implementation: only quantities that are unique are compared.

For A = U S V^T (singular values s0 >= s1 >= s2 >= 0) and sigma = sign det(V U^T) the rotation R maximising trace(R A) is
R* = V diag(1, 1, sigma) U^T, the maximum is s0 + s1 + sigma s2, and R* is unique as long as gap = (s1 + sigma s2) / s0 > 0; its
condition number is 1 / gap.  (closest_rotation returns the rotation closest to A^T, which is this R*.)

tests/test_rotation_cases.py holds the CPU oracle to ORACLE_WORST; tests/test_gpu_rotations.py holds the device to ten times that
(mesh_valence.tolerances' convention: the device replaces sqrt and / by Newton-refined hardware estimates).
"""
from __future__ import annotations

import functools
import itertools

import mpmath
import numpy as np

SEED = 20261019
DIGITS = 60
EPS = 2.0 ** -52
GAP_MIN = 1e-9                          # below this the rotation is not compared with R* (it is not unique, or nearly so)
NOT_UNIQUE = ("rank1", "zero", "c*Q reflect")          # the only families allowed below GAP_MIN

# What oracle.closest_rotation showed over every family at SEED (tests/test_rotation_cases.py prints the measurement):
#   orthogonality 1.33e-15 (several families), determinant 1.78e-15, optimality 1.78e-15 and K 6.00 (all `near equal`)
# rounded up; the smallest gap outside NOT_UNIQUE was 1.0e-8 (`graded det<0`).  K: max|R - R*| <= K * 2^-52 / gap.
ORACLE_WORST = dict(orth=1.5e-15, det=2e-15, opt=2e-15, K=7.0)
GPU_FACTOR = 10.0


def bounds(factor=1.0):
    return {k: factor * v for k, v in ORACLE_WORST.items()}


def _rotations(rng, n):
    """n random proper rotations"""
    Q = np.empty((n, 3, 3))
    for k in range(n):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 2] = -q[:, 2]
        Q[k] = q
    return Q


def _conj(Q, d):
    return np.einsum("nij,j,nkj->nik", Q, np.asarray(d, np.float64), Q)


def signed_permutations():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            P = np.zeros((3, 3))
            for j in range(3):
                P[perm[j], j] = signs[j]
            out.append(P)
    return np.array(out)


def _build():
    rng = np.random.default_rng(SEED)
    F = {}
    F["random scaled"] = rng.normal(size=(300, 3, 3)) * 10.0 ** rng.uniform(-12, 12, size=(300, 1, 1))
    F["det<0"] = rng.normal(size=(100, 3, 3)) @ np.diag([1.0, 1.0, -1.0])
    a, b, c, d = (rng.integers(-9, 10, size=(100, 3)).astype(np.float64) for _ in range(4))
    F["rank2 integer"] = np.einsum("ni,nj->nij", a, b) + np.einsum("ni,nj->nij", c, d)
    planar = np.zeros((100, 3, 3))
    planar[:, :2, :2] = rng.normal(size=(100, 2, 2))
    F["rank2 planar"] = planar
    F["rank2 + noise"] = _conj(_rotations(rng, 100), [1.0, 0.3, 0.0]) + 1e-17 * rng.normal(size=(100, 3, 3))
    unit = np.array([np.outer(np.eye(3)[i], np.eye(3)[j]) for i in range(3) for j in range(3)])
    F["rank1"] = np.concatenate([np.einsum("ni,nj->nij", rng.normal(size=(50, 3)), rng.normal(size=(50, 3))), unit])
    F["zero"] = np.zeros((1, 3, 3))
    F["c*Q"] = _rotations(rng, 50) * 10.0 ** rng.uniform(-3, 3, size=(50, 1, 1))
    F["c*Q reflect"] = _rotations(rng, 50) @ np.diag([1.0, 1.0, -1.0])
    F["two equal"] = np.concatenate([_conj(_rotations(rng, 50), [2.0, 1.0, 1.0]), _conj(_rotations(rng, 50), [2.0, 2.0, 1.0])])
    F["near equal"] = _conj(_rotations(rng, 50), [1.0, 1.0 - 1e-8, 1.0 - 2e-8])
    F["signed perm"] = signed_permutations() @ np.diag([3.0, 2.0, 1.0])
    B = rng.normal(size=(100, 3, 5))
    F["sym psd"] = B @ B.transpose(0, 2, 1)
    for name, sign in (("graded", 1.0), ("graded det<0", -1.0)):
        F[name] = np.concatenate([_conj(_rotations(rng, 10), [1.0, 10.0 ** -k, sign * 10.0 ** (-2 * k)]) for k in range(1, 9)])
    F["tiny"] = rng.normal(size=(20, 3, 3)) * 1e-60
    F["huge"] = rng.normal(size=(20, 3, 3)) * 1e60
    for v in F.values():
        v.setflags(write=False)
    return F


_FAMILIES = _build()
FAMILIES = tuple(_FAMILIES)
FINITE_TOTAL = sum(len(v) for v in _FAMILIES.values())


def family(name):
    """(n, 3, 3) float64, read-only"""
    return _FAMILIES[name]


def signed_perm_answer():
    """R* of the `signed perm` family in closed form: A = P diag(3, 2, 1) has U = P, V = I, so R* = diag(1, 1, det P) P^T — exactly
    representable, and what an implementation whose Jacobi sweep finds nothing to rotate must return bit for bit."""
    P = signed_permutations()
    det = np.round(np.linalg.det(P))
    return np.einsum("nj,nkj->njk", np.stack([np.ones(48), np.ones(48), det], axis=1), P)


def _svd_mp(A):
    """U, [s0, s1, s2] descending, V of one double matrix, in mpmath"""
    M = mpmath.matrix(A.tolist())
    if not A.any():
        return mpmath.eye(3), [mpmath.mpf(0)] * 3, mpmath.eye(3)
    U, S, Vt = mpmath.svd_r(M, compute_uv=True)
    order = sorted(range(3), key=lambda j: -S[j])
    U2, V2 = mpmath.matrix(3, 3), mpmath.matrix(3, 3)
    for new, old in enumerate(order):
        for r in range(3):
            U2[r, new] = U[r, old]
            V2[r, new] = Vt[old, r]
    return U2, [S[j] for j in order], V2


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict(Rstar (n,3,3) float64, gap (n,) float64, sigma (n,), s (n,3) float64, opt [mpf], s0 [mpf]) — computed once"""
    A = family(name)
    n = len(A)
    Rstar, gap, sigma, s = np.empty((n, 3, 3)), np.empty(n), np.empty(n), np.empty((n, 3))
    opt, s0 = [], []
    with mpmath.workdps(DIGITS):
        for k in range(n):
            U, S, V = _svd_mp(A[k])
            sg = 1 if mpmath.det(V * U.T) > 0 else -1
            R = V * mpmath.diag([1, 1, sg]) * U.T
            Rstar[k] = np.array([[float(R[i, j]) for j in range(3)] for i in range(3)])
            sigma[k] = sg
            s[k] = [float(x) for x in S]
            gap[k] = float((S[1] + sg * S[2]) / S[0]) if S[0] > 0 else 0.0
            opt.append(S[0] + S[1] + sg * S[2])
            s0.append(S[0])
    for a in (Rstar, gap, sigma, s):
        a.setflags(write=False)
    return dict(Rstar=Rstar, gap=gap, sigma=sigma, s=s, opt=tuple(opt), s0=tuple(s0))


def measure(name, R):
    """the worst orthogonality, determinant, optimality and K of an implementation's rotations R (n,3,3) on a family"""
    A, ref = family(name), reference(name)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    assert R.shape == A.shape and np.isfinite(R).all(), name
    Rl = R.astype(np.longdouble)
    orth = float(np.abs(np.einsum("nki,nkj->nij", Rl, Rl) - np.eye(3)).max())
    det = float(np.abs(Rl[:, 0, 0] * (Rl[:, 1, 1] * Rl[:, 2, 2] - Rl[:, 1, 2] * Rl[:, 2, 1])
                       - Rl[:, 0, 1] * (Rl[:, 1, 0] * Rl[:, 2, 2] - Rl[:, 1, 2] * Rl[:, 2, 0])
                       + Rl[:, 0, 2] * (Rl[:, 1, 0] * Rl[:, 2, 1] - Rl[:, 1, 1] * Rl[:, 2, 0]) - 1).max())
    opt = 0.0
    with mpmath.workdps(DIGITS):
        for k in range(len(A)):
            if ref["s0"][k] == 0:
                continue
            tr = mpmath.fsum(mpmath.mpf(float(R[k, i, j])) * mpmath.mpf(float(A[k, j, i])) for i in range(3) for j in range(3))
            opt = max(opt, abs(float((ref["opt"][k] - tr) / ref["s0"][k])))
    unique = ref["gap"] >= GAP_MIN
    K = 0.0
    if unique.any():
        dist = np.abs(R - ref["Rstar"]).reshape(len(A), 9).max(1)
        K = float((dist[unique] * ref["gap"][unique] / EPS).max())
    return dict(orth=orth, det=det, opt=opt, K=K, min_gap=float(ref["gap"].min()), compared=int(unique.sum()))


def check(name, R, bound, label=""):
    """measure(), print beside the bounds, assert; exact answers where they exist.  -> the measurement"""
    m = measure(name, R)
    print(f"[measured] {label}{name}: orthogonality {m['orth']:.2e} (bound {bound['orth']:.1e}) determinant {m['det']:.2e} "
          f"(bound {bound['det']:.1e}) optimality {m['opt']:.2e} (bound {bound['opt']:.1e}) K {m['K']:.2f} (bound {bound['K']:.1f}) "
          f"on {m['compared']}/{len(family(name))} with gap >= {GAP_MIN:.0e}, smallest gap {m['min_gap']:.1e}")
    if name not in NOT_UNIQUE:
        assert m["compared"] == len(family(name)), (name, m)
    assert m["orth"] <= bound["orth"] and m["det"] <= bound["det"], (name, m)
    assert m["opt"] <= bound["opt"], (name, m)
    assert m["K"] <= bound["K"], (name, m)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    if name == "zero":
        assert np.array_equal(R[0], np.eye(3))
    if name == "signed perm":
        assert np.abs(reference(name)["Rstar"] - signed_perm_answer()).max() <= 1e-50
        assert np.array_equal(R, signed_perm_answer())
    return m
