"""The SRT fit (srt.hip) at its edges, through the C-ABI: match counts around the 64-lane and 256-thread strides of its sums, the
residual's own consistency, the pick rule, poisoned matches, the wrapping integer pixel distance, the branch of k_srt_pick that no
finite hypothesis reaches, and degenerate inputs.  Where the answer is not unique (rank-deficient S, near-ties between hypotheses)
only invariants are asserted; tolerances against the oracle are those of test_gpu_geom.py: s 1e-12, R and t 1e-9.
"""
import functools

import numpy as np
import pytest

from multiviewstitch_amd import scene as S
from tests import rotation_cases as RC

pytestmark = pytest.mark.gpu
SIZES = (3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
N_TRI = 64
CLOSED, RANSAC = 0, 1


@pytest.fixture(scope="module")
def srt():
    from multiviewstitch_amd import _lib, srt
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    return srt


@functools.lru_cache(maxsize=None)
def cams():
    sc = S.make_scene(0)
    return sc.cams[0], sc.cams[1]


def truth():
    ang = 0.4
    return 1.05, np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]), np.array([0.3, -0.1, 0.2])


@functools.lru_cache(maxsize=None)
def problem(n):
    """matches and 64 triples of three distinct indices; triple 40 repeats triple 5, triple 50 is triple 5 in another order"""
    c1, c2 = cams()
    rng = np.random.default_rng(2100 + n)
    m = S.make_matches(rng, c1, c2, *truth(), n=n)
    tri = np.array([rng.choice(n, 3, replace=False) for _ in range(N_TRI)], np.int32)
    tri[40] = tri[5]
    tri[50] = tri[5][[2, 0, 1]]
    assert all(len(set(t.tolist())) == 3 for t in tri)
    m.setflags(write=False)
    tri.setflags(write=False)
    return m, tri


def solver(srt, m):
    sol = srt.SRTSolver(1)
    sol.SetInput(m, *cams())
    return sol


def bits(*a):
    return b"".join(np.ascontiguousarray(x, dtype=np.float64).tobytes() for x in a)


def same_pattern(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and \
        np.array_equal(np.isneginf(a), np.isneginf(b))


def residual_is_its_own(sol, s, R, t, res):
    """the residual mvs_srt_fit hands out is mvs_srt_residual's mean at the returned transform: the wave's lane-by-lane sum and the
    host loop add the same terms in the same order"""
    e = sol.ResidualError(s, R, t)
    return bits(e) == bits(res)


@pytest.mark.parametrize("n", SIZES)
def test_fit_at_stride_edges(srt, oracle, n):
    """the closed form and every hypothesis on its own against the oracle; the residual against itself; the pick rule against the
    device's own hypothesis residuals (between the best and the second best hypothesis lies far less than one pixel flip per match,
    so the device's winner need not be the oracle's)"""
    c1, c2 = cams()
    m, tri = problem(n)
    sol = solver(srt, m)
    # ---- closed form
    s, R, t, res = sol._fit(CLOSED)
    so, Ro, to, _ = oracle.srt_fit(m, c1, c2, 0)
    ds, dR, dt = abs(s - so), float(np.abs(R - Ro).max()), float(np.abs(t - to).max())
    assert ds < 1e-12 and dR < 1e-9 and dt < 1e-9, (ds, dR, dt)
    assert residual_is_its_own(sol, s, R, t, res)
    _, pm = sol.ResidualError(so, Ro, to, per_match=True)
    assert bits(pm) == bits(oracle.srt_residual(m, c1, c2, so, Ro, to)[1])                # integer pixels at the oracle's transform
    # ---- every hypothesis alone
    single, worst = [], [ds, dR, dt]
    for k in range(N_TRI):
        sk, Rk, tk, rk = sol._fit(RANSAC, tri[k:k + 1])
        so, Ro, to, _ = oracle.srt_fit(m, c1, c2, 1, tri[k:k + 1], 1)
        d = (abs(sk - so), float(np.abs(Rk - Ro).max()), float(np.abs(tk - to).max()))
        worst = [max(a, b) for a, b in zip(worst, d)]
        assert d[0] < 1e-12 and d[1] < 1e-9 and d[2] < 1e-9, (k, d)
        single.append((sk, Rk, tk, rk))
    assert residual_is_its_own(sol, *single[7])
    assert bits(*single[40]) == bits(*single[5])
    # ---- the pick: the first index of the strict minimum
    res_k = np.array([x[3] for x in single])
    assert np.isfinite(res_k).all()
    best, arg = np.inf, -1
    for k in range(N_TRI):
        if res_k[k] < best:
            best, arg = res_k[k], k
    assert arg != 40 and (arg != 50 or res_k[50] < res_k[5])
    s, R, t, res = sol._fit(RANSAC, tri)
    assert bits(s, R, t, res) == bits(*single[arg])
    assert residual_is_its_own(sol, s, R, t, res)
    second = np.sort(res_k)[1] - best
    print(f"[measured] n={n}: closed form and {N_TRI} single hypotheses against the oracle: s {worst[0]:.2e} (tol 1e-12) R {worst[1]:.2e} "
          f"t {worst[2]:.2e} (tol 1e-9); winner {arg} residual {best:.6f}, second best {second:.2e} above")
    # the first of two equal minima wins: the winner's triple once more behind it changes nothing
    again = np.concatenate([tri, tri[arg:arg + 1]])
    assert bits(*sol._fit(RANSAC, again)) == bits(s, R, t, res)


# ---- poisoned matches ----
def poisoned():
    """n = 16, and one row spoiled in each way: (name, matches)"""
    c1, c2 = cams()
    m = np.array(S.make_matches(np.random.default_rng(77), c1, c2, *truth(), n=16, outlier_frac=0.0))
    centre1 = -c1.R.T @ c1.t
    out = []
    for name, row, edit in (("p1 x 1e6", 2, lambda r: r.__setitem__(slice(0, 3), r[0:3] * 1e6)),
                            ("p2 negated", 5, lambda r: r.__setitem__(slice(3, 6), -r[3:6])),
                            ("NaN coordinate", 7, lambda r: r.__setitem__(1, np.nan)),
                            ("NaN coordinate of p2", 8, lambda r: r.__setitem__(5, np.nan)),
                            ("p2 inf", 11, lambda r: r.__setitem__(slice(3, 6), np.inf)),
                            ("p1 at camera 1's centre", 13, lambda r: r.__setitem__(slice(0, 3), centre1))):
        p = m.copy()
        edit(p[row])
        out.append((name, row, p))
    allp = m.copy()
    for _, row, p in out:
        allp[row] = p[row]
    out.append(("all of them", -1, allp))
    return m, out


def test_poisoned_matches_give_the_oracles_pixels(srt, oracle):
    """x86 converts NaN, inf and out-of-range to INT_MIN and the squared pixel distance wraps: the oracle returns integer-derived
    values (finite, or NaN under a negative wrapped square) for the spoiled rows, and the device must return the same bits"""
    c1, c2 = cams()
    clean, cases = poisoned()
    so, Ro, to, _ = oracle.srt_fit(clean, c1, c2, 0)
    seen_nan = seen_finite = 0
    for name, row, p in cases:
        ref_e, ref = oracle.srt_residual(p, c1, c2, so, Ro, to)
        e, pm = solver(srt, p).ResidualError(so, Ro, to, per_match=True)
        print(f"[measured] poisoned ({name}): oracle row {ref[row] if row >= 0 else ref[[2, 5, 7, 8, 11, 13]].tolist()} mean {ref_e}")
        assert np.array_equal(np.isnan(pm), np.isnan(ref)), name
        assert bits(pm) == bits(ref), name
        assert bits(e) == bits(ref_e), name
        if row >= 0:
            others = np.arange(16) != row
            assert np.isfinite(ref[others]).all() and (ref[others] < 4).all()
            assert (ref[row] > 20).any() or np.isnan(ref[row]).any(), name               # the spoiled row shows
            seen_nan += int(np.isnan(ref[row]).any())
            seen_finite += int(np.isfinite(ref[row]).any())
    assert seen_finite >= 3                                                              # INT_MIN-derived values that are NOT NaN


# ---- the wrap, and the branch of k_srt_pick that no finite hypothesis reaches ----
@functools.lru_cache(maxsize=None)
def wrapped():
    """One match moved: its p2 goes to depth 0.05 in front of camera 2 and 24 units sideways (fx = 112: about 53 760 pixels from the
    image, as 2400 units would be at depth 5; so close to the camera the move shifts the barycentre b2 by 0.2 units only and the scale
    stays near 1, so that every hypothesis still maps p1 into the image)."""
    c1, c2 = cams()
    n, j = 129, 70
    m, tri = problem(n)
    m = np.array(m)
    q = c2.R @ m[j, 3:6] + c2.t
    m[j, 3:6] = c2.R.T @ (np.array([q[0] + 24.0, q[1], 0.05]) - c2.t)
    m.setflags(write=False)
    return m, tri, j


def test_wrapped_pixel_distance_and_no_finite_hypothesis(srt, oracle):
    from tests import ref_numpy
    c1, c2 = cams()
    m, tri, j = wrapped()

    def px(c, p):
        q = c.R @ p + c.t
        return np.array([c.fx * q[0] / q[2] + c.cx, c.fy * q[1] / q[2] + c.cy])

    # on the CPU: for every hypothesis the match's two projections in camera 2 are 46341 .. 65535 pixels apart, the int32 square is
    # negative, e1 is NaN and so is the hypothesis residual
    so = oracle.srt_fit(m, c1, c2, 0)[0]
    b1, b2 = m[:, 0:3].mean(0), m[:, 3:6].mean(0)
    X, Y = (m[:, 0:3] - b1) * so, m[:, 3:6] - b2
    far = []
    for k in range(N_TRI):
        Rk = ref_numpy.kabsch(X[tri[k]].T @ Y[tri[k]])
        tk = b2 - so * Rk @ b1
        e, pm = oracle.srt_residual(m, c1, c2, so, Rk, tk)
        assert np.isnan(pm[j, 0]) and np.isnan(e), k
        assert np.isfinite(np.delete(pm, j, axis=0)).all()
        d = px(c2, m[j, 3:6]) - px(c2, so * Rk @ m[j, 0:3] + tk)
        far.append(np.hypot(d[0], d[1]))
        # oracle.srt_fit keeps a hypothesis only if its residual is finite: this one is not kept
        _, Ro, to, ro = oracle.srt_fit(m, c1, c2, 1, tri[k:k + 1], 1)
        assert np.array_equal(Ro, np.eye(3)) and np.array_equal(to, np.zeros(3)) and np.isnan(ro)
    assert 46341 < min(far) and max(far) < 65535
    so, Ro, to, ro = oracle.srt_fit(m, c1, c2, 1, tri, N_TRI)
    assert np.array_equal(Ro, np.eye(3)) and np.array_equal(to, np.zeros(3)) and np.isnan(ro) and 0.5 < so < 2
    sol = solver(srt, m)
    s, R, t, res = sol._fit(RANSAC, tri)
    print(f"[measured] wrap: pixel distance {min(far):.0f} .. {max(far):.0f}; scale {s!r} against the oracle's {so!r} (tol 1e-12), "
          f"R = I {np.array_equal(R, np.eye(3))} t = 0 {np.array_equal(t, np.zeros(3))} residual {res}")
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
    assert abs(s - so) < 1e-12
    assert np.isnan(res) and residual_is_its_own(sol, s, R, t, res)
    for k in (0, 31, 63):                                                                 # a single NaN hypothesis as well
        sk, Rk, tk, rk = sol._fit(RANSAC, tri[k:k + 1])
        assert np.array_equal(Rk, np.eye(3)) and np.array_equal(tk, np.zeros(3)) and bits(sk) == bits(s) and np.isnan(rk)
    _, pm = sol.ResidualError(so, Ro, to, per_match=True)
    assert bits(pm) == bits(oracle.srt_residual(m, c1, c2, so, Ro, to)[1])
    # the closed form is not scored: it returns its rotation, and a NaN residual
    s, R, t, res = sol._fit(CLOSED)
    so, Ro, to, ro = oracle.srt_fit(m, c1, c2, 0)
    assert abs(s - so) < 1e-12 and np.abs(R - Ro).max() < 1e-9 and np.abs(t - to).max() < 1e-9 and np.isnan(res) and np.isnan(ro)


# ---- degenerate inputs: invariants only ----
def test_one_match_and_identical_matches(srt, oracle):
    """Every centred vector is 0, the scale 0 / 0, and everything after it NaN.  The coordinates are multiples of 1/64: the sum of five
    equal values and its fifth are then exact in ANY order of summation, so that the barycentre is the point itself for the oracle's
    loop and for the device's tree alike (otherwise a last-bit difference of the barycentres decides between 0 / 0 and x / 0).  A
    NaN transform projects to INT_MIN and the wrapped pixel distance is finite: RANSAC keeps such a hypothesis, as the oracle does."""
    c1, c2 = cams()
    m = np.round(np.array(problem(7)[0]) * 64) / 64
    one = m[:1]
    five = np.repeat(m[3:4], 5, axis=0)
    for name, mm, mode, tri in (("n = 1", one, CLOSED, None), ("five identical", five, CLOSED, None),
                                ("five identical, RANSAC", five, RANSAC, np.array([[0, 1, 2], [4, 2, 0]], np.int32))):
        s, R, t, res = solver(srt, mm)._fit(mode, tri)
        so, Ro, to, ro = oracle.srt_fit(mm, c1, c2, mode, tri, 0 if tri is None else len(tri))
        print(f"[measured] {name}: device s {s} R[0] {R[0]} t {t} residual {res}; oracle s {so} R[0] {Ro[0]} t {to} residual {ro}")
        assert same_pattern([s], [so]) and same_pattern(R, Ro) and same_pattern(t, to), name
        assert np.isnan(so) and np.isnan(Ro).all() and np.isnan(to).all()
        assert bits(res) == bits(ro), name                                                # integer pixels


def test_rank_deficient_fits_keep_their_invariants(srt, oracle):
    """n = 2 (closed form), and triples (i, i, i) and (i, i, j): S has rank <= 1 (<= 2) and the rotation is not unique.  s is the
    oracle's, R is a proper rotation within the bounds of tests/rotation_cases.py, t = b2 - s R b1, the residual is its own."""
    c1, c2 = cams()
    m7, _ = problem(7)
    bound = RC.bounds(RC.GPU_FACTOR)
    cases = [("n = 2", np.array(m7[:2]), CLOSED, None)]
    for tri in ([3, 3, 3], [0, 0, 0], [6, 6, 6], [2, 2, 5], [5, 2, 2], [4, 1, 4]):
        cases.append((f"triple {tri}", np.array(m7), RANSAC, np.array([tri], np.int32)))
    for name, mm, mode, tri in cases:
        sol = solver(srt, mm)
        s, R, t, res = sol._fit(mode, tri)
        so = oracle.srt_fit(mm, c1, c2, mode, tri, 0 if tri is None else 1)[0]
        assert np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(res), name
        Rl = R.astype(np.longdouble)
        orth = float(np.abs(Rl.T @ Rl - np.eye(3)).max())
        det = float(abs(np.linalg.det(R) - 1))
        b1, b2 = mm[:, 0:3].mean(0), mm[:, 3:6].mean(0)
        dt = float(np.abs(t - (b2 - s * (R @ b1))).max())
        print(f"[measured] {name}: |s - oracle| {abs(s - so):.2e} (tol 1e-12) orthogonality {orth:.2e} (bound {bound['orth']:.1e}) "
              f"determinant {det:.2e} (bound {bound['det']:.1e}) |t - (b2 - s R b1)| {dt:.2e} (tol 1e-12)")
        assert abs(s - so) < 1e-12, name
        assert orth <= bound["orth"] and det <= bound["det"], name
        assert dt < 1e-12, name
        assert residual_is_its_own(sol, s, R, t, res), name
