"""svd3_dev.h on the device, directly (mvs_test_rotations, include/mvs_test.h): closest_rotation, kabsch_rotation and svd3_dev on
the edge families of tests/rotation_cases.py.  Every ARAP local step and every SRT hypothesis runs this code, and the solves and
fits of the rest of the suite never show it a rank-deficient, reflected, repeated, graded or badly scaled matrix.

Only unique quantities are asserted (rotation_cases.check), at ten times the figures the CPU oracle shows against the 60-digit
reference; equality of bits only between two runs of the same code.

Mutations of svd3_dev.h tried against this file (never committed): the second swap's `<` as `<=` fails `zero` (the tied columns
of V are swapped and the identity is lost); without the det < 0 re-flip of closest_rotation every family with a reflection fails.
Dropping one of the two Newton steps of rsqrt_nr is NOT seen: the worst orthogonality rises from 1.3e-15 to 3.6e-15, the
determinant from 1.4e-15 to 4.0e-15, K from 4.0 to 10.0 — all inside ten times the oracle's figures (1.5e-14, 2e-14, 70).
"""
import numpy as np
import pytest

from tests import rotation_cases as RC

pytestmark = pytest.mark.gpu
BOUND = RC.bounds(RC.GPU_FACTOR)


@pytest.fixture(scope="module")
def rot():
    from multiviewstitch_amd import _lib as L
    if L.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")

    def run(A, rule=0, svd=False, guard=0):
        """-> R (n,3,3) [, U, Vm]; `guard` extra rows behind every output, filled with -7, are returned too"""
        A = L.arr(A, np.float64).reshape(-1, 3, 3)
        n = len(A)
        out = [np.full((n + guard, 3, 3), -7.0) for _ in range(3 if svd else 1)]
        L.check(L.lib().mvs_test_rotations(n, L.ptr(A), rule, *(L.ptr(o) for o in out), *([None, None] if not svd else [])))
        return out if svd else out[0]

    return run


@pytest.mark.parametrize("name", RC.FAMILIES)
def test_closest_rotation_on_every_family(rot, name):
    A = RC.family(name)
    R = rot(A, 0)
    RC.check(name, R, BOUND, "device ")
    # kabsch_rotation differs from closest_rotation only in its reflection test (|det + 1| <= 1e-9 against det < 0) and the
    # determinant of V U^T is +-1 to rounding: the same bits
    assert rot(A, 1).tobytes() == R.tobytes()
    assert rot(A, 0).tobytes() == R.tobytes()                                  # and two identical calls give identical bytes


@pytest.mark.parametrize("name", RC.FAMILIES)
def test_svd_factors_on_every_family(rot, name):
    A = RC.family(name)
    R, U, Vm = rot(A, 0, svd=True)
    assert R.tobytes() == rot(A, 0).tobytes()
    assert np.isfinite(U).all() and np.isfinite(Vm).all()
    eye = np.eye(3)
    ou = float(np.abs(np.einsum("nki,nkj->nij", U, U) - eye).max())
    ov = float(np.abs(np.einsum("nki,nkj->nij", Vm, Vm) - eye).max())
    S = np.einsum("nki,nkl,nlj->nij", U, A, Vm)                                # U^T A Vm
    d = np.einsum("nii->ni", S)
    s0 = np.maximum(RC.reference(name)["s"][:, 0], np.finfo(float).tiny)
    neg = float((-d / s0[:, None]).max())
    asc = float(((d[:, 1:] - d[:, :-1]) / s0[:, None]).max())
    amax = np.maximum(np.abs(A).reshape(len(A), 9).max(1), np.finfo(float).tiny)
    back = np.einsum("nij,nj,nkj->nik", U, d, Vm)
    rec = float((np.abs(back - A).reshape(len(A), 9).max(1) / amax).max())
    print(f"[measured] device {name}: U orthogonality {ou:.2e} V {ov:.2e} (bound {BOUND['orth']:.1e}) -min s/s0 {neg:.2e} "
          f"largest ascent/s0 {asc:.2e} (bound {BOUND['orth']:.1e}) reconstruction/max|A| {rec:.2e} (bound 1e-13)")
    assert ou <= BOUND["orth"] and ov <= BOUND["orth"]
    assert neg <= BOUND["orth"] and asc <= BOUND["orth"]
    assert rec <= 1e-13


def _mixed():
    rng = np.random.default_rng(RC.SEED + 1)
    A = np.concatenate([RC.family(f) for f in ("random scaled", "rank2 planar", "graded det<0", "signed perm")])[:500].copy()
    at = np.sort(rng.choice(len(A), 40, replace=False))
    at[0], at[-1] = 0, len(A) - 1
    at = np.unique(at)
    for k, i in enumerate(at):
        A[i].reshape(9)[k % 9] = np.nan                                        # every position of the matrix in turn
    A[at[3]] = np.nan                                                          # and one matrix of nine NaN
    return A, at


def test_nan_rows_poison_only_themselves(rot):
    """a NaN never passes the convergence test: the sweep runs to its cap of 64 and hands out NaN; the rows beside it are those
    of a call without the NaN rows, bit for bit"""
    A, at = _mixed()
    R = rot(A, 0)
    assert np.isnan(R[at]).all()
    fin = np.setdiff1d(np.arange(len(A)), at)
    assert np.isfinite(R[fin]).all()
    assert R[fin].tobytes() == rot(A[fin], 0).tobytes()
    R1 = rot(A, 1)
    assert np.isnan(R1[at]).all() and R1[fin].tobytes() == R[fin].tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_launch_edges(rot, n):
    A = np.concatenate([RC.family("random scaled"), RC.family("det<0")])[:n]
    whole = rot(np.concatenate([RC.family("random scaled"), RC.family("det<0")])[:257], 0, svd=True)
    out = rot(A, 0, svd=True, guard=1)
    for o, w in zip(out, whole):
        assert o[:n].tobytes() == w[:n].tobytes()
        assert (o[n:] == -7.0).all()                                           # the guard row behind every output


def test_arguments(rot):
    from multiviewstitch_amd import _lib as L
    f = L.lib().mvs_test_rotations
    A, R = np.eye(3).reshape(1, 3, 3).copy(), np.empty((1, 3, 3))
    assert f(1, None, 0, L.ptr(R), None, None) == -1 and f(1, L.ptr(A), 0, None, None, None) == -1
    assert f(-1, L.ptr(A), 0, L.ptr(R), None, None) == -1
    assert f(1, L.ptr(A), 2, L.ptr(R), None, None) == -1 and f(1, L.ptr(A), -1, L.ptr(R), None, None) == -1
    assert f(1, L.ptr(A), 1, L.ptr(R), None, None) == 0 and np.array_equal(R[0], np.eye(3))
