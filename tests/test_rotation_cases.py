"""The CPU oracle's closest_rotation on the edge families of tests/rotation_cases.py, against the 60-digit reference: the oracle
stays within ORACLE_WORST, the figures the device bounds of tests/test_gpu_rotations.py are ten times of."""
import numpy as np
import pytest

from tests import rotation_cases as RC


def test_families_are_what_they_say():
    n = {f: len(RC.family(f)) for f in RC.FAMILIES}
    assert n == {"random scaled": 300, "det<0": 100, "rank2 integer": 100, "rank2 planar": 100, "rank2 + noise": 100, "rank1": 59,
                 "zero": 1, "c*Q": 50, "c*Q reflect": 50, "two equal": 100, "near equal": 50, "signed perm": 48, "sym psd": 100,
                 "graded": 80, "graded det<0": 80, "tiny": 20, "huge": 20}
    assert all(np.isfinite(RC.family(f)).all() for f in RC.FAMILIES)
    s = RC.reference("rank2 integer")["s"]
    assert (s[:, 2] <= 1e-50).all() and (s[:, 1] > 1e-3).all()
    s = RC.reference("rank1")["s"]
    assert (s[:, 1] <= 1e-15 * s[:, 0]).all()                  # (rounded outer products: rank 1 to rounding, below the 1e-14 switch)
    assert (RC.reference("det<0")["sigma"] == -1).mean() > 0.3 and (RC.reference("graded det<0")["sigma"] == -1).all()
    assert (RC.reference("c*Q reflect")["sigma"] == -1).all() and (RC.reference("c*Q reflect")["gap"] < 1e-15).all()
    A = RC.family("signed perm")                               # columns orthogonal, every order of 3, 2, 1 present
    G = np.einsum("nki,nkj->nij", A, A)
    assert (G[:, ~np.eye(3, dtype=bool)] == 0).all()
    assert {tuple(np.diag(g)) for g in G} == {(9.0, 4.0, 1.0)} and len({a.tobytes() for a in A}) == 48
    order = {tuple(np.argmax(np.abs(a), axis=0)) for a in A}
    assert len(order) == 6
    g = RC.reference("graded")["s"]                            # both sides of the s1 > 1e-14 s0 switch of the U completion ...
    assert g[:, 1].min() / g[:, 0].max() > 1e-14 and g[:, 2].min() < 1e-14 < g[:, 2].max()
    assert 1e-61 < np.abs(RC.family("tiny")).max() < 1e-59 and 1e59 < np.abs(RC.family("huge")).max() < 1e61   # the stated scale range


@pytest.mark.parametrize("name", RC.FAMILIES)
def test_oracle_closest_rotation_within_oracle_worst(oracle, name):
    R = np.array([oracle.closest_rotation(a) for a in RC.family(name)])
    RC.check(name, R, RC.bounds(), "oracle ")


def test_a_wrong_rotation_is_caught():
    """the helper itself: the transpose of R*, an improper R*, and R* turned by 1e-13 about an axis all miss the bounds"""
    name = "det<0"
    Rs = RC.reference(name)["Rstar"]
    RC.check(name, Rs, RC.bounds(), "R* ")
    c, s = np.cos(1e-13), np.sin(1e-13)
    turn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    for bad in (Rs.transpose(0, 2, 1), Rs * np.array([1.0, 1.0, -1.0])[None, :, None], turn @ Rs):
        with pytest.raises(AssertionError):
            RC.check(name, bad, RC.bounds(), "wrong ")
