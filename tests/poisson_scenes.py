"""Small seeded scenes for mvs_poisson_reconstruct: oriented points with outward normals, and the parameters of the call (scale
must exceed 1 + 4 / 2^depth_min, so the coarse scenes widen their cube).  The reference
of a scene (tests/ref_poisson.py) is computed once per process and shared by the tests; nobody changes it."""
import functools

import numpy as np

from tests import ref_poisson as R

TOL = 1e-12                      # solve_tol of the GPU comparison


def _sphere(rng, n, centre, radius):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.asarray(centre) + radius * d, d


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _make(name):
    if name == "sphere":                                   # off centre, D = 4
        rng = np.random.default_rng(11)
        P, N = _sphere(rng, 500, (0.3, -0.2, 1.7), 1.0)
        return P, N, dict(depth_min=4, depth_max=4, scale=1.3)
    if name == "ellipsoid":                                # rotated, semi-axes 1, 0.7, 0.5: swapped axes show, D = 5
        rng = np.random.default_rng(12)
        d, _ = _sphere(rng, 2001, (0, 0, 0), 1.0)
        ax = np.array([1.0, 0.7, 0.5])
        Rm = _rot(rng)
        n = d / ax
        n /= np.linalg.norm(n, axis=1)[:, None]
        return (d * ax) @ Rm.T + np.array([0.5, 0.25, -0.75]), n @ Rm.T, dict(depth_min=5, depth_max=5, scale=1.2)
    if name == "two_spheres":                              # disjoint: Euler characteristic 4, D = 4
        rng = np.random.default_rng(13)
        P1, N1 = _sphere(rng, 900, (-0.9, 0.0, 0.1), 0.6)
        P2, N2 = _sphere(rng, 900, (0.9, 0.2, -0.1), 0.6)
        return np.concatenate([P1, P2]), np.concatenate([N1, N2]), dict(depth_min=4, depth_max=4, scale=1.3)
    if name == "hemisphere":                               # an open scan; Poisson closes it, D = 3
        rng = np.random.default_rng(14)
        P, N = _sphere(rng, 1200, (0, 0, 0), 1.0)
        keep = P[:, 2] > 0.0
        return P[keep], N[keep], dict(depth_min=3, depth_max=3, scale=1.6)
    if name == "picked":                                   # depth_min 3, depth_max 5: rule 3 picks D = 4
        rng = np.random.default_rng(15)
        P, N = _sphere(rng, 1000, (1.0, 2.0, 3.0), 0.8)
        return P, N, dict(depth_min=3, depth_max=5, scale=1.6)
    raise KeyError(name)


NAMES = ("sphere", "ellipsoid", "two_spheres", "hemisphere", "picked")
DEPTHS = dict(sphere=4, ellipsoid=5, two_spheres=4, hemisphere=3, picked=4)
COMPONENTS = dict(sphere=1, ellipsoid=1, two_spheres=2, hemisphere=1, picked=1)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (points [n, 3], normals [n, 3], parameter fields)"""
    P, N, prm = _make(name)
    P.setflags(write=False)
    N.setflags(write=False)
    return P, N, prm


@functools.lru_cache(maxsize=None)
def reference(name):
    P, N, prm = scene(name)
    return R.reconstruct(P, N, **prm)


def big_sphere(n=60000, seed=21):
    """the scale case: a unit sphere, D = 7"""
    return _sphere(np.random.default_rng(seed), n, (0.1, 0.2, 0.3), 1.0)
