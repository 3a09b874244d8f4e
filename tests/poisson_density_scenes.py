"""Small seeded scenes for mvs_poisson_reconstruct_density (rules 14-18 of include/mvs.h): oriented points on a unit sphere about the
origin whose sampling density is not uniform, the parameters of the call and the density parameters.  The reference of a scene
(tests/ref_poisson_density.py), with and without the weighting of rule 16, is computed once per process and shared by the tests; nobody
changes it.  The seeds were picked on the CPU so that every scene meets the exactness conditions tests/test_poisson_density_host.py
asserts."""
import functools

import numpy as np

from tests import ref_poisson_density as RD

TOL = 1e-12                      # solve_tol of the GPU comparison
TRIM_RATIO = 0.25                # the trim threshold of `open` over its mean point density


def _dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def _make(name):
    if name == "uneven":                                   # one half of the sphere sampled 4 : 1 against the other, D = 5
        rng = np.random.default_rng(31)
        d = _dirs(rng, 16000)
        d = np.concatenate([d[d[:, 0] > 0.0][:6400], d[d[:, 0] <= 0.0][:1600]])
        return d, d, dict(depth_min=5, depth_max=5, scale=1.3), {}
    if name == "seam":                                     # the sphere plus a second copy of a 120 degree lune displaced by 0.4 %, D = 5
        rng = np.random.default_rng(32)
        d = _dirs(rng, 5000)
        e = _dirs(rng, 7500)
        e = e[np.abs(np.arctan2(e[:, 1], e[:, 0])) < np.pi / 3.0]
        return np.concatenate([d, e + np.array([0.004, 0.0, 0.0])]), np.concatenate([d, e]), dict(depth_min=5, depth_max=5, scale=1.3), {}
    if name == "open":                                     # cut at z = -0.2: the solve closes it, the trim opens it again, D = 5
        rng = np.random.default_rng(33)
        d = _dirs(rng, 10000)
        d = d[d[:, 2] > -0.2][:6000]
        return d, d, dict(depth_min=5, depth_max=5, scale=1.3), {}
    if name == "clamped":                                  # a densely sampled sphere whose cap z > 0.8 holds six points only, D = 4
        rng = np.random.default_rng(34)
        d = _dirs(rng, 4000)
        cap = d[:, 2] > 0.8
        d = np.concatenate([d[~cap][:2400], d[cap][:6]])
        return d, d, dict(depth_min=4, depth_max=4, scale=1.3), {}
    if name == "drop_floor":                               # D = 3 with density_drop = 4: Dd sits at its floor of 2
        rng = np.random.default_rng(35)
        d = _dirs(rng, 4000)
        d = np.concatenate([d[d[:, 1] > 0.0][:1600], d[d[:, 1] <= 0.0][:400]])
        return d, d, dict(depth_min=3, depth_max=3, scale=1.6), dict(density_drop=4)
    if name == "drop_zero":                                # density_drop = 0: the density grid is the solve grid, D = 4
        rng = np.random.default_rng(36)
        d = _dirs(rng, 6000)
        d = np.concatenate([d[d[:, 2] > 0.0][:2400], d[d[:, 2] <= 0.0][:600]])
        return d, d, dict(depth_min=4, depth_max=4, scale=1.3), dict(density_drop=0)
    if name == "uniform":                                  # the control of the quality test: weighting must not hurt, D = 5
        d = _dirs(np.random.default_rng(37), 8000)
        return d, d, dict(depth_min=5, depth_max=5, scale=1.3), {}
    raise KeyError(name)


NAMES = ("uneven", "seam", "open", "clamped", "drop_floor", "drop_zero")
DEPTHS = dict(uneven=5, seam=5, open=5, clamped=4, drop_floor=3, drop_zero=4, uniform=5)
DENSITY_DEPTHS = dict(uneven=4, seam=4, open=4, clamped=3, drop_floor=2, drop_zero=4, uniform=4)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (points [n, 3], normals [n, 3], parameter fields, density parameter fields without the flag)"""
    P, N, prm, dprm = _make(name)
    P, N = np.ascontiguousarray(P), np.ascontiguousarray(N)
    P.setflags(write=False)
    N.setflags(write=False)
    return P, N, prm, dprm


@functools.lru_cache(maxsize=None)
def reference(name, weight):
    P, N, prm, dprm = scene(name)
    ref = RD.reconstruct(P, N, weight=bool(weight), **dprm, **prm)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
