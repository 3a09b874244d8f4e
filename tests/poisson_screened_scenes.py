"""Small seeded scenes for mvs_poisson_reconstruct_screened (rules 19-23 of include/mvs.h): `uneven`, `seam`, `uniform` and `open` of
tests/poisson_density_scenes.py at D = 5, and one scene each for D = 3, D = 4, D = 4 with alpha = 64, D = 4 with
MVS_POISSON_WEIGHT_NORMALS, and D = 6 — the smallest depth at which the launched kernels of the large levels run, not only the one
workgroup of the coarse levels.  The reference of a scene (tests/ref_poisson_screened.py) is computed once per process and shared by the
tests; nobody changes it.  The seeds were picked on the CPU so that every scene meets the exactness conditions
tests/test_poisson_screened_host.py asserts."""
import functools

import numpy as np

from tests import poisson_density_scenes as DS, ref_poisson_screened as RS

TOL = 1e-12                      # solve_tol of the GPU comparison
ALPHA = 4.0                      # the default of mvs_poisson_screen_params


def _sphere(seed, n):
    return DS._dirs(np.random.default_rng(seed), n)


def _make(name):
    """-> (points, normals, parameter fields, density parameter fields, weight, alpha)"""
    if name in ("uneven", "seam", "uniform", "open"):
        P, N, prm, dprm = DS.scene(name)
        return P, N, prm, dprm, False, ALPHA
    if name == "d3":                                       # D = 3: every level inside the one workgroup, two of them
        d = _sphere(41, 2000)
        return d, d, dict(depth_min=3, depth_max=3, scale=1.6), {}, False, ALPHA
    if name == "d4":
        d = _sphere(42, 6000)
        d = np.concatenate([d[d[:, 2] > 0.0][:2400], d[d[:, 2] <= 0.0][:600]])
        return d, d, dict(depth_min=4, depth_max=4, scale=1.3), {}, False, ALPHA
    if name == "d4_alpha64":                               # the largest alpha the call accepts
        d = _sphere(43, 3000)
        return d, d, dict(depth_min=4, depth_max=4, scale=1.3), {}, False, 64.0
    if name == "d4_weighted":                              # both solves with the weighted normals of rule 16
        d = _sphere(44, 6000)
        d = np.concatenate([d[d[:, 0] > 0.0][:2400], d[d[:, 0] <= 0.0][:600]])
        return d, d, dict(depth_min=4, depth_max=4, scale=1.3), {}, True, ALPHA
    if name == "d6":                                       # 65^3 nodes: level 6 runs the launched smoother, residual, restriction, prolongation
        d = _sphere(45, 6000)
        return d, d, dict(depth_min=6, depth_max=6, scale=1.3), {}, False, ALPHA
    raise KeyError(name)


NAMES = ("uneven", "seam", "uniform", "open", "d3", "d4", "d4_alpha64", "d4_weighted", "d6")
DEPTHS = dict(uneven=5, seam=5, uniform=5, open=5, d3=3, d4=4, d4_alpha64=4, d4_weighted=4, d6=6)


@functools.lru_cache(maxsize=None)
def scene(name):
    P, N, prm, dprm, weight, alpha = _make(name)
    P, N = np.ascontiguousarray(P), np.ascontiguousarray(N)
    P.setflags(write=False)
    N.setflags(write=False)
    return P, N, prm, dprm, weight, alpha


def _freeze(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, alpha=None):
    """the restatement of the scene with its own alpha, or with the given one (0: the unscreened mesh of the same call)"""
    P, N, prm, dprm, weight, a = scene(name)
    return _freeze(RS.reconstruct(P, N, alpha=a if alpha is None else alpha, weight=weight, **dprm, **prm))
