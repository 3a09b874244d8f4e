"""Scenes for the band levels of the Poisson stage (rules 24-31): oriented points, the parameters of the plain call and base_depth / band.  The restatement
of a scene (tests/ref_poisson_band.py) is computed once per process and shared by the tests; nobody changes it.  Every scene of
PARITY must leave blocks inactive at every band level and have free nodes beside fixed ones in all six directions
(tests/test_poisson_band_host.py holds them to that; level 4 of `hemisphere`, 4^3 blocks, is the one exception it names)."""
import functools

import numpy as np

from tests import poisson_scenes as SC, ref_poisson_band as RB

TOL = SC.TOL


def _sphere6k():
    return SC._sphere(np.random.default_rng(31), 6000, (0.1, 0.2, 0.3), 1.0)


def _make(name):
    if name == "at_base":                                  # D = 4 = base_depth: the plain call
        P, N, prm = SC.scene("sphere")
        return P, N, dict(prm), dict(base_depth=4, band=2)
    if name == "all_active":                               # one band level, every block of it active
        P, N = _sphere6k()
        return P, N, dict(depth_min=5, depth_max=5, scale=1.3), dict(base_depth=4, band=8)
    if name == "two_levels":                               # an inactive core and inactive corners on both levels
        P, N = _sphere6k()
        return P, N, dict(depth_min=6, depth_max=6, scale=1.3), dict(base_depth=4, band=1)
    if name == "two_spheres":                              # two bands with inactive blocks between them: the gap is five blocks of level 6
        rng = np.random.default_rng(33)
        P1, N1 = SC._sphere(rng, 900, (-1.1, 0.0, 0.1), 0.45)
        P2, N2 = SC._sphere(rng, 900, (1.1, 0.2, -0.1), 0.45)
        return np.concatenate([P1, P2]), np.concatenate([N1, N2]), dict(depth_min=6, depth_max=6, scale=1.3), dict(base_depth=4, band=1)
    if name == "clipped":                                  # scale just above 1 + 4 / 2^6: the band reaches the boundary of the grid
        P, N = _sphere6k()
        return P, N, dict(depth_min=6, depth_max=6, scale=1.07), dict(base_depth=5, band=2)   # from base 4, level 5 would be all active
    if name == "hemisphere":                               # an open scan that stays closed: the low points of the dome keep the blocks
                                                           # under it active (level 4 is 4^3 blocks, all of them active)
        P, N, prm = SC.scene("hemisphere")
        return P, N, dict(prm, depth_min=5, depth_max=5), dict(base_depth=3, band=1)
    if name == "cap":                                      # the cap z > 0.5 of a sphere: the base solve closes it half a radius from
        P, N = SC._sphere(np.random.default_rng(32), 3000, (0, 0, 0), 1.0)   # every sample, where level 6 has no block: open edges
        keep = P[:, 2] > 0.5
        return P[keep], N[keep], dict(depth_min=6, depth_max=6, scale=1.3), dict(base_depth=4, band=1)
    raise KeyError(name)


PARITY = ("two_levels", "two_spheres", "clipped", "hemisphere", "cap")       # the scenes with a band: compared level by level
NAMES = ("at_base", "all_active") + PARITY


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (points [n, 3], normals [n, 3], fields of mvs_poisson_params, fields of mvs_poisson_band_params)"""
    P, N, prm, bprm = _make(name)
    P.setflags(write=False)
    N.setflags(write=False)
    return P, N, prm, bprm


@functools.lru_cache(maxsize=None)
def reference(name):
    P, N, prm, bprm = scene(name)
    return RB.reconstruct(P, N, **bprm, **prm)
