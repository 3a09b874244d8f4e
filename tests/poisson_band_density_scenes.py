"""Scenes for mvs_poisson_reconstruct_band_density (rules 32-35 of include/mvs.h): the points of tests/poisson_density_scenes.py — a
unit sphere about the origin whose sampling density is not uniform — forced to a band depth, all with scale 1.3 and solve_tol 1e-12.
The restatement of a scene (tests/ref_poisson_band_density.py), with and without the weighting of rule 33, is computed once per
process and shared by the tests; nobody changes it.  tests/test_poisson_band_density_host.py holds the scenes to the conditions that
keep them from testing nothing."""
import functools

import numpy as np

from tests import poisson_density_scenes as DS, ref_poisson_band_density as RBD

TOL = DS.TOL
TRIM_RATIO = DS.TRIM_RATIO

# name -> (points of, D, base_depth, band, density fields)
_SCENES = dict(
    uneven6=("uneven", 6, dict(base_depth=4, band=1), dict(density_drop=1)),        # Dd = 5 > B: block storage
    uneven6_drop2=("uneven", 6, dict(base_depth=4, band=1), dict(density_drop=2)),  # Dd = 4 = B: dense storage
    uneven6_drop0=("uneven", 6, dict(base_depth=4, band=1), dict(density_drop=0)),  # Dd = D
    open6=("open", 6, dict(base_depth=4, band=1), dict(density_drop=1)),            # open edges and the trim
    all_active5=("uneven", 5, dict(base_depth=4, band=8), {}),                      # every block active
    at_base=("uneven", 5, dict(base_depth=5), {}),                                  # D <= B
)
SIX = ("uneven6", "uneven6_drop2", "uneven6_drop0", "open6")                        # compared level by level
UNEVEN6 = ("uneven6", "uneven6_drop2", "uneven6_drop0")
NAMES = SIX + ("all_active5", "at_base")
DENSITY_DEPTHS = dict(uneven6=5, uneven6_drop2=4, uneven6_drop0=6, open6=5, all_active5=4, at_base=4)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (points [n, 3], normals [n, 3], fields of mvs_poisson_params, of mvs_poisson_band_params, of mvs_poisson_density_params
    without the flag)"""
    src, D, bprm, dprm = _SCENES[name]
    P, N, _, _ = DS.scene(src)
    return P, N, dict(depth_min=D, depth_max=D, scale=1.3), dict(bprm), dict(dprm)


@functools.lru_cache(maxsize=None)
def reference(name, weight):
    P, N, prm, bprm, dprm = scene(name)
    ref = RBD.reconstruct(P, N, weight=bool(weight), **bprm, **dprm, **prm)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref
