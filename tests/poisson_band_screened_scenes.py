"""Scenes and raw calls for mvs_poisson_reconstruct_band_screened (rules 36-41 of include/mvs.h), shared by
tests/test_poisson_band_screened_host.py and tests/test_gpu_poisson_band_screened.py: `two_levels`, `clipped` and `cap` of
tests/poisson_band_scenes.py, `uneven6` of tests/poisson_band_density_scenes.py with the weight flag, all at alpha = 4, and
`block_corners` at alpha = 64; all at solve_tol 1e-12, levels 5 and 6 only.  The restatement of a scene
(tests/ref_poisson_band_screened.py) is computed once per process and shared by the tests; nobody changes it.

block_corners: 400-odd points near a sphere of radius 0.7, one in every level-6 cell whose index is 3 mod 4 on all three axes and
whose centre lies in the shell, plus the two corners (-1, -1, -1) and (1, 1, 1), which fix the cube.  The eight corners of such a cell
belong to eight different stored blocks, and the row of the cell's high corner reaches seven other blocks.  The cube of rule 2 is centred
on the bounding box, so the cells of the two extreme points of an axis add up to 2^6 - 1 = 63 = 3 (mod 4): not both can be 3 mod 4, and
no scene can hold EVERY used point to the property.  The corner (-1, -1, -1) lies in cell (7, 7, 7) and keeps it; (1, 1, 1) lies in
cell (56, 56, 56), the one point that does not (tests/test_poisson_band_screened_host.py asserts all of this)."""
import ctypes as C
import functools
import math

import numpy as np

from multiviewstitch_amd import _lib as L, processor as P
from tests import poisson_band_density_scenes as DS, poisson_band_scenes as BS, ref_poisson_band_screened as RBS

TOL = 1e-12
E_INVALID = -1
BLOCK_CORNERS_SCALE = 1.306
LEVEL_SCENES = ("two_levels", "clipped", "cap", "uneven6", "block_corners")


def _block_corners():
    side = 2.0 * BLOCK_CORNERS_SCALE
    h, o = side / 64.0, -0.5 * side
    rng = np.random.default_rng(41)
    idx = np.array([(4 * a + 3, 4 * b + 3, 4 * c + 3) for c in range(2, 14) for b in range(2, 14) for a in range(2, 14)], np.float64)
    centre = o + h * (idx + 0.5)
    r = np.sqrt((centre ** 2).sum(1))
    keep = (r >= 0.55) & (r <= 0.85)
    pts = o + h * (idx[keep] + rng.uniform(0.2, 0.8, (int(keep.sum()), 3)))
    pts = np.concatenate([[[-1.0, -1.0, -1.0]], pts, [[1.0, 1.0, 1.0]]])
    return pts, pts / np.sqrt((pts ** 2).sum(1))[:, None]


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (points, normals, fields of mvs_poisson_params, of mvs_poisson_band_params, of mvs_poisson_density_params with the flag, alpha)"""
    if name == "uneven6":
        pts, nrm, prm, bprm, dprm = DS.scene(name)
        return pts, nrm, prm, bprm, dict(dprm, flags=P.WEIGHT_NORMALS), 4.0
    if name == "block_corners":
        pts, nrm = _block_corners()
        pts.setflags(write=False)
        nrm.setflags(write=False)
        return pts, nrm, dict(depth_min=6, depth_max=6, scale=BLOCK_CORNERS_SCALE), dict(base_depth=4, band=1), dict(flags=0), 64.0
    if name == "at_base":
        pts, nrm, prm, bprm, dprm = DS.scene(name)
        return pts, nrm, prm, bprm, dict(dprm, flags=0), 4.0
    pts, nrm, prm, bprm = BS.scene(name)
    return pts, nrm, dict(prm), dict(bprm), dict(flags=0), 4.0


@functools.lru_cache(maxsize=None)
def reference(name):
    pts, nrm, prm, bprm, dprm, alpha = scene(name)
    dkw = {k: v for k, v in dprm.items() if k != "flags"}
    ref = RBS.reconstruct(pts, nrm, weight=bool(dprm["flags"]), alpha=alpha, **bprm, **dkw, **prm)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def structs(name, alpha=None, **kw):
    pts, nrm, prm, bprm, dprm, a = scene(name)
    return (P.poisson_params(**dict(prm, solve_tol=TOL, **kw)), P.poisson_band_params(**bprm), P.poisson_density_params(**dprm),
            P.poisson_screen_params(alpha=a if alpha is None else alpha))


# ------------------------------------------------------------------ raw calls on four points ----
FORMS = ("mvs_poisson_reconstruct_band_screened", "mvs_poisson_reconstruct_band_screened_dev")


def call(fn=FORMS[0], n=4, points=True, normals=True, prm=True, bprm=True, dprm=True, sprm=True, info=True, binfo=True, dinfo=True, sinfo=True, bsinfo=True,
         vertices=True, density=True, faces=True, vcap=8, fcap=8, bfields=None, reserved=(0, 0), dfields=None, sfields=None, big=False, **fields):
    rows = 2 ** 22 + 1 if big else 4
    pts, nrm = np.zeros((rows, 3)), np.zeros((rows, 3))
    pts[:4, 0] = np.arange(4)
    v, d, f = np.zeros((8, 3)), np.zeros(8), np.zeros((8, 3), np.int32)
    ci, bi, di, si, bsi = L.CPoissonInfo(), L.CPoissonBandInfo(), L.CPoissonDensityInfo(), L.CPoissonScreenInfo(), L.CPoissonBandScreenInfo()
    p, bp, dp = P.poisson_params(**fields), P.poisson_band_params(**(bfields or {})), P.poisson_density_params(**(dfields or {}))
    sp = P.poisson_screen_params(**(sfields or {}))
    bp.reserved[0], bp.reserved[1] = reserved
    args = [rows if big else n, L.ptr(pts) if points else None, L.ptr(nrm) if normals else None, C.byref(p) if prm else None,
            C.byref(bp) if bprm else None, C.byref(dp) if dprm else None, C.byref(ci) if info else None, C.byref(bi) if binfo else None,
            C.byref(di) if dinfo else None, L.ptr(v) if vertices else None, L.ptr(d) if density else None, vcap, L.ptr(f) if faces else None, fcap]
    if fn.endswith("_dev"):
        args.append(None)
    args += [C.byref(sp) if sprm else None, C.byref(si) if sinfo else None, C.byref(bsi) if bsinfo else None]
    return getattr(L.lib(), fn)(*args)


# what the band-density call refuses (tests/poisson_band_density_calls.py's table, restated) ...
BAND_DENSITY = [dict(points=False), dict(normals=False), dict(prm=False), dict(info=False), dict(vertices=False), dict(faces=False), dict(n=-1),
                dict(bprm=False), dict(binfo=False), dict(bfields=dict(base_depth=2)), dict(bfields=dict(base_depth=10)), dict(bfields=dict(band=0)),
                dict(bfields=dict(band=65)), dict(reserved=(1, 0)), dict(reserved=(0, -1)), dict(depth_min=11, depth_max=11), dict(vcap=-1), dict(fcap=-1),
                dict(max_cycles=0), dict(scale=1.03125), dict(depth_min=8, depth_max=7), dict(dprm=False), dict(dinfo=False),
                dict(dfields=dict(max_gain=math.nan)), dict(dfields=dict(max_gain=math.inf)), dict(dfields=dict(max_gain=0.999)),
                dict(dfields=dict(max_gain=16.001)), dict(dfields=dict(density_drop=-1)), dict(dfields=dict(density_drop=9)), dict(dfields=dict(flags=2)),
                dict(dfields=dict(flags=-1)), dict(dfields=dict(flags=1), big=True)]
# ... what the dense screened call refuses of sparams and sinfo, and a NULL bsinfo
SCREEN = [dict(sprm=False), dict(sinfo=False), dict(bsinfo=False), dict(sfields=dict(alpha=math.nan)), dict(sfields=dict(alpha=math.inf)),
          dict(sfields=dict(alpha=-0.001)), dict(sfields=dict(alpha=64.001)), dict(sfields=dict(reserved=1))]
BAD = BAND_DENSITY + SCREEN
