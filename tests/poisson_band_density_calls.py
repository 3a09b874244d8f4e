"""Raw calls of mvs_poisson_reconstruct_band_density(_dev) on four points, and the table of what the call refuses before a device is
needed (include/mvs.h behind rule 35): shared by tests/test_poisson_band_density_host.py and tests/test_gpu_poisson_band_density.py.
Every array whose address goes into a call is bound to a name that lives until the call has returned."""
import ctypes as C
import math

import numpy as np

from multiviewstitch_amd import _lib as L, processor as P

E_INVALID, E_NO_DEVICE = -1, -4
FORMS = ("mvs_poisson_reconstruct_band_density", "mvs_poisson_reconstruct_band_density_dev")


def call(fn=FORMS[0], n=4, points=True, normals=True, prm=True, bprm=True, dprm=True, info=True, binfo=True, dinfo=True, vertices=True, density=True,
         faces=True, vcap=8, fcap=8, bfields=None, reserved=(0, 0), dfields=None, big=False, **fields):
    rows = 2 ** 22 + 1 if big else 4
    pts, nrm = np.zeros((rows, 3)), np.zeros((rows, 3))
    pts[:4, 0] = np.arange(4)
    v, d, f = np.zeros((8, 3)), np.zeros(8), np.zeros((8, 3), np.int32)
    ci, bi, di = L.CPoissonInfo(), L.CPoissonBandInfo(), L.CPoissonDensityInfo()
    p, bp, dp = P.poisson_params(**fields), P.poisson_band_params(**(bfields or {})), P.poisson_density_params(**(dfields or {}))
    bp.reserved[0], bp.reserved[1] = reserved
    args = [rows if big else n, L.ptr(pts) if points else None, L.ptr(nrm) if normals else None, C.byref(p) if prm else None,
            C.byref(bp) if bprm else None, C.byref(dp) if dprm else None, C.byref(ci) if info else None, C.byref(bi) if binfo else None,
            C.byref(di) if dinfo else None, L.ptr(v) if vertices else None, L.ptr(d) if density else None, vcap, L.ptr(f) if faces else None, fcap]
    if fn.endswith("_dev"):
        args.append(None)
    return getattr(L.lib(), fn)(*args)


# what the band call refuses ...
BAND = [dict(points=False), dict(normals=False), dict(prm=False), dict(info=False), dict(vertices=False), dict(faces=False), dict(n=-1),
        dict(bprm=False), dict(binfo=False), dict(bfields=dict(base_depth=2)), dict(bfields=dict(base_depth=10)), dict(bfields=dict(band=0)),
        dict(bfields=dict(band=65)), dict(reserved=(1, 0)), dict(reserved=(0, -1)), dict(depth_min=11, depth_max=11), dict(vcap=-1), dict(fcap=-1),
        dict(max_cycles=0), dict(scale=1.03125), dict(depth_min=8, depth_max=7)]
# ... and what the density call refuses of dparams and dinfo
DENSITY = [dict(dprm=False), dict(dinfo=False), dict(dfields=dict(max_gain=math.nan)), dict(dfields=dict(max_gain=math.inf)),
           dict(dfields=dict(max_gain=0.999)), dict(dfields=dict(max_gain=16.001)), dict(dfields=dict(density_drop=-1)),
           dict(dfields=dict(density_drop=9)), dict(dfields=dict(flags=2)), dict(dfields=dict(flags=-1)), dict(dfields=dict(flags=1), big=True)]
BAD = BAND + DENSITY


def ident(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())
