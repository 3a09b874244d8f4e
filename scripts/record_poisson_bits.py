"""The bytes of the Poisson stage (csrc/poisson.hip, csrc/poisson_band.hip, csrc/mesh_trim.hip), recorded: for every case below the sha256 of the raw bytes of
every output array, the integer and floating fields of the info structs (floats as float.hex()) and the return code.  The library is built
with -ffp-contract=off and nothing in the stage but integer atomics is unordered, so these digests are a function of the written fp64
operations and their order; tests/test_gpu_poisson_bits.py holds every build to the recording in tests/golden/poisson_bits.json.  The
restatements solve directly, so the other tests hold chi to a bound only and cannot see a changed operation order in the solver.

The cases are the smallest that reach each path of the solver, at solve_tol = 1e-12 as in the scene files:
  field/<scene>        mvs_test_poisson_field: `hemisphere` D = 3 (two levels, all in the one workgroup), `picked` (rule 3 chooses),
                       `ellipsoid` D = 5 (the top of the coarse kernel)
  density/<scene>      mvs_test_poisson_density with MVS_POISSON_WEIGHT_NORMALS: `clamped`, `drop_floor`
  screened/<scene>/<diagonal>
                       mvs_test_poisson_screened: diagonal 0 on `d3`, `d4_alpha64`, `d4_weighted`, `d6` (D = 6: the launched levels);
                       diagonals 1 and 2 on `d4` and `d6`
  depth7/<call>        the three public host calls on poisson_scenes.big_sphere() at depth 7: two launched levels above the coarse kernel
  trim/open            mvs_mesh_trim_by_value on the mesh of `open` at TRIM_RATIO
and for the band levels (rules 24-35), whose conjugate gradients, iso sum and extraction the restatements hold to a bound only:
  band/<scene>         RunPoissonBand on `two_levels`, `clipped`, `hemisphere`, `cap`, `all_active` of tests/poisson_band_scenes.py: both
                       forms of the level below, the grid boundary, base depth 3, open edges, the band that is the whole grid; the mesh,
                       info and the band info (scratch_bytes of rule 35 included)
  band_level/two_levels/<l>
                       mvs_test_poisson_band_level on levels 5 and 6: active, cls, b, chi
  band_density/<scene>[/unweighted]
                       RunPoissonBandDensity with MVS_POISSON_WEIGHT_NORMALS on `uneven6` (the sums in blocks), `uneven6_drop2` (dense
                       sums) and `open6` of tests/poisson_band_density_scenes.py, and on `uneven6` without the flag: the mesh, the vertex
                       densities and the three info structs
  band_density_level/uneven6/6
                       mvs_test_poisson_band_density_level with the flag: node_sums, rho, gain, active, cls, b, chi

A deliberate change of the solver's arithmetic re-records: build the library, then on a GPU
  python scripts/record_poisson_bits.py --parent $(git rev-parse HEAD) --out tests/golden/poisson_bits.json
`--only <case> ...` records some cases (to compare two diagnostics builds, say); without --out the JSON goes to stdout."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOL = 1e-12
CASES = (("field/hemisphere", "field/picked", "field/ellipsoid", "density/clamped", "density/drop_floor") +
         tuple(f"screened/{name}/0" for name in ("d3", "d4_alpha64", "d4_weighted", "d6")) +
         tuple(f"screened/{name}/{diag}" for diag in (1, 2) for name in ("d4", "d6")) +
         ("depth7/plain", "depth7/density", "depth7/screened", "trim/open") +
         tuple(f"band/{name}" for name in ("two_levels", "clipped", "hemisphere", "cap", "all_active")) +
         ("band_level/two_levels/5", "band_level/two_levels/6") +
         ("band_density/uneven6", "band_density/uneven6_drop2", "band_density/open6", "band_density/uneven6/unweighted") +
         ("band_density_level/uneven6/6",))


def digest(a) -> str:
    """sha256 of the raw bytes of an array, in C order"""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fields(info) -> dict:
    """the fields of an info struct, or of the info dict of multiviewstitch_amd.processor: integers as they are, floats as float.hex()"""
    items = info.items() if isinstance(info, dict) else ((k, getattr(info, k)) for k, _ in info._fields_)
    out = {}
    for k, v in items:
        v = list(v) if isinstance(v, (C.Array, np.ndarray)) else v
        if isinstance(v, list):
            out[k] = [float(x).hex() for x in v]
        else:
            out[k] = float(v).hex() if isinstance(v, (float, np.floating)) else int(v)
    return out


def _field(scene):
    from multiviewstitch_amd import _lib as L, processor as P
    from tests import poisson_scenes as PS
    pts, nrm, prm = PS.scene(scene)
    prm = P.poisson_params(**dict(prm, solve_tol=TOL))
    nn = (2 ** PS.DEPTHS[scene] + 1) ** 3
    rhs, chi, info = np.full(nn, np.nan), np.full(nn, np.nan), L.CPoissonInfo()
    rc = L.lib().mvs_test_poisson_field(len(pts), L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(info), L.ptr(rhs), L.ptr(chi), nn)
    return dict(rc=rc, arrays=dict(rhs=digest(rhs), chi=digest(chi)), info=fields(info))


def _density(scene):
    from multiviewstitch_amd import _lib as L, processor as P
    from tests import poisson_density_scenes as DS
    pts, nrm, prm, dprm = DS.scene(scene)
    prm, dp = P.poisson_params(**dict(prm, solve_tol=TOL)), P.poisson_density_params(flags=P.WEIGHT_NORMALS, **dprm)
    n, nd, nn = len(pts), (2 ** DS.DENSITY_DEPTHS[scene] + 1) ** 3, (2 ** DS.DEPTHS[scene] + 1) ** 3
    sums, rho, gain, rhs, chi = np.full(nd, -1, np.int64), np.full(n, np.nan), np.full(n, np.nan), np.full(nn, np.nan), np.full(nn, np.nan)
    info, dinfo = L.CPoissonInfo(), L.CPoissonDensityInfo()
    rc = L.lib().mvs_test_poisson_density(n, L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(dp), C.byref(info), C.byref(dinfo), L.ptr(sums), nd,
                                          L.ptr(rho), L.ptr(gain), L.ptr(rhs), L.ptr(chi), nn)
    return dict(rc=rc, arrays=dict(node_sums=digest(sums), rho=digest(rho), gain=digest(gain), rhs=digest(rhs), chi=digest(chi)),
                info=fields(info), dinfo=fields(dinfo))


def _screened(scene, diagonal):
    from multiviewstitch_amd import _lib as L, processor as P
    from tests import poisson_screened_scenes as SC
    pts, nrm, prm, dprm, weight, alpha = SC.scene(scene)
    prm, sp = P.poisson_params(**dict(prm, solve_tol=TOL)), P.poisson_screen_params(alpha=alpha)
    dp = P.poisson_density_params(flags=P.WEIGHT_NORMALS if weight else 0, **dprm)
    nn = (2 ** SC.DEPTHS[scene] + 1) ** 3
    st, f, chi0, chi = np.full((nn, 27), -1, np.int64), np.full(nn, np.nan), np.full(nn, np.nan), np.full(nn, np.nan)
    info, dinfo, sinfo = L.CPoissonInfo(), L.CPoissonDensityInfo(), L.CPoissonScreenInfo()
    rc = L.lib().mvs_test_poisson_screened(len(pts), L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(dp), C.byref(sp), C.byref(info), C.byref(dinfo),
                                           C.byref(sinfo), L.ptr(st), L.ptr(f), L.ptr(chi0), L.ptr(chi), nn, int(diagonal))
    return dict(rc=rc, arrays=dict(stencil=digest(st), f=digest(f), chi0=digest(chi0), chi=digest(chi)), info=fields(info), dinfo=fields(dinfo),
                sinfo=fields(sinfo))


def _depth7(call):
    from multiviewstitch_amd import processor as P
    from tests import poisson_scenes as PS
    pts, nrm = PS.big_sphere()
    prm = P.poisson_params(depth_min=7, depth_max=7, solve_tol=TOL)
    if call == "plain":
        v, f, info = P.RunPoisson(pts, nrm, prm)
        return dict(rc=0, arrays=dict(vertices=digest(v), faces=digest(f)), info=fields(info))
    v, f, d, info = (P.RunPoissonDensity if call == "density" else P.RunPoissonScreened)(pts, nrm, prm)
    return dict(rc=0, arrays=dict(vertices=digest(v), faces=digest(f), vertex_density=digest(d)), info=fields(info))


def _trim(scene):
    from multiviewstitch_amd import processor as P
    from tests import poisson_density_scenes as DS
    pts, nrm, prm, dprm = DS.scene(scene)
    v, f, d, info = P.RunPoissonDensity(pts, nrm, P.poisson_params(**dict(prm, solve_tol=TOL)), P.poisson_density_params(**dprm))
    tv, tf, tn = P.TrimByValue(v, f, d, DS.TRIM_RATIO * info["mean_density"], normals=-v)
    return dict(rc=0, arrays=dict(vertices=digest(tv), faces=digest(tf), normals=digest(tn)), info=dict(V=len(tv), F=len(tf)))


def _band(scene):
    from multiviewstitch_amd import processor as P
    from tests import poisson_band_scenes as BS
    pts, nrm, prm, bprm = BS.scene(scene)
    v, f, info, binfo = P.RunPoissonBand(pts, nrm, P.poisson_params(**dict(prm, solve_tol=TOL)), P.poisson_band_params(**bprm))
    return dict(rc=0, arrays=dict(vertices=digest(v), faces=digest(f)), info=fields(info), binfo=fields(binfo))


def _band_level(scene, level):
    from multiviewstitch_amd import _lib as L, processor as P
    from tests import poisson_band_scenes as BS
    pts, nrm, prm, bprm = BS.scene(scene)
    prm, bp = P.poisson_params(**dict(prm, solve_tol=TOL)), P.poisson_band_params(**bprm)
    nn, nb = (2 ** int(level) + 1) ** 3, (2 ** int(level) // 4) ** 3
    active, cls, b, chi = np.full(nb, 7, np.uint8), np.full(nn, 7, np.uint8), np.full(nn, -1.0), np.full(nn, -1.0)
    hp, hn = L.arr(pts, np.float64), L.arr(nrm, np.float64)
    info, binfo = L.CPoissonInfo(), L.CPoissonBandInfo()
    rc = L.lib().mvs_test_poisson_band_level(len(hp), L.ptr(hp), L.ptr(hn), C.byref(prm), C.byref(bp), C.byref(info), C.byref(binfo), int(level),
                                             L.ptr(active), L.ptr(cls), L.ptr(b), L.ptr(chi), nn)
    return dict(rc=rc, arrays=dict(active=digest(active), cls=digest(cls), b=digest(b), chi=digest(chi)), info=fields(info), binfo=fields(binfo))


def _band_density_params(scene, weight):
    from multiviewstitch_amd import processor as P
    from tests import poisson_band_density_scenes as S
    pts, nrm, prm, bprm, dprm = S.scene(scene)
    return (pts, nrm, P.poisson_params(**dict(prm, solve_tol=TOL)), P.poisson_band_params(**bprm),
            P.poisson_density_params(flags=P.WEIGHT_NORMALS if weight else 0, **dprm))


def _band_density(scene, weight="weighted"):
    from multiviewstitch_amd import processor as P
    v, f, d, info, binfo, dinfo = P.RunPoissonBandDensity(*_band_density_params(scene, weight == "weighted"))
    return dict(rc=0, arrays=dict(vertices=digest(v), faces=digest(f), vertex_density=digest(d)), info=fields(info), binfo=fields(binfo),
                dinfo=fields(dinfo))


def _band_density_level(scene, level):
    from multiviewstitch_amd import _lib as L
    from tests import poisson_band_density_scenes as S
    pts, nrm, prm, bp, dp = _band_density_params(scene, True)
    n, nn, nb, nd = len(pts), (2 ** int(level) + 1) ** 3, (2 ** int(level) // 4) ** 3, (2 ** S.DENSITY_DEPTHS[scene] + 1) ** 3
    active, cls, b, chi = np.full(nb, 7, np.uint8), np.full(nn, 7, np.uint8), np.full(nn, -1.0), np.full(nn, -1.0)
    sums, rho, gain = np.full(nd, -1, np.int64), np.full(n, np.nan), np.full(n, np.nan)
    hp, hn = L.arr(pts, np.float64), L.arr(nrm, np.float64)
    info, binfo, dinfo = L.CPoissonInfo(), L.CPoissonBandInfo(), L.CPoissonDensityInfo()
    rc = L.lib().mvs_test_poisson_band_density_level(n, L.ptr(hp), L.ptr(hn), C.byref(prm), C.byref(bp), C.byref(dp), C.byref(info), C.byref(binfo),
                                                     C.byref(dinfo), int(level), L.ptr(active), L.ptr(cls), L.ptr(b), L.ptr(chi), nn, L.ptr(sums), nd,
                                                     L.ptr(rho), L.ptr(gain))
    return dict(rc=rc, arrays=dict(node_sums=digest(sums), rho=digest(rho), gain=digest(gain), active=digest(active), cls=digest(cls), b=digest(b),
                                   chi=digest(chi)), info=fields(info), binfo=fields(binfo), dinfo=fields(dinfo))


def record(case) -> dict:
    kind, *rest = case.split("/")
    return dict(field=_field, density=_density, screened=_screened, depth7=_depth7, trim=_trim, band=_band, band_level=_band_level,
                band_density=_band_density, band_density_level=_band_density_level)[kind](*rest)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the commit the library was built from")
    ap.add_argument("--only", nargs="+", choices=CASES, help="these cases only")
    ap.add_argument("--out", help="the file to write (default: stdout)")
    a = ap.parse_args()
    text = json.dumps(dict(parent=a.parent, solve_tol=TOL, cases={c: record(c) for c in (a.only or CASES)}), indent=1, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
