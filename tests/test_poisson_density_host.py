"""Host side of mvs_poisson_reconstruct_density and mvs_mesh_trim_by_value (include/mvs.h, rules 14-18): symbols, the layouts and defaults
of mvs_poisson_density_params and mvs_poisson_density_info, the argument checks (they run before a device is needed), the conditions the
scenes of tests/poisson_density_scenes.py must meet for the GPU comparison to be exact, what the weighting and the trim achieve on the
numpy restatement tests/ref_poisson_density.py, and the shared rules header (csrc/poisson_rules.h) as a stand-alone program under the
address and undefined-behaviour sanitizers against numbers dumped from the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P
from tests import poisson_density_scenes as SC, ref_poisson as R, ref_poisson_density as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = -1, -4
BOTH = (False, True)


def _call(n=4, points=True, normals=True, prm=True, dprm=True, info=True, dinfo=True, vertices=True, density=True, faces=True, vcap=8, fcap=8,
          dfields=None, big=False, fn="mvs_poisson_reconstruct_density", **fields):
    rows = 2 ** 22 + 1 if big else 4
    pts, nrm = np.zeros((rows, 3)), np.zeros((rows, 3))
    pts[:4, 0] = np.arange(4)
    v, d, f = np.zeros((8, 3)), np.zeros(8), np.zeros((8, 3), np.int32)
    ci, di = L.CPoissonInfo(), L.CPoissonDensityInfo()
    p, dp = P.poisson_params(**fields), P.poisson_density_params(**(dfields or {}))
    args = [rows if big else n, L.ptr(pts) if points else None, L.ptr(nrm) if normals else None, C.byref(p) if prm else None,
            C.byref(dp) if dprm else None, C.byref(ci) if info else None, C.byref(di) if dinfo else None, L.ptr(v) if vertices else None,
            L.ptr(d) if density else None, vcap, L.ptr(f) if faces else None, fcap]
    if fn.endswith("_dev"):
        args.append(None)
    return getattr(L.lib(), fn)(*args)


def test_symbols_layouts_and_defaults():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_poisson_density_default_params", "mvs_poisson_reconstruct_density", "mvs_poisson_reconstruct_density_dev",
                 "mvs_mesh_trim_by_value", "mvs_mesh_trim_by_value_dev", "mvs_processor_poisson_density", "mvs_test_poisson_density"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T, I = L.CPoissonDensityParams, L.CPoissonDensityInfo
    assert C.sizeof(T) == 16 and T.max_gain.offset == 0 and T.flags.offset == 8 and T.density_drop.offset == 12
    assert C.sizeof(I) == 32 and I.mean_density.offset == 0 and I.min_point_density.offset == 8 and I.max_point_density.offset == 16
    assert I.density_depth.offset == 24 and I.n_clamped.offset == 28
    p = P.poisson_density_params()
    assert (p.max_gain, p.flags, p.density_drop) == (4.0, 0, 1) and P.WEIGHT_NORMALS == 1
    assert lib.mvs_abi_version() == 4
    assert C.sizeof(L.CPoissonParams) == 40 and C.sizeof(L.CPoissonInfo) == 80                # the plain call keeps its layout
    with pytest.raises(L.MvsError):
        P.poisson_density_params(gain=2.0)


W = dict(flags=1)
BAD = [dict(points=False), dict(normals=False), dict(prm=False), dict(dprm=False), dict(info=False), dict(dinfo=False), dict(vertices=False),
       dict(faces=False), dict(n=-1), dict(vcap=-1), dict(fcap=-1), dict(max_cycles=0), dict(scale=1.03125),
       dict(dfields=dict(max_gain=math.nan)), dict(dfields=dict(max_gain=math.inf)), dict(dfields=dict(max_gain=-math.inf)),
       dict(dfields=dict(max_gain=0.999)), dict(dfields=dict(max_gain=16.001)), dict(dfields=dict(max_gain=0.0)), dict(dfields=dict(max_gain=-4.0)),
       dict(dfields=dict(density_drop=-1)), dict(dfields=dict(density_drop=9)), dict(dfields=dict(flags=2)), dict(dfields=dict(flags=-1)),
       dict(dfields=W, big=True)]


def _id(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


@pytest.mark.parametrize("fn", ("mvs_poisson_reconstruct_density", "mvs_poisson_reconstruct_density_dev"))
@pytest.mark.parametrize("kw", BAD, ids=[_id(kw) for kw in BAD])
def test_argument_errors_need_no_device(kw, fn):
    assert _call(fn=fn, **kw) == E_INVALID
    assert fn.encode() in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    ok = (0, E_NO_DEVICE) if L.device_count() else (E_NO_DEVICE,)
    assert _call() in ok
    assert _call(density=False) in ok                                       # vertex_density may be NULL
    assert _call(dfields=dict(max_gain=1.0, density_drop=0, flags=1)) in ok
    assert _call(dfields=dict(max_gain=16.0, density_drop=8)) in ok
    if not L.device_count():
        assert _call(big=True) == E_NO_DEVICE                               # 2^22 + 1 rows are refused with the flag only


def _trim(V=3, F=1, vertices=True, normals=False, faces=True, values=True, thr=0.0, vout=True, nout=False, fout=True, nv=True, nf=True,
          fn="mvs_mesh_trim_by_value"):
    v, f, val = np.zeros((3, 3)), np.array([[0, 1, 2]], np.int32), np.ones(3)
    ov, on, of, cv, cf = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((1, 3), np.int32), C.c_int64(), C.c_int64()
    args = [V, L.ptr(v) if vertices else None, L.ptr(v) if normals else None, F, L.ptr(f) if faces else None, L.ptr(val) if values else None, thr,
            L.ptr(ov) if vout else None, L.ptr(on) if nout else None, L.ptr(of) if fout else None, C.byref(cv) if nv else None,
            C.byref(cf) if nf else None]
    if fn.endswith("_dev"):
        args.append(None)
    return getattr(L.lib(), fn)(*args)


TRIM_BAD = [dict(vertices=False), dict(faces=False), dict(values=False), dict(vout=False), dict(fout=False), dict(nv=False), dict(nf=False),
            dict(normals=True), dict(V=-1), dict(F=-1), dict(V=2 ** 31), dict(F=2 ** 31), dict(thr=math.nan)]


@pytest.mark.parametrize("fn", ("mvs_mesh_trim_by_value", "mvs_mesh_trim_by_value_dev"))
@pytest.mark.parametrize("kw", TRIM_BAD, ids=[_id(kw) for kw in TRIM_BAD])
def test_trim_argument_errors_need_no_device(kw, fn):
    assert _trim(fn=fn, **kw) == E_INVALID
    assert fn.encode() in L.lib().mvs_last_error()


def test_the_hook_and_the_file_entry_check_their_arguments_too(tmp_path):
    ok = (0, E_NO_DEVICE) if L.device_count() else (E_NO_DEVICE,)
    assert _trim() in ok and _trim(normals=True, nout=True) in ok and _trim(thr=-math.inf) in ok and _trim(thr=math.inf) in ok
    buf, ci, di = np.zeros((8, 3)), L.CPoissonInfo(), L.CPoissonDensityInfo()
    p, dp, bad_dp = P.poisson_params(), P.poisson_density_params(), P.poisson_density_params(max_gain=17.0)
    hook = L.lib().mvs_test_poisson_density
    assert hook(4, L.ptr(buf), L.ptr(buf), C.byref(p), C.byref(bad_dp), C.byref(ci), C.byref(di), L.ptr(buf), 8, L.ptr(buf), L.ptr(buf), L.ptr(buf), None,
                8) == E_INVALID
    assert b"mvs_test_poisson_density" in L.lib().mvs_last_error()
    assert hook(4, L.ptr(buf), L.ptr(buf), C.byref(p), C.byref(dp), C.byref(ci), C.byref(di), L.ptr(buf), 8, None, L.ptr(buf), L.ptr(buf), None, 8) == E_INVALID
    obj = os.fsencode(str(tmp_path / "m.obj"))
    assert L.lib().mvs_processor_poisson_density(None, C.byref(p), C.byref(dp), 0.25, obj, None, None) == E_INVALID
    assert L.lib().mvs_processor_poisson_density(obj, C.byref(p), C.byref(dp), 0.25, None, None, None) == E_INVALID
    assert L.lib().mvs_processor_poisson_density(obj, C.byref(p), None, math.nan, obj, None, None) == E_INVALID
    if L.device_count() == 0:
        with pytest.raises(L.MvsError) as e:
            P.PoissonFiles(str(tmp_path / "none.npts"), str(tmp_path / "m.obj"), dparams=P.poisson_density_params(flags=1), trim_ratio=0.25)
        assert e.value.code == E_NO_DEVICE and not (tmp_path / "m.obj").exists()
        with pytest.raises(L.MvsError) as e:
            P.TrimByValue(np.zeros((3, 3)), np.array([[0, 1, 2]]), np.ones(3), 0.5)
        assert e.value.code == E_NO_DEVICE


@pytest.mark.parametrize("weight", BOTH, ids=("plain", "weighted"))
@pytest.mark.parametrize("name", SC.NAMES)
def test_scene_conditions(name, weight):
    """what makes the GPU comparison at solve_tol = 1e-12 exact, as tests/test_poisson_host.py asks of its scenes — every node clears iso
    by 100 * 2E, the vertex bound B is at most 1e-4 h — and, for the new rules, no rho_mean / rho_p within 1e-9 relative of max_gain and
    no vertex density within 1e-9 relative of the trim threshold.  (Every scene has depth_min = depth_max: rule 3 has no choice.)"""
    pts, nrm, prm, dprm = SC.scene(name)
    ref = SC.reference(name, weight)
    D, h = ref["depth"], ref["h"]
    assert prm["depth_min"] == prm["depth_max"] == D == SC.DEPTHS[name] and ref["density_depth"] == SC.DENSITY_DEPTHS[name]
    assert 2000 <= len(pts) <= 8000 and ref["n_used"] == len(pts)
    E = R.stop_bound(SC.TOL, ref["rhs"], D)
    margin = float(np.abs(ref["chi"] - ref["iso"]).min())
    B = math.sqrt(3.0) * h * 4.0 * E / (ref["gap"] - 2.0 * E)
    max_gain = dprm.get("max_gain", 4.0)
    ratio = ref["rho_mean"] / ref["rho"]
    near_gain = float(np.abs(ratio / max_gain - 1.0).min())
    thr = SC.TRIM_RATIO * ref["rho_mean"]
    near_thr = float(np.abs(ref["vertex_density"] / thr - 1.0).min())
    print(f"{name} weight {weight}: D {D} Dd {ref['density_depth']} E {E:.2e} node margin {margin / (200.0 * E):.0f} x 200 E, B {B / h:.2e} h, rho_mean "
          f"{ref['rho_mean']:.4f} rho in [{ref['rho'].min():.3f}, {ref['rho'].max():.3f}] clamped {ref['n_clamped']} nearest gain {near_gain:.1e} "
          f"nearest threshold {near_thr:.1e}")
    assert margin >= 100.0 * 2.0 * E
    assert ref["gap"] > 2.0 * E and B <= 1e-4 * h
    assert ref["rel_residual"] <= 1e-13
    assert near_gain > 1e-9 and near_thr > 1e-9
    assert ref["rho"].min() >= 0.125 * (1.0 - 1e-9)                         # a point sees its own splat
    assert len(ref["vertices"]) > 100 and ref["vertex_density"].min() >= 0.0
    if name == "clamped":
        assert 0 < ref["n_clamped"] < len(pts)
    if name == "drop_floor":
        assert D - dprm["density_drop"] < 2 == ref["density_depth"]
    if name == "drop_zero":
        assert ref["Gd"] == ref["G"] and ref["hd"] == ref["h"]


def test_the_weighting_repairs_uneven_sampling_and_leaves_even_sampling_alone():
    """radial rms of the restatement's mesh about the unit sphere, in cells: on `uneven` and `seam` the weighted mesh has at most half the
    error of the unweighted one (measured: 0.052 h against 0.653 h, and 0.053 h against 0.236 h); on a uniformly sampled sphere the two
    agree to 25 % (0.050 h against 0.052 h: the method's own error)."""
    for name in ("uneven", "seam"):
        plain, weighted = SC.reference(name, False), SC.reference(name, True)
        rp, mp = RD.radial_rms(plain["vertices"], (0, 0, 0), 1.0, plain["h"])
        rw, mw = RD.radial_rms(weighted["vertices"], (0, 0, 0), 1.0, weighted["h"])
        print(f"{name}: radial rms {rp:.4f} h (max {mp:.3f} h) unweighted, {rw:.4f} h (max {mw:.3f} h) weighted")
        assert rw <= 0.5 * rp
        assert not np.array_equal(plain["rhs"], weighted["rhs"])
    plain, weighted = SC.reference("uniform", False), SC.reference("uniform", True)
    rp, rw = RD.radial_rms(plain["vertices"], (0, 0, 0), 1.0, plain["h"])[0], RD.radial_rms(weighted["vertices"], (0, 0, 0), 1.0, weighted["h"])[0]
    print(f"uniform: radial rms {rp:.4f} h unweighted, {rw:.4f} h weighted")
    assert abs(rw - rp) <= 0.25 * rp


def test_the_trim_removes_the_closure_of_an_open_scan():
    """`open` is a sphere cut at z = -0.2: the solve closes it (the untrimmed mesh is closed), the trim at 0.25 x the mean point density
    drops every vertex of the cap (z / r < -0.35), keeps every vertex of the sampled part (z / r > -0.1) and leaves one boundary loop"""
    for weight in BOTH:
        ref = SC.reference("open", weight)
        v, f, dv = ref["vertices"], ref["faces"], ref["vertex_density"]
        assert R.mesh_properties(v, f)[0]
        kept, kf = RD.trim(len(v), f, dv, SC.TRIM_RATIO * ref["rho_mean"])
        z = v[:, 2] / np.sqrt((v ** 2).sum(1))
        is_kept = np.zeros(len(v), bool)
        is_kept[kept] = True
        print(f"open weight {weight}: V {len(v)} kept {len(kept)}, faces {len(f)} kept {len(kf)}, cap vertices {int((z < -0.35).sum())}")
        assert (z < -0.35).sum() > 500 and not is_kept[z < -0.35].any() and is_kept[z > -0.1].all()
        assert kf.dtype == np.int32 and kf.min() == 0 and kf.max() == len(kept) - 1 and np.array_equal(np.unique(kf), np.arange(len(kept)))
        assert np.array_equal(v[kept][kf], v[f[is_kept[f].all(1)]])           # the same triangles, renumbered, in their order
        loops, simple = RD.boundary_loops(kf)
        assert simple and loops == 1
    # the edges of rule 18 on a tiny mesh: NaN does not pass, a passing vertex without a kept face goes, nothing kept is V = F = 0
    f = np.array([[0, 1, 2], [2, 1, 3], [3, 1, 4]], np.int32)
    kept, kf = RD.trim(6, f, np.array([1.0, 1.0, 1.0, np.nan, 1.0, 1.0]), 0.5)
    assert kept.tolist() == [0, 1, 2] and kf.tolist() == [[0, 1, 2]]
    kept, kf = RD.trim(6, f, np.ones(6), math.inf)
    assert len(kept) == 0 and kf.shape == (0, 3)
    kept, kf = RD.trim(6, f, np.ones(6), -math.inf)
    assert kept.tolist() == [0, 1, 2, 3, 4] and np.array_equal(kf, f)


def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "poisson_density_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "poisson_density_rules.cpp"), "-o", exe])
    return exe


def test_the_density_rules_under_the_sanitizers(tmp_path):
    """tests/poisson_density_rules.cpp: the floor of the density depth, the gain and its cut, ties of the density quantisation, NaN and
    infinities at the trim, a point's own splat; then the header against the restatement on two scenes — `clamped` (gains on both sides of
    max_gain) and `drop_floor` (Dd at its floor): quantised weights, rho_p, its quantised form, s_p and the vertex densities, bit for bit"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "poisson density rules ok" in run.stdout, run.stdout + run.stderr
    for name in ("clamped", "drop_floor"):
        pts, _, prm, dprm = SC.scene(name)
        ref = SC.reference(name, True)
        o, side, D, Gd, hd, S = ref["origin"], ref["side"], ref["depth"], ref["Gd"], ref["hd"], ref["node_sums"]
        max_gain, drop = dprm.get("max_gain", 4.0), dprm.get("density_drop", 1)
        Pp = np.concatenate([pts, [o, o + side]])                            # plus the two corners of the cube
        Vv = ref["vertices"]
        fin, fout = str(tmp_path / f"{name}.in"), str(tmp_path / f"{name}.out")
        with open(fin, "wb") as fh:
            fh.write(np.asarray(list(o) + [side, ref["rho_mean"], max_gain], np.float64).tobytes())
            fh.write(np.asarray([D, drop, len(Pp), len(Vv)], np.int32).tobytes())
            fh.write(np.ascontiguousarray(Pp, np.float64).tobytes())
            fh.write(np.ascontiguousarray(Vv, np.float64).tobytes())
            fh.write(np.ascontiguousarray(S, np.int64).tobytes())
        run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, run.stdout + run.stderr
        raw = open(fout, "rb").read()
        head = np.frombuffer(raw[:8], np.int32)
        assert head.tolist() == [ref["density_depth"], Gd] and np.frombuffer(raw[8:16], np.float64)[0] == hd
        rec = np.dtype([("q", "<i8", (8,)), ("rho", "<f8"), ("rq", "<i8"), ("s", "<f8")])
        got = np.frombuffer(raw[16:16 + rec.itemsize * len(Pp)], rec)
        _, w = R.corners_weights(Pp, o, hd, Gd)
        assert np.array_equal(got["q"], np.stack([np.rint(wc * RD.Q).astype(np.int64) for wc in w], 1))
        rho = RD.density_at(Pp, S, o, hd, Gd)
        assert got["rho"].tobytes() == rho.tobytes() and got["rho"][:len(pts)].tobytes() == ref["rho"].tobytes()
        assert np.array_equal(got["rq"], np.rint(rho * RD.QR).astype(np.int64))
        s, _ = RD.gains(rho, ref["rho_mean"], max_gain)
        assert got["s"].tobytes() == s.tobytes() and got["s"][:len(pts)].tobytes() == ref["gain"].tobytes()
        dv = np.frombuffer(raw[16 + rec.itemsize * len(Pp):], np.float64)
        assert dv.tobytes() == ref["vertex_density"].tobytes()
