"""mvs_poisson_reconstruct_band_density on the GPU (csrc/poisson_band.hip, rules 32-35 of include/mvs.h) against the numpy / scipy
restatement tests/ref_poisson_band_density.py on the scenes of tests/poisson_band_density_scenes.py, at solve_tol = 1e-12.  Level by
level through the hook: the node sums of the density grid, rho_p, s_p and the density info exactly, the active blocks, the node classes
and the weighted b exactly, chi within the accumulated bound of the two chains of solves; then the mesh — faces exactly
(tests/test_poisson_band_density_host.py checks on the restatement that no inside decision can move), vertices within B, the open
edges exactly, the vertex densities within B / hd * max(W), two runs the same bytes —; the dense density call where the band is the
whole grid and at or below the base depth; flags = 0 against the band call; the three forms, capacities, refusals, non-finite rows, the
trim of the file form and the quality of the device's own mesh.
Every array whose address goes into a raw call is bound to a name that lives until the call has returned."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P
from tests import poisson_band_density_calls as CALLS, poisson_band_density_scenes as S
from tests import ref_poisson_band as RB, ref_poisson_density as RD

pytestmark = pytest.mark.gpu
E_INVALID = -1


def params(name, **kw):
    return P.poisson_params(**dict(S.scene(name)[2], solve_tol=S.TOL, **kw))


def bparams(name):
    return P.poisson_band_params(**S.scene(name)[3])


def dparams(name, weight):
    return P.poisson_density_params(flags=P.WEIGHT_NORMALS if weight else 0, **S.scene(name)[4])


def run(name, weight, **kw):
    pts, nrm = S.scene(name)[:2]
    return P.RunPoissonBandDensity(pts, nrm, params(name), bparams(name), dparams(name, weight), **kw)


def ref_rel(l, lv):
    return lv["rel"] if "rel" in lv else lv["rel_residual"]


def bounds(ref, base_rel, band_rel, upto):
    """E = E_dev + E_ref, the accumulated bound with the device's own residuals plus the restatement's, both truncated at level `upto`"""
    cut = dict(ref, levels={l: lv for l, lv in ref["levels"].items() if l <= upto})
    return RB.accumulated_bound(cut, lambda l, lv: base_rel if l == ref["base_depth"] else band_rel[l]) + RB.accumulated_bound(cut, ref_rel)


def vertex_bound(ref, E):
    return math.sqrt(3.0) * ref["h"] * 4.0 * E / (ref["gap"] - 2.0 * E)


def hook(name, weight, l):
    """the hook on level l -> (status, info, binfo, dinfo, active, cls, b, chi, node_sums, rho, gain)"""
    pts, nrm = S.scene(name)[:2]
    prm, bprm, dprm = params(name), bparams(name), dparams(name, weight)
    n, n1, gb, nd = len(pts), 2 ** l + 1, 2 ** l // 4, (2 ** S.DENSITY_DEPTHS[name] + 1) ** 3
    active, cls = np.full(gb ** 3, 7, np.uint8), np.full(n1 ** 3, 7, np.uint8)
    b, chi = np.full(n1 ** 3, -1.0), np.full(n1 ** 3, -1.0)
    sums, rho, gain = np.full(nd, -1, np.int64), np.full(n, np.nan), np.full(n, np.nan)
    hp, hn = L.arr(pts, np.float64), L.arr(nrm, np.float64)
    info, binfo, dinfo = L.CPoissonInfo(), L.CPoissonBandInfo(), L.CPoissonDensityInfo()
    rc = L.lib().mvs_test_poisson_band_density_level(n, L.ptr(hp), L.ptr(hn), C.byref(prm), C.byref(bprm), C.byref(dprm), C.byref(info), C.byref(binfo),
                                                     C.byref(dinfo), l, L.ptr(active), L.ptr(cls), L.ptr(b), L.ptr(chi), n1 ** 3, L.ptr(sums), nd, L.ptr(rho),
                                                     L.ptr(gain))
    return rc, info, binfo, dinfo, active.reshape(gb, gb, gb), cls.reshape(n1, n1, n1), b.reshape(n1, n1, n1), chi.reshape(n1, n1, n1), sums, rho, gain


def check_density(ref, dinfo, sums, rho, gain):
    assert sums.tobytes() == ref["node_sums"].tobytes()
    assert rho.tobytes() == ref["rho"].tobytes()
    assert gain.tobytes() == ref["gain"].tobytes()
    assert dinfo.mean_density == ref["rho_mean"] and dinfo.min_point_density == ref["rho"].min() and dinfo.max_point_density == ref["rho"].max()
    assert dinfo.n_clamped == ref["n_clamped"] and dinfo.density_depth == ref["density_depth"]


LEVELS = [(name, l) for name in S.SIX for l in (5, 6)]


@pytest.mark.parametrize("name,l", LEVELS, ids=[f"{n}-{l}" for n, l in LEVELS])
def test_a_weighted_level_equals_the_restatement(name, l):
    ref = S.reference(name, True)
    lv = ref["levels"][l]
    rc, info, binfo, dinfo, active, cls, b, chi, sums, rho, gain = hook(name, True, l)
    assert rc == 0, L.lib().mvs_last_error()
    assert info.depth == ref["depth"] == 6 and binfo.base_depth == ref["base_depth"] == 4 and info.n_used == ref["n_used"] and info.h == ref["h"]
    assert list(info.origin) == ref["origin"].tolist() and ref["density_depth"] == S.DENSITY_DEPTHS[name]
    check_density(ref, dinfo, sums, rho, gain)
    assert np.array_equal(active, lv["act"].astype(np.uint8))
    assert np.array_equal(cls, lv["cls"])
    free = lv["cls"] == RB.FREE
    assert b[free].tobytes() == lv["b"][free].tobytes()
    assert b[free].tobytes() != S.reference(name, False)["levels"][l]["b"][free].tobytes()            # the weighting is in it
    assert np.array_equal(np.isnan(chi), np.isnan(lv["chi"])) and np.array_equal(np.isnan(b), np.isnan(lv["b"])) and (b[lv["cls"] == RB.FIXED] == 0.0).all()
    for q in (5, 6):
        assert binfo.n_active_blocks[q] == ref["levels"][q]["n_active"] and binfo.n_free[q] == ref["levels"][q]["n_free"], q
        assert binfo.rel_residual[q] <= S.TOL, q
    E = bounds(ref, info.rel_residual, binfo.rel_residual, l)
    has = ~np.isnan(lv["chi"])
    diff = float(np.abs(chi[has] - lv["chi"][has]).max())
    print(f"{name} level {l}: blocks {binfo.n_active_blocks[l]} free {binfo.n_free[l]} iterations {binfo.iterations[l]} rel_residual {binfo.rel_residual[l]:.2e} "
          f"max |chi - chi_ref| {diff:.2e} against {E:.2e}; scratch {binfo.scratch_bytes}")
    assert diff <= E
    assert info.rel_residual <= S.TOL and binfo.failed_level == 0
    if l == ref["depth"]:
        print(f"{name}: iso {info.iso!r} against {ref['iso']!r}")
        assert abs(info.iso - ref["iso"]) <= E


@pytest.mark.parametrize("name", S.SIX)
def test_the_weighted_mesh_equals_the_restatement_and_two_runs_agree(name):
    ref = S.reference(name, True)
    v, f, d, info, binfo, dinfo = run(name, True)
    assert info["depth"] == ref["depth"] and info["n_vertices"] == len(ref["vertices"]) == len(v) == len(d) and info["n_faces"] == len(ref["faces"]) == len(f)
    assert f.dtype == np.int32 and np.array_equal(f, ref["faces"])
    assert binfo["n_open_edges"] == ref["n_open_edges"] and (ref["n_open_edges"] > 0) == (name == "open6")
    E = bounds(ref, info["rel_residual"], binfo["rel_residual"], ref["depth"])
    B = vertex_bound(ref, E)
    dist = float(np.sqrt(((v - ref["vertices"]) ** 2).sum(1)).max())
    bound = RD.vertex_density_bound(B, ref["hd"], ref["node_sums"])
    ddiff = float(np.abs(d - ref["vertex_density"]).max())
    print(f"{name}: V {len(v)} F {len(f)} open {binfo['n_open_edges']} max vertex distance {dist:.2e} ({dist / ref['h']:.2e} h) against B {B:.2e}; "
          f"max |d_v - ref| {ddiff:.2e} against {bound:.2e}; iterations {binfo['iterations']} scratch {binfo['scratch_bytes']}")
    assert dist <= B and ddiff <= bound
    assert dinfo == dict(mean_density=ref["rho_mean"], min_point_density=ref["rho"].min(), max_point_density=ref["rho"].max(),
                         density_depth=ref["density_depth"], n_clamped=ref["n_clamped"])
    v2, f2, d2, info2, binfo2, dinfo2 = run(name, True)
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes() and d.tobytes() == d2.tobytes()
    assert binfo == binfo2 and dinfo == dinfo2 and info["iso"] == info2["iso"]


def test_with_every_block_active_the_density_and_b_are_those_of_the_dense_call():
    """all_active5 with the flag against mvs_test_poisson_density and RunPoissonDensity on the same points at depth 5 (Dd = 4 = B: the
    dense storage of rule 32)"""
    name = "all_active5"
    pts, nrm = S.scene(name)[:2]
    rc, info, binfo, dinfo, active, cls, b, chi, sums, rho, gain = hook(name, True, 5)
    assert rc == 0 and active.all() and info.depth == 5 and binfo.base_depth == 4 and dinfo.density_depth == 4
    n, nd, nn = len(pts), 17 ** 3, 33 ** 3
    dsums, drho, dgain, drhs = np.full(nd, -1, np.int64), np.full(n, np.nan), np.full(n, np.nan), np.full(nn, np.nan)
    ci, di, prm, dp = L.CPoissonInfo(), L.CPoissonDensityInfo(), params(name), dparams(name, True)
    L.check(L.lib().mvs_test_poisson_density(n, L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(dp), C.byref(ci), C.byref(di), L.ptr(dsums), nd, L.ptr(drho),
                                             L.ptr(dgain), L.ptr(drhs), None, nn))
    assert ci.depth == 5 and di.density_depth == 4
    assert sums.tobytes() == dsums.tobytes() and rho.tobytes() == drho.tobytes() and gain.tobytes() == dgain.tobytes()
    assert (dinfo.mean_density, dinfo.min_point_density, dinfo.max_point_density, dinfo.n_clamped) == (di.mean_density, di.min_point_density,
                                                                                                         di.max_point_density, di.n_clamped)
    free = cls == RB.FREE
    assert free.sum() == 31 ** 3 and b[free].tobytes() == drhs.reshape(33, 33, 33)[free].tobytes()
    check_density(S.reference(name, True), dinfo, sums, rho, gain)
    v, f, d, out, bout, dout = run(name, True)
    dv, df, dd, dinfo2 = P.RunPoissonDensity(pts, nrm, params(name), dparams(name, True))
    assert np.array_equal(f, df) and np.array_equal(f, S.reference(name, True)["faces"]) and len(v) == len(dv)
    assert dout["mean_density"] == dinfo2["mean_density"] and dout["n_clamped"] == dinfo2["n_clamped"]


@pytest.mark.parametrize("weight", (False, True), ids=("plain", "weighted"))
def test_at_or_below_the_base_depth_the_call_is_the_density_call(weight):
    pts, nrm = S.scene("at_base")[:2]
    v, f, d, info, binfo, dinfo = run("at_base", weight)
    dv, df, dd, dense = P.RunPoissonDensity(pts, nrm, params("at_base"), dparams("at_base", weight))
    assert info["depth"] == dense["depth"] == 5 and len(v) > 1000
    assert v.tobytes() == dv.tobytes() and f.tobytes() == df.tobytes() and d.tobytes() == dd.tobytes()
    for key, val in dict(info, **dinfo).items():
        assert np.array_equal(dense[key], val), key
    assert binfo == dict(P._poisson_band_info(L.CPoissonBandInfo()), base_depth=5)


def test_without_the_flag_the_bytes_are_those_of_the_band_call():
    """rule 35 on uneven6: vertices, faces, info and binfo — but for scratch_bytes, which counts the density structure —, with and
    without vertex_density; the vertex densities still meet the restatement"""
    name = "uneven6"
    pts, nrm = S.scene(name)[:2]
    ref = S.reference(name, False)
    bv, bf, binfo0, bband = P.RunPoissonBand(pts, nrm, params(name), bparams(name))
    v, f, d, info, binfo, dinfo = run(name, False)
    assert v.tobytes() == bv.tobytes() and f.tobytes() == bf.tobytes()
    for key, val in binfo0.items():
        assert np.array_equal(info[key], val), key
    assert dict(binfo, scratch_bytes=0) == dict(bband, scratch_bytes=0)
    assert binfo["scratch_bytes"] >= bband["scratch_bytes"] + 16 * len(pts)
    assert np.array_equal(f, ref["faces"]) and not np.array_equal(f, S.reference(name, True)["faces"])
    E = bounds(ref, info["rel_residual"], binfo["rel_residual"], ref["depth"])
    B = vertex_bound(ref, E)
    bound = RD.vertex_density_bound(B, ref["hd"], ref["node_sums"])
    ddiff = float(np.abs(d - ref["vertex_density"]).max())
    print(f"{name} flags 0: max |d_v - ref| {ddiff:.2e} against {bound:.2e}; scratch {binfo['scratch_bytes']} against the band call's {bband['scratch_bytes']}")
    assert ddiff <= bound and dinfo["mean_density"] == ref["rho_mean"] and dinfo["n_clamped"] == ref["n_clamped"]
    # without vertex_density
    ov, of = np.full((len(v), 3), np.nan), np.full((len(f), 3), -1, np.int32)
    prm, bp, dp, ci, bi, di = params(name), bparams(name), dparams(name, False), L.CPoissonInfo(), L.CPoissonBandInfo(), L.CPoissonDensityInfo()
    L.check(L.lib().mvs_poisson_reconstruct_band_density(len(pts), L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(bp), C.byref(dp), C.byref(ci), C.byref(bi),
                                                         C.byref(di), L.ptr(ov), None, len(v), L.ptr(of), len(f)))
    assert ov.tobytes() == bv.tobytes() and of.tobytes() == bf.tobytes() and ci.iso == binfo0["iso"] and di.mean_density == ref["rho_mean"]


def test_host_device_and_file_forms_agree(tmp_path):
    import torch
    name = "uneven6_drop2"
    pts, nrm = S.scene(name)[:2]
    v, f, d, info, binfo, dinfo = run(name, True)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sp, sn = torch.from_numpy(np.array(pts)).cuda(), torch.from_numpy(np.array(nrm)).cuda()
    assert torch.cuda.current_stream() != st                            # the points are pending on st; the call must order itself there
    for capacity in (None, (3, 5)):                                     # (3, 5): the first attempt is too small and the call is repeated
        sv, sf, sd, si, sb, sdi = P.RunPoissonBandDensity(sp, sn, params(name), bparams(name), dparams(name, True), stream=st.cuda_stream, capacity=capacity)
        assert sv.is_cuda and sf.is_cuda and sd.is_cuda and sd.dtype == torch.float64 and sf.dtype == torch.int32
        assert sv.cpu().numpy().tobytes() == v.tobytes() and sf.cpu().numpy().tobytes() == f.tobytes() and sd.cpu().numpy().tobytes() == d.tobytes()
        assert sb == binfo and sdi == dinfo and si["iso"] == info["iso"]
    # the raw device entry on that stream
    ov, of = torch.empty((len(v), 3), dtype=torch.float64, device="cuda"), torch.empty((len(f), 3), dtype=torch.int32, device="cuda")
    od = torch.empty(len(v), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    prm, bp, dp, ci, bi, di = params(name), bparams(name), dparams(name, True), L.CPoissonInfo(), L.CPoissonBandInfo(), L.CPoissonDensityInfo()
    L.check(L.lib().mvs_poisson_reconstruct_band_density_dev(len(pts), L.ptr(sp), L.ptr(sn), C.byref(prm), C.byref(bp), C.byref(dp), C.byref(ci), C.byref(bi),
                                                             C.byref(di), L.ptr(ov), L.ptr(od), len(v), L.ptr(of), len(f), L.ptr(st.cuda_stream)))
    assert ov.cpu().numpy().tobytes() == v.tobytes() and of.cpu().numpy().tobytes() == f.tobytes() and od.cpu().numpy().tobytes() == d.tobytes()
    # the file form: the formats carry six significant digits, so the arrays are those of the call on the points as the file holds them
    src, dst = str(tmp_path / "PSR.npts"), str(tmp_path / "Model.obj")
    IO.write_npts(src, np.array(pts), np.array(nrm))
    fp, fn = IO.read_npts(src)
    hv, hf, _, _, hb, _ = P.RunPoissonBandDensity(fp, fn, params(name), bparams(name), dparams(name, True))
    V, F, opened = C.c_int64(), C.c_int64(), C.c_int64(-1)
    prm, bp, dp = params(name), bparams(name), dparams(name, True)
    L.check(L.lib().mvs_processor_poisson_band_density(os.fsencode(src), C.byref(prm), C.byref(bp), C.byref(dp), 0.0, os.fsencode(dst), C.byref(V), C.byref(F),
                                                       C.byref(opened)))
    assert (V.value, F.value, opened.value) == (len(hv), len(hf), hb["n_open_edges"]) and V.value > 1000
    lines = open(dst).read().split("\n")
    ov = np.array([[float(x) for x in q.split()[1:4]] for q in lines if q.startswith("v ")])
    of = np.array([[int(x.split("/")[0]) - 1 for x in q.split()[1:4]] for q in lines if q.startswith("f ")], np.int32)
    assert sum(q.startswith("vn ") for q in lines) == V.value and np.array_equal(of, hf) and (np.abs(ov - hv) <= 5.1e-6 * np.abs(hv)).all()
    # dparams = NULL and trim_ratio = 0: the bytes of mvs_processor_poisson_band
    model = tmp_path / "Band.obj"                                        # one path: the file's head names it
    sizes = P.PoissonFiles(src, str(model), params(name), bparams=bparams(name))
    band = model.read_bytes()
    model.unlink()
    L.check(L.lib().mvs_processor_poisson_band_density(os.fsencode(src), C.byref(prm), C.byref(bp), None, 0.0, os.fsencode(str(model)), C.byref(V), C.byref(F), None))
    assert (V.value, F.value) == sizes and model.read_bytes() == band
    model.unlink()
    assert P.PoissonFiles(src, str(model), params(name), bparams=bparams(name), dparams=P.poisson_density_params(), trim_ratio=0.0) == sizes
    assert model.read_bytes() == band


def test_capacities_that_are_too_small_report_the_need():
    name = "uneven6_drop2"
    pts, nrm = S.scene(name)[:2]
    ref = S.reference(name, True)
    V, F = len(ref["vertices"]), len(ref["faces"])
    prm, bp, dp = params(name), bparams(name), dparams(name, True)
    for vcap, fcap in ((V - 1, F), (V, F - 1), (0, 0)):
        v, d, f = np.full((V, 3), np.nan), np.full(V, np.nan), np.full((F, 3), -1, np.int32)
        ci, bi, di = L.CPoissonInfo(), L.CPoissonBandInfo(), L.CPoissonDensityInfo()
        rc = L.lib().mvs_poisson_reconstruct_band_density(len(pts), L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(bp), C.byref(dp), C.byref(ci), C.byref(bi),
                                                          C.byref(di), L.ptr(v), L.ptr(d), vcap, L.ptr(f), fcap)
        assert rc == E_INVALID and b"capacity" in L.lib().mvs_last_error()
        assert (ci.n_vertices, ci.n_faces) == (V, F) and di.mean_density == ref["rho_mean"] and di.density_depth == 4
        assert bi.n_free[6] == ref["levels"][6]["n_free"] and bi.scratch_bytes > 0
        assert np.isnan(v).all() and np.isnan(d).all() and (f == -1).all()                  # nothing was written


@pytest.mark.parametrize("fn", CALLS.FORMS)
def test_every_refusal(fn):
    for kw in CALLS.BAD:
        assert CALLS.call(fn=fn, **kw) == E_INVALID, kw
        assert fn.encode() in L.lib().mvs_last_error(), kw


def test_non_finite_rows_change_nothing():
    name = "uneven6"
    pts, nrm = S.scene(name)[:2]
    v, f, d, info, binfo, dinfo = run(name, True)
    bad_p, bad_n = np.array(pts[:2]), np.array(nrm[:2])
    bad_p[0, 1] = np.nan
    bad_n[1, 2] = np.inf
    p2, n2 = np.concatenate([pts[:100], bad_p, pts[100:]]), np.concatenate([nrm[:100], bad_n, nrm[100:]])
    v2, f2, d2, info2, binfo2, dinfo2 = P.RunPoissonBandDensity(p2, n2, params(name), bparams(name), dparams(name, True))
    assert info2["n_used"] == info["n_used"] == len(pts) and v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes() and d2.tobytes() == d.tobytes()
    assert info2["iso"] == info["iso"] and dinfo2 == dinfo
    assert dict(binfo2, scratch_bytes=0) == dict(binfo, scratch_bytes=0)
    assert binfo2["scratch_bytes"] == binfo["scratch_bytes"] + 2 * 16                       # rho_p and s_p are kept per row, used or not


def test_the_trim_of_the_open_scene(tmp_path):
    """PoissonFiles(bparams, dparams, trim_ratio) on open6: RD.trim of the device's own mesh and density, and RunPoissonBandDensity
    followed by TrimByValue (on the points as the file holds them)"""
    name = "open6"
    pts, nrm = S.scene(name)[:2]
    src, dst = str(tmp_path / "PSR.npts"), str(tmp_path / "Model.obj")
    IO.write_npts(src, np.array(pts), np.array(nrm))
    fp, fn = IO.read_npts(src)
    v, f, d, info, binfo, dinfo = P.RunPoissonBandDensity(fp, fn, params(name), bparams(name), dparams(name, True))
    thr = S.TRIM_RATIO * dinfo["mean_density"]
    kept, kf = RD.trim(len(v), f, d, thr)
    tv, tf = P.TrimByValue(v, f, d, thr)
    assert 0 < len(kept) < len(v) and np.array_equal(tf, kf) and tv.tobytes() == v[kept].tobytes()
    V, F = P.PoissonFiles(src, dst, params(name), dparams=dparams(name, True), trim_ratio=S.TRIM_RATIO, bparams=bparams(name))
    Vu, Fu = P.PoissonFiles(src, str(tmp_path / "Model_u.obj"), params(name), dparams=dparams(name, True), trim_ratio=0.0, bparams=bparams(name))
    assert (V, F) == (len(kept), len(kf)) and (Vu, Fu) == (len(v), len(f)) and binfo["n_open_edges"] > 0
    lines = open(dst).read().split("\n")
    ov = np.array([[float(x) for x in q.split()[1:4]] for q in lines if q.startswith("v ")])
    of = np.array([[int(x.split("/")[0]) - 1 for x in q.split()[1:4]] for q in lines if q.startswith("f ")], np.int32)
    print(f"open6: V {len(v)} F {len(f)} open {binfo['n_open_edges']}; trimmed at {S.TRIM_RATIO} of the mean density V {V} F {F}")
    assert sum(q.startswith("vn ") for q in lines) == V and np.array_equal(of, kf) and (np.abs(ov - tv) <= 5.1e-6 * np.abs(tv)).all()


def test_the_radial_error_of_the_device_mesh():
    """uneven6: the device mesh's radial rms equals the restatement's (0.074 h weighted, 1.311 h unweighted) within B / h — every vertex
    lies within B of its reference — and is a tenth of the unweighted one"""
    rms = {}
    for weight in (False, True):
        ref = S.reference("uneven6", weight)
        v, f, d, info, binfo, dinfo = run("uneven6", weight)
        B = vertex_bound(ref, bounds(ref, info["rel_residual"], binfo["rel_residual"], ref["depth"]))
        rms[weight] = RD.radial_rms(v, (0, 0, 0), 1.0, info["h"])[0]
        want = RD.radial_rms(ref["vertices"], (0, 0, 0), 1.0, ref["h"])[0]
        print(f"uneven6 {'weighted' if weight else 'plain'}: radial rms {rms[weight]:.6f} h against the restatement's {want:.6f} h, B / h {B / ref['h']:.2e}")
        assert abs(rms[weight] - want) <= B / ref["h"]
    assert rms[True] <= 0.1 and rms[True] <= 0.1 * rms[False]
