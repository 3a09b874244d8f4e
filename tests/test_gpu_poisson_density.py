"""mvs_poisson_reconstruct_density and mvs_mesh_trim_by_value on the GPU (csrc/poisson.hip, rules 14-18 of include/mvs.h) against the numpy
restatement tests/ref_poisson_density.py on the scenes of tests/poisson_density_scenes.py, at solve_tol = 1e-12: with flags = 0 the bytes of
mvs_poisson_reconstruct; the node sums of the density grid, rho_p, s_p, the density info and the weighted right-hand side exactly; the
weighted mesh — faces exactly, chi within E + E_ref, vertices within the scene's bound B, vertex densities within B / hd * max(W) —
tests/test_poisson_density_host.py checks on the restatement that no decision of these scenes can move under those bounds —; what the
weighting achieves on the device's own meshes; the trim against the restatement and at its edges; run-to-run identity, the host, device
and torch forms, capacities; the file form and its chain into the trim of the model."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P
from tests import poisson_density_scenes as SC, poisson_scenes as PS, ref_poisson as R, ref_poisson_density as RD

pytestmark = pytest.mark.gpu
E_INVALID, E_BAD_MESH = -1, -2
BOTH = (False, True)
IDS = ("plain", "weighted")


def params(name, **kw):
    return P.poisson_params(**dict(SC.scene(name)[2], solve_tol=SC.TOL, **kw))


def dparams(name, weight):
    return P.poisson_density_params(flags=P.WEIGHT_NORMALS if weight else 0, **SC.scene(name)[3])


def run(name, weight, **kw):
    pts, nrm, _, _ = SC.scene(name)
    return P.RunPoissonDensity(pts, nrm, params(name), dparams(name, weight), **kw)


def hook(name, weight, with_chi):
    pts, nrm, _, _ = SC.scene(name)
    n, nd, nn = len(pts), (2 ** SC.DENSITY_DEPTHS[name] + 1) ** 3, (2 ** SC.DEPTHS[name] + 1) ** 3
    sums, rho, gain = np.full(nd, -1, np.int64), np.full(n, np.nan), np.full(n, np.nan)
    rhs, chi = np.full(nn, np.nan), np.full(nn, np.nan)
    info, dinfo, prm, dp = L.CPoissonInfo(), L.CPoissonDensityInfo(), params(name), dparams(name, weight)
    rc = L.lib().mvs_test_poisson_density(n, L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(dp), C.byref(info), C.byref(dinfo), L.ptr(sums), nd,
                                          L.ptr(rho), L.ptr(gain), L.ptr(rhs), L.ptr(chi) if with_chi else None, nn)
    return rc, info, dinfo, sums, rho, gain, rhs, chi


@pytest.mark.parametrize("name", PS.NAMES)
def test_without_the_flag_the_bytes_are_those_of_the_plain_call(name):
    pts, nrm, prm = PS.scene(name)
    prm = P.poisson_params(**dict(prm, solve_tol=PS.TOL))
    v, f, info = P.RunPoisson(pts, nrm, prm)
    dv, df, dens, dinfo = P.RunPoissonDensity(pts, nrm, prm)
    assert dv.tobytes() == v.tobytes() and df.tobytes() == f.tobytes() and len(dens) == len(v) and np.isfinite(dens).all()
    for key, val in info.items():
        assert np.array_equal(dinfo[key], val), key
    assert dinfo["density_depth"] == max(info["depth"] - 1, 2) and dinfo["n_clamped"] >= 0 and dinfo["mean_density"] >= 0.125
    # without vertex_density
    ov, of, ci, di, dp = np.full((len(v), 3), np.nan), np.full((len(f), 3), -1, np.int32), L.CPoissonInfo(), L.CPoissonDensityInfo(), P.poisson_density_params()
    L.check(L.lib().mvs_poisson_reconstruct_density(len(pts), L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(dp), C.byref(ci), C.byref(di), L.ptr(ov), None,
                                                    len(v), L.ptr(of), len(f)))
    assert ov.tobytes() == v.tobytes() and of.tobytes() == f.tobytes() and ci.iso == info["iso"] and ci.cycles == info["cycles"]
    assert ci.rel_residual == info["rel_residual"] and di.mean_density == dinfo["mean_density"]


@pytest.mark.parametrize("weight", BOTH, ids=IDS)
@pytest.mark.parametrize("name", SC.NAMES)
def test_the_density_equals_the_restatement(name, weight):
    ref = SC.reference(name, weight)
    rc, info, dinfo, sums, rho, gain, rhs, _ = hook(name, weight, False)
    assert rc == 0 and info.depth == ref["depth"] and info.n_used == ref["n_used"] and info.h == ref["h"]
    assert list(info.origin) == ref["origin"].tolist()
    assert sums.tobytes() == ref["node_sums"].tobytes()
    assert rho.tobytes() == ref["rho"].tobytes()
    assert gain.tobytes() == ref["gain"].tobytes()
    assert dinfo.mean_density == ref["rho_mean"] and dinfo.min_point_density == ref["rho"].min() and dinfo.max_point_density == ref["rho"].max()
    assert dinfo.n_clamped == ref["n_clamped"] and dinfo.density_depth == ref["density_depth"] == SC.DENSITY_DEPTHS[name]
    assert rhs.tobytes() == ref["rhs"].reshape(-1).tobytes()
    if weight and name in ("uneven", "clamped"):
        assert rhs.tobytes() != SC.reference(name, False)["rhs"].reshape(-1).tobytes()


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_weighted_mesh_equals_the_restatement(name):
    """E bounds what the stopping rule moves any chi value by, B what that moves a vertex by (tests/test_poisson_host.py).  A vertex
    displacement of at most B moves its density by at most B times the density's largest slope, max(W) / hd along an axis for a trilinear
    W whose node values lie in [0, max W]: ref_poisson_density.vertex_density_bound."""
    ref = SC.reference(name, True)
    rc, info, dinfo, _, _, _, _, chi = hook(name, True, True)
    assert rc == 0
    E = R.stop_bound(SC.TOL, ref["rhs"], ref["depth"])
    E_ref = R.stop_bound(ref["rel_residual"], ref["rhs"], ref["depth"])
    diff = float(np.abs(chi - ref["chi"].reshape(-1)).max())
    print(f"{name}: cycles {info.cycles} rel_residual {info.rel_residual:.2e} max |chi - chi_ref| {diff:.2e} against E + E_ref {E + E_ref:.2e}")
    assert diff <= E + E_ref and abs(info.iso - ref["iso"]) <= E + E_ref and info.rel_residual <= SC.TOL
    v, f, d, out = run(name, True)
    assert out["n_vertices"] == len(ref["vertices"]) == len(v) == len(d) and out["n_faces"] == len(ref["faces"]) == len(f)
    assert f.dtype == np.int32 and np.array_equal(f, ref["faces"])
    B = math.sqrt(3.0) * ref["h"] * 4.0 * E / (ref["gap"] - 2.0 * E)
    dist = float(np.sqrt(((v - ref["vertices"]) ** 2).sum(1)).max())
    bound = RD.vertex_density_bound(B, ref["hd"], ref["node_sums"])
    ddiff = float(np.abs(d - ref["vertex_density"]).max())
    print(f"{name}: V {len(v)} F {len(f)} max vertex distance {dist:.2e} against B {B:.2e}; max |d_v - ref| {ddiff:.2e} against {bound:.2e}")
    assert dist <= B and ddiff <= bound
    assert out["iso"] == info.iso and out["mean_density"] == ref["rho_mean"] and out["n_clamped"] == ref["n_clamped"]
    if name in ("uneven", "seam"):
        assert not np.array_equal(f, SC.reference(name, False)["faces"])


@pytest.mark.parametrize("name", ("uneven", "seam"))
def test_the_weighting_halves_the_radial_error_of_the_device_mesh(name):
    rms = {}
    for weight in BOTH:
        v, f, d, info = run(name, weight)
        rms[weight] = RD.radial_rms(v, (0, 0, 0), 1.0, info["h"])
    print(f"{name}: radial rms {rms[False][0]:.4f} h (max {rms[False][1]:.3f} h) unweighted, {rms[True][0]:.4f} h (max {rms[True][1]:.3f} h) weighted")
    assert rms[True][0] <= 0.5 * rms[False][0]


def _device_trim(v, f, values, thr, **kw):
    """-> (indices of the kept vertices, kept faces, kept vertices): the index of every vertex rides along as its normal"""
    tag = np.zeros((len(v), 3))
    tag[:, 0] = np.arange(len(v))
    tv, tf, tn = P.TrimByValue(v, f, values, thr, normals=tag, **kw)
    return tn[:, 0].astype(np.int64), tf, tv


@pytest.mark.parametrize("weight", BOTH, ids=IDS)
def test_the_trim_of_the_open_scene_equals_the_restatement(weight):
    ref = SC.reference("open", weight)
    v, f, d, info = run("open", weight)
    thr = SC.TRIM_RATIO * info["mean_density"]
    kept, kf = RD.trim(len(ref["vertices"]), ref["faces"], ref["vertex_density"], SC.TRIM_RATIO * ref["rho_mean"])
    gk, gf, gv = _device_trim(v, f, d, thr)
    assert np.array_equal(gk, kept) and gf.dtype == np.int32 and np.array_equal(gf, kf) and gv.tobytes() == v[kept].tobytes()
    z = gv[:, 2] / np.sqrt((gv ** 2).sum(1))
    assert 0 < len(gk) < len(v) and z.min() > -0.35
    assert RD.boundary_loops(gf) == (1, True)
    g2 = _device_trim(v, f, d, thr)
    assert g2[1].tobytes() == gf.tobytes() and g2[2].tobytes() == gv.tobytes()               # two runs, the same bytes


def _random_mesh(V, F, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(V, 3)), rng.integers(0, V, size=(F, 3)).astype(np.int32), rng.uniform(0.0, 1.0, V)


def test_trim_edges():
    ref = SC.reference("drop_floor", False)
    v, f, d = np.array(ref["vertices"]), np.array(ref["faces"]), np.array(ref["vertex_density"])
    tv, tf = P.TrimByValue(v, f, d, -math.inf)
    assert tv.tobytes() == v.tobytes() and tf.tobytes() == f.tobytes()                        # the identity: every vertex of the mesh lies in a face
    tv, tf = P.TrimByValue(v, f, d, math.inf)
    assert tv.shape == (0, 3) and tf.shape == (0, 3)
    d[f[7, 1]] = np.nan
    kept, kf = RD.trim(len(v), f, d, -math.inf)
    gk, gf, _ = _device_trim(v, f, d, -math.inf)
    assert len(kept) < len(v) and np.array_equal(gk, kept) and np.array_equal(gf, kf)
    # one face
    tri_v, tri_f = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[2, 0, 1]], np.int32)
    tv, tf = P.TrimByValue(tri_v, tri_f, np.array([1.0, 2.0, 3.0]), 1.0)
    assert tv.tobytes() == tri_v.tobytes() and tf.tolist() == [[2, 0, 1]]
    tv, tf = P.TrimByValue(tri_v, tri_f, np.array([1.0, 2.0, 3.0]), 1.5)
    assert len(tv) == 0 and len(tf) == 0
    tv, tf = P.TrimByValue(np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros(0), 0.0)
    assert len(tv) == 0 and len(tf) == 0
    with pytest.raises(L.MvsError) as e:
        P.TrimByValue(tri_v, np.array([[0, 1, 3]], np.int32), np.ones(3), 0.0)
    assert e.value.code == E_BAD_MESH
    with pytest.raises(L.MvsError) as e:
        P.TrimByValue(tri_v, np.array([[0, -1, 2]], np.int32), np.ones(3), 0.0)
    assert e.value.code == E_BAD_MESH


@pytest.mark.parametrize("V,F", [(255, 255), (256, 256), (257, 257), (255, 257), (257, 255), (700, 1500)])
def test_trim_across_the_workgroup_size_of_the_compaction(V, F):
    v, f, val = _random_mesh(V, F, 100 * V + F)
    for thr in (0.3, 0.0):
        kept, kf = RD.trim(V, f, val, thr)
        gk, gf, gv = _device_trim(v, f, val, thr)
        assert 0 < len(kf) and np.array_equal(gk, kept) and np.array_equal(gf, kf) and gv.tobytes() == v[kept].tobytes()
    last_v = np.zeros(V)
    last_v[[V - 1, V - 2, 0]] = 1.0                                                          # the last slots of the last workgroup
    f[F - 1] = (V - 1, 0, V - 2)
    kept, kf = RD.trim(V, f, last_v, 0.5)
    gk, gf, _ = _device_trim(v, f, last_v, 0.5)
    assert np.array_equal(gk, kept) and np.array_equal(gf, kf) and kept.tolist() == [0, V - 2, V - 1] and kf[-1].tolist() == [2, 0, 1]


def test_two_runs_and_the_host_device_and_torch_forms_agree():
    import torch
    pts, nrm, _, _ = SC.scene("clamped")
    v, f, d, info = run("clamped", True)
    v2, f2, d2, info2 = run("clamped", True)
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes() and d.tobytes() == d2.tobytes() and info2["iso"] == info["iso"]
    tp, tn = torch.from_numpy(np.array(pts)).cuda(), torch.from_numpy(np.array(nrm)).cuda()
    torch.cuda.synchronize()
    dv, df, dd, dinfo = P.RunPoissonDensity(tp, tn, params("clamped"), dparams("clamped", True))
    assert dv.is_cuda and df.is_cuda and dd.is_cuda and dd.dtype == torch.float64 and df.dtype == torch.int32
    assert dv.cpu().numpy().tobytes() == v.tobytes() and df.cpu().numpy().tobytes() == f.tobytes() and dd.cpu().numpy().tobytes() == d.tobytes()
    assert dinfo["mean_density"] == info["mean_density"] and dinfo["n_clamped"] == info["n_clamped"] and dinfo["cycles"] == info["cycles"]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sp, sn = torch.from_numpy(np.array(pts)).cuda(), torch.from_numpy(np.array(nrm)).cuda()
    assert torch.cuda.current_stream() != st                            # the points are pending on st; the call must order itself there
    for capacity in (None, (3, 5)):                                     # (3, 5): the first attempt is too small and the call is repeated
        sv, sf, sd, _ = P.RunPoissonDensity(sp, sn, params("clamped"), dparams("clamped", True), stream=st.cuda_stream, capacity=capacity)
        assert sv.cpu().numpy().tobytes() == v.tobytes() and sf.cpu().numpy().tobytes() == f.tobytes() and sd.cpu().numpy().tobytes() == d.tobytes()
    # the trim on tensors, ordered on the stream that made them
    thr = 0.5 * info["mean_density"]
    hv, hf = P.TrimByValue(v, f, d, thr)
    assert 0 < len(hv) < len(v)
    tv, tf = P.TrimByValue(sv, sf, sd, thr, stream=st.cuda_stream)
    assert tv.is_cuda and tf.is_cuda and tv.cpu().numpy().tobytes() == hv.tobytes() and tf.cpu().numpy().tobytes() == hf.tobytes()
    # the raw device entry
    ov, of = torch.empty((len(v), 3), dtype=torch.float64, device="cuda"), torch.empty((len(f), 3), dtype=torch.int32, device="cuda")
    od = torch.empty(len(v), dtype=torch.float64, device="cuda")
    prm, dp, ci, di = params("clamped"), dparams("clamped", True), L.CPoissonInfo(), L.CPoissonDensityInfo()
    L.check(L.lib().mvs_poisson_reconstruct_density_dev(len(pts), L.ptr(tp), L.ptr(tn), C.byref(prm), C.byref(dp), C.byref(ci), C.byref(di), L.ptr(ov),
                                                        L.ptr(od), len(v), L.ptr(of), len(f), None))
    assert ov.cpu().numpy().tobytes() == v.tobytes() and of.cpu().numpy().tobytes() == f.tobytes() and od.cpu().numpy().tobytes() == d.tobytes()


def test_capacities_that_are_too_small_report_the_need():
    pts, nrm, _, _ = SC.scene("drop_floor")
    ref = SC.reference("drop_floor", True)
    V, F = len(ref["vertices"]), len(ref["faces"])
    prm, dp = params("drop_floor"), dparams("drop_floor", True)
    for vcap, fcap in ((V - 1, F), (V, F - 1), (0, 0)):
        v, d, f = np.full((V, 3), np.nan), np.full(V, np.nan), np.full((F, 3), -1, np.int32)
        ci, di = L.CPoissonInfo(), L.CPoissonDensityInfo()
        rc = L.lib().mvs_poisson_reconstruct_density(len(pts), L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(dp), C.byref(ci), C.byref(di), L.ptr(v), L.ptr(d),
                                                     vcap, L.ptr(f), fcap)
        assert rc == E_INVALID and b"capacity" in L.lib().mvs_last_error()
        assert (ci.n_vertices, ci.n_faces) == (V, F) and di.mean_density == ref["rho_mean"] and di.density_depth == 2
        assert np.isnan(v).all() and np.isnan(d).all() and (f == -1).all()                  # nothing was written


def test_the_file_form_and_its_chain_into_the_cull(tmp_path):
    from tests import pointsample_scenes as PSS
    cameras, depths, p = PSS.scene("AB")
    got = P.RunPointSample(cameras, depths, PSS.c_params(p))
    paths = []
    for k, (pp, nn, _, _) in enumerate(got):
        paths.append(str(tmp_path / f"seq{k}.npts"))
        IO.write_npts(paths[-1], pp, nn)
    res = tmp_path / "Result"
    res.mkdir()
    scales, Rs, ts = np.ones(2), np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))
    assert P.StitchPointSets(paths, scales, Rs, ts, cameras, str(res), truncate=True).sum() > 100
    psr = str(res / "PSR.npts")
    prm = P.poisson_params(depth_min=5, depth_max=5, scale=1.3)          # 800 points: a 33^3 grid holds several per node of the density grid
    model = res / "Model.obj"                                            # one path: the file's head names it
    V0, F0 = P.PoissonFiles(psr, str(model), prm)
    plain = model.read_bytes()
    model.unlink()
    Vd, Fd = C.c_int64(), C.c_int64()
    L.check(L.lib().mvs_processor_poisson_density(os.fsencode(psr), C.byref(prm), None, 0.0, os.fsencode(str(model)), C.byref(Vd), C.byref(Fd)))
    assert (Vd.value, Fd.value) == (V0, F0) and model.read_bytes() == plain
    model.unlink()
    assert P.PoissonFiles(psr, str(model), prm, dparams=P.poisson_density_params()) == (V0, F0) and model.read_bytes() == plain
    V, F = P.PoissonFiles(psr, str(res / "Model_w.obj"), prm, dparams=P.poisson_density_params(flags=P.WEIGHT_NORMALS), trim_ratio=0.25)
    lines = (res / "Model_w.obj").read_text().split("\n")
    assert 100 < V and 100 < F
    assert sum(q.startswith("v ") for q in lines) == V == sum(q.startswith("vn ") for q in lines) and sum(q.startswith("f ") for q in lines) == F
    Vu, Fu = P.PoissonFiles(psr, str(res / "Model_u.obj"), prm, dparams=P.poisson_density_params(flags=P.WEIGHT_NORMALS))
    assert V < Vu and F < Fu                                                                # the trim only removes
    Vc, Fc = P.CullPoissonModel(str(res / "Model_w.obj"), scales, Rs, ts, cameras, str(res / "Model_cull.obj"))
    print(f"chain: plain V {V0} F {F0}; weighted V {Vu} F {Fu}; trimmed at 0.25 V {V} F {F}; culled V {Vc} F {Fc}")
    assert 0 < Vc <= V and 0 < Fc <= F
