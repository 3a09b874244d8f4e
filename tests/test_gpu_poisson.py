"""mvs_poisson_reconstruct on the GPU (csrc/poisson.hip) against the numpy / scipy restatement tests/ref_poisson.py on the scenes of
tests/poisson_scenes.py, at solve_tol = 1e-12: depth, grid and the right-hand side exactly (integer sums), chi within the bound E + E_ref
that the two stopping residuals allow, the faces exactly and the vertices within the scene's bound B — tests/test_poisson_host.py checks
on the restatement that no inside decision of these scenes can move under 2E —; then run-to-run identity, the host, device and torch
forms, capacities, non-finite rows, the other status codes, one call at depth 7 and the chain into the trim of the model."""
import ctypes as C
import math

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P
from tests import poisson_scenes as SC, ref_poisson as R

pytestmark = pytest.mark.gpu
E_INVALID, E_SOLVER, E_DEGENERATE = -1, -7, -9


def params(name, **kw):
    return P.poisson_params(**dict(SC.scene(name)[2], solve_tol=SC.TOL, **kw))


def field(points, normals, prm):
    n1 = 2 ** min(prm.depth_max, 9) + 1
    rhs, chi, info = np.full(n1 ** 3, np.nan), np.full(n1 ** 3, np.nan), L.CPoissonInfo()
    pts, nrm = L.arr(points, np.float64), L.arr(normals, np.float64)
    rc = L.lib().mvs_test_poisson_field(len(pts), L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(info), L.ptr(rhs), L.ptr(chi), n1 ** 3)
    m = (2 ** info.depth + 1) ** 3
    return rc, info, rhs[:m], chi[:m]


def raw_call(points, normals, prm, vcap, fcap):
    pts, nrm = L.arr(points, np.float64), L.arr(normals, np.float64)
    v, f, info = np.full((max(vcap, 1), 3), np.nan), np.full((max(fcap, 1), 3), -1, np.int32), L.CPoissonInfo()
    rc = L.lib().mvs_poisson_reconstruct(len(pts), L.ptr(pts), L.ptr(nrm), C.byref(prm), C.byref(info), L.ptr(v), vcap, L.ptr(f), fcap)
    return rc, info, v, f


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_field_equals_the_restatement(name):
    pts, nrm, _ = SC.scene(name)
    ref = SC.reference(name)
    prm = params(name)
    rc, info, rhs, chi = field(pts, nrm, prm)
    assert rc == 0
    assert info.depth == ref["depth"] == SC.DEPTHS[name] and info.n_used == ref["n_used"]
    assert list(info.origin) == ref["origin"].tolist() and info.h == ref["h"]
    assert rhs.tobytes() == ref["rhs"].reshape(-1).tobytes()
    E = R.stop_bound(SC.TOL, ref["rhs"], ref["depth"])
    E_ref = R.stop_bound(ref["rel_residual"], ref["rhs"], ref["depth"])
    diff = float(np.abs(chi - ref["chi"].reshape(-1)).max())
    print(f"{name}: cycles {info.cycles} rel_residual {info.rel_residual:.2e} max |chi - chi_ref| {diff:.2e} against E + E_ref {E + E_ref:.2e}; "
          f"iso {info.iso!r} against {ref['iso']!r}")
    assert diff <= E + E_ref
    assert info.rel_residual <= SC.TOL and 1 <= info.cycles <= prm.max_cycles
    assert abs(info.iso - ref["iso"]) <= E + E_ref


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_mesh_equals_the_restatement_and_two_runs_agree(name):
    pts, nrm, _ = SC.scene(name)
    ref = SC.reference(name)
    v, f, info = P.RunPoisson(pts, nrm, params(name))
    assert info["n_vertices"] == len(ref["vertices"]) == len(v) and info["n_faces"] == len(ref["faces"]) == len(f)
    assert f.dtype == np.int32 and np.array_equal(f, ref["faces"])
    E = R.stop_bound(SC.TOL, ref["rhs"], ref["depth"])
    B = math.sqrt(3.0) * ref["h"] * 4.0 * E / (ref["gap"] - 2.0 * E)
    diff = float(np.sqrt(((v - ref["vertices"]) ** 2).sum(1)).max())
    print(f"{name}: V {len(v)} F {len(f)} max vertex distance {diff:.2e} ({diff / ref['h']:.2e} h) against B {B:.2e} ({B / ref['h']:.2e} h)")
    assert diff <= B
    v2, f2, _ = P.RunPoisson(pts, nrm, params(name))
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes()


def test_host_device_and_torch_forms_agree():
    import torch
    pts, nrm, _ = SC.scene("sphere")
    v, f, info = P.RunPoisson(pts, nrm, params("sphere"))
    tp, tn = torch.from_numpy(np.array(pts)).cuda(), torch.from_numpy(np.array(nrm)).cuda()
    torch.cuda.synchronize()
    dv, df, dinfo = P.RunPoisson(tp, tn, params("sphere"))
    assert dv.is_cuda and df.is_cuda and dv.dtype == torch.float64 and df.dtype == torch.int32
    assert dv.cpu().numpy().tobytes() == v.tobytes() and df.cpu().numpy().tobytes() == f.tobytes()
    assert dinfo["iso"] == info["iso"] and dinfo["cycles"] == info["cycles"] and dinfo["rel_residual"] == info["rel_residual"]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sp, sn = torch.from_numpy(np.array(pts)).cuda(), torch.from_numpy(np.array(nrm)).cuda()
    assert torch.cuda.current_stream() != st                            # the points are pending on st; the call must order itself there
    for capacity in (None, (3, 5)):                                     # (3, 5): the first attempt is too small and the call is repeated
        sv, sf, _ = P.RunPoisson(sp, sn, params("sphere"), stream=st.cuda_stream, capacity=capacity)
        assert sv.cpu().numpy().tobytes() == v.tobytes() and sf.cpu().numpy().tobytes() == f.tobytes()
    # the raw device entry
    cap_v, cap_f = len(v), len(f)
    ov, of = torch.empty((cap_v, 3), dtype=torch.float64, device="cuda"), torch.empty((cap_f, 3), dtype=torch.int32, device="cuda")
    prm, ci = params("sphere"), L.CPoissonInfo()
    L.check(L.lib().mvs_poisson_reconstruct_dev(len(pts), L.ptr(tp), L.ptr(tn), C.byref(prm), C.byref(ci), L.ptr(ov), cap_v, L.ptr(of), cap_f, None))
    assert ov.cpu().numpy().tobytes() == v.tobytes() and of.cpu().numpy().tobytes() == f.tobytes()


def test_capacities_that_are_too_small_report_the_need():
    pts, nrm, _ = SC.scene("hemisphere")
    ref = SC.reference("hemisphere")
    V, F = len(ref["vertices"]), len(ref["faces"])
    for vcap, fcap in ((V - 1, F), (V, F - 1), (0, 0)):
        rc, info, v, f = raw_call(pts, nrm, params("hemisphere"), vcap, fcap)
        assert rc == E_INVALID and b"capacity" in L.lib().mvs_last_error()
        assert (info.n_vertices, info.n_faces) == (V, F) and np.isnan(v).all() and (f == -1).all()          # nothing was written
    rc, info, v, f = raw_call(pts, nrm, params("hemisphere"), info.n_vertices, info.n_faces)                  # sized by the (0, 0) call
    assert rc == 0 and np.array_equal(f, ref["faces"]) and not np.isnan(v).any()


def test_non_finite_rows_are_not_used():
    pts, nrm, _ = SC.scene("hemisphere")
    v, f, info = P.RunPoisson(pts, nrm, params("hemisphere"))
    bad_p, bad_n = np.array(pts[:2]), np.array(nrm[:2])
    bad_p[0, 1] = np.nan
    bad_n[1, 2] = np.inf
    p2, n2 = np.concatenate([pts[:100], bad_p, pts[100:]]), np.concatenate([nrm[:100], bad_n, nrm[100:]])
    v2, f2, info2 = P.RunPoisson(p2, n2, params("hemisphere"))
    assert info2["n_used"] == info["n_used"] == len(pts) and v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    assert info2["iso"] == info["iso"]
    v3, f3, info3 = P.RunPoisson(p2[:150], n2[:150], params("hemisphere"))
    assert info3["n_used"] == 148


def test_the_other_status_codes():
    pts, nrm, _ = SC.scene("sphere")
    with pytest.raises(L.MvsError) as e:
        P.RunPoisson(pts, nrm, params("sphere", max_cycles=1))
    assert e.value.code == E_SOLVER and "residual" in str(e.value)
    rc, info, _, _ = field(pts, nrm, params("sphere", max_cycles=1))
    assert rc == E_SOLVER and info.cycles == 1 and SC.TOL < info.rel_residual < 1.0
    for p1, n1 in ((pts[:1], nrm[:1]), (np.repeat(pts[:1], 5, 0), nrm[:5]), (np.zeros((0, 3)), np.zeros((0, 3)))):
        with pytest.raises(L.MvsError) as e:
            P.RunPoisson(p1, n1, params("sphere"))
        assert e.value.code == E_DEGENERATE
    v, f, info = P.RunPoisson(pts, np.zeros_like(pts), params("sphere"))
    assert len(v) == 0 and len(f) == 0 and info["n_vertices"] == 0 and info["n_faces"] == 0 and info["cycles"] == 0


def test_depth_7_with_60000_points():
    """a 129^3 grid: the levels 7 and 6 run as launches of their own, the five below in one workgroup; the two compactions span tens of
    thousands of workgroups.  Checked by properties: closed, outward (the signed volume
    is positive), genus 0, the sphere's volume, the residual."""
    pts, nrm = SC.big_sphere()
    v, f, info = P.RunPoisson(pts, nrm, P.poisson_params(depth_min=7, depth_max=7))
    closed, euler, comps, vol = R.mesh_properties(v, f)
    print(f"depth 7: V {len(v)} F {len(f)} cycles {info['cycles']} rel_residual {info['rel_residual']:.2e} volume {vol:.4f} iso {info['iso']:.4g}")
    assert info["depth"] == 7 and info["n_used"] == len(pts) and info["rel_residual"] <= 1e-8 and info["cycles"] <= 64
    assert closed and comps == 1 and euler == 2
    rad = np.sqrt(((v - np.array([0.1, 0.2, 0.3])) ** 2).sum(1))
    print(f"depth 7: radial error {np.abs(rad - 1.0).max() / info['h']:.3f} h")
    # a surface that stays within one cell of the unit sphere encloses its volume to within 3 h / r
    assert abs(vol - 4.0 / 3.0 * math.pi) <= 3.0 * info["h"] * 4.0 / 3.0 * math.pi


def test_chain_point_sample_stitch_poisson_cull(tmp_path):
    from tests import pointsample_scenes as PS
    cameras, depths, p = PS.scene("AB")
    got = P.RunPointSample(cameras, depths, PS.c_params(p))
    paths = []
    for k, (pp, nn, _, _) in enumerate(got):
        paths.append(str(tmp_path / f"seq{k}.npts"))
        IO.write_npts(paths[-1], pp, nn)
    res = tmp_path / "Result"
    res.mkdir()
    scales, Rs, ts = np.ones(2), np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))
    assert P.StitchPointSets(paths, scales, Rs, ts, cameras, str(res), truncate=True).sum() > 100
    seen = []
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_int, C.c_double)
    cb = CB(lambda ctx, name, phase, ms: seen.append((name.decode(), phase)))
    assert L.lib().mvs_set_trace(C.cast(cb, C.c_void_p), None) == 0
    try:
        V, F = P.PoissonFiles(str(res / "PSR.npts"), str(res / "Model.obj"))
    finally:
        assert L.lib().mvs_set_trace(None, None) == 0
    assert ("mvs_processor_poisson", 0) in seen and ("mvs_processor_poisson", 1) in seen
    lines = (res / "Model.obj").read_text().split("\n")
    assert V > 100 and F > 100
    assert sum(q.startswith("v ") for q in lines) == V == sum(q.startswith("vn ") for q in lines) and sum(q.startswith("f ") for q in lines) == F
    Vc, Fc = P.CullPoissonModel(str(res / "Model.obj"), scales, Rs, ts, cameras, str(res / "Model_cull.obj"))
    print(f"chain: Model.obj V {V} F {F}; culled V {Vc} F {Fc}")
    assert 0 < Vc <= V and 0 < Fc <= F
