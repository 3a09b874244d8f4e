"""mvs_poisson_reconstruct_band on the GPU (csrc/poisson_band.hip, rules 24-31) against the numpy / scipy restatement
tests/ref_poisson_band.py on the scenes of tests/poisson_band_scenes.py, at solve_tol = 1e-12.  Level by level through the hook: the
active blocks, the node classes and b exactly (integer sums), chi within the accumulated bound of the two chains of solves; then the
mesh — faces exactly (tests/test_poisson_band_entry_host.py checks on the restatement that no inside decision can move), vertices within
B, the open edges exactly, two runs the same bytes —, the dense call where the band is the whole grid, the plain call at or below the
base depth, the three forms, capacities, a solve that cannot converge, non-finite rows and the chain into Model.obj.
Every array whose address goes into a raw call is bound to a name that lives until the call has returned."""
import ctypes as C
import math

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P
from tests import poisson_band_scenes as BS, ref_poisson_band as RB

pytestmark = pytest.mark.gpu
E_INVALID, E_SOLVER = -1, -7


def params(name, **kw):
    return P.poisson_params(**dict(BS.scene(name)[2], solve_tol=BS.TOL, **kw))


def bparams(name):
    return P.poisson_band_params(**BS.scene(name)[3])


def ref_rel(l, lv):
    return lv["rel"] if "rel" in lv else lv["rel_residual"]


def level(name, l):
    """the hook on level l -> (status, info, binfo, active, cls, b, chi)"""
    pts, nrm, _, _ = BS.scene(name)
    prm, bprm = params(name), bparams(name)
    n1, gb = 2 ** l + 1, 2 ** l // 4
    active, cls = np.full(gb ** 3, 7, np.uint8), np.full(n1 ** 3, 7, np.uint8)
    b, chi = np.full(n1 ** 3, -1.0), np.full(n1 ** 3, -1.0)
    hp, hn = L.arr(pts, np.float64), L.arr(nrm, np.float64)
    info, binfo = L.CPoissonInfo(), L.CPoissonBandInfo()
    rc = L.lib().mvs_test_poisson_band_level(len(hp), L.ptr(hp), L.ptr(hn), C.byref(prm), C.byref(bprm), C.byref(info), C.byref(binfo), l,
                                             L.ptr(active), L.ptr(cls), L.ptr(b), L.ptr(chi), n1 ** 3)
    return rc, info, binfo, active.reshape(gb, gb, gb), cls.reshape(n1, n1, n1), b.reshape(n1, n1, n1), chi.reshape(n1, n1, n1)


def raw_call(name, vcap, fcap):
    pts, nrm, _, _ = BS.scene(name)
    prm, bprm = params(name), bparams(name)
    hp, hn = L.arr(pts, np.float64), L.arr(nrm, np.float64)
    v, f = np.full((max(vcap, 1), 3), np.nan), np.full((max(fcap, 1), 3), -1, np.int32)
    info, binfo = L.CPoissonInfo(), L.CPoissonBandInfo()
    rc = L.lib().mvs_poisson_reconstruct_band(len(hp), L.ptr(hp), L.ptr(hn), C.byref(prm), C.byref(bprm), C.byref(info), C.byref(binfo), L.ptr(v), vcap,
                                              L.ptr(f), fcap)
    return rc, info, binfo, v, f


def device_bound(ref, base_rel, band_rel, upto):
    """the accumulated bound with the device's own residuals (the base solve's, then band_rel[l]) and with the restatement's, both
    truncated at level `upto`"""
    cut = dict(ref, levels={l: lv for l, lv in ref["levels"].items() if l <= upto})
    return RB.accumulated_bound(cut, lambda l, lv: base_rel if l == ref["base_depth"] else band_rel[l]), RB.accumulated_bound(cut, ref_rel)


LEVELS = [(name, l) for name in BS.PARITY for l in range(BS.scene(name)[3]["base_depth"] + 1, BS.scene(name)[2]["depth_max"] + 1)]


@pytest.mark.parametrize("name,l", LEVELS, ids=[f"{n}-{l}" for n, l in LEVELS])
def test_a_level_equals_the_restatement(name, l):
    """bnorm, the last assertion, measures the level below as much as the sum: b' = b - A_fc chi_c takes its fixed values from it.  With
    the base solve of `clipped` stopped at the first cycle that met 1e-12 (3.5e-13) bnorm[6] was 1.29e-12 relative from the restatement's,
    whose base stands at 5.4e-15 (2.5e-10 / 1.29e-12 / 3.5e-13 / 3.3e-14 at solve_tol 1e-10 / 1e-12 / 1e-13 / 1e-14); the base solve of
    the band call therefore runs one cycle past its criterion (rule 25)."""
    ref = BS.reference(name)
    assert sorted(ref["levels"]) == [q for n, q in LEVELS if n == name]
    lv = ref["levels"][l]
    rc, info, binfo, active, cls, b, chi = level(name, l)
    assert rc == 0, L.lib().mvs_last_error()
    assert info.depth == ref["depth"] and binfo.base_depth == ref["base_depth"] and info.n_used == ref["n_used"] and info.h == ref["h"]
    assert list(info.origin) == ref["origin"].tolist()
    assert np.array_equal(active, lv["act"].astype(np.uint8))
    assert np.array_equal(cls, lv["cls"])
    free = lv["cls"] == RB.FREE
    assert b[free].tobytes() == lv["b"][free].tobytes()
    assert np.array_equal(np.isnan(chi), np.isnan(lv["chi"])) and np.array_equal(np.isnan(b), np.isnan(lv["b"])) and (b[lv["cls"] == RB.FIXED] == 0.0).all()
    for q in sorted(ref["levels"]):
        assert binfo.n_active_blocks[q] == ref["levels"][q]["n_active"] and binfo.n_free[q] == ref["levels"][q]["n_free"], q
        assert binfo.rel_residual[q] <= BS.TOL, q
    for q in range(11):
        if q not in ref["levels"]:
            assert (binfo.n_active_blocks[q], binfo.n_free[q], binfo.rel_residual[q], binfo.bnorm[q], binfo.iterations[q]) == (0, 0, 0.0, 0.0, 0)
    E_dev, E_ref = device_bound(ref, info.rel_residual, binfo.rel_residual, l)
    has = ~np.isnan(lv["chi"])
    diff = float(np.abs(chi[has] - lv["chi"][has]).max())
    print(f"{name} level {l}: blocks {binfo.n_active_blocks[l]} free {binfo.n_free[l]} iterations {binfo.iterations[l]} rel_residual {binfo.rel_residual[l]:.2e} "
          f"max |chi - chi_ref| {diff:.2e} against {E_dev + E_ref:.2e}; scratch {binfo.scratch_bytes}")
    assert diff <= E_dev + E_ref
    assert info.rel_residual <= BS.TOL and binfo.failed_level == 0
    if l == ref["depth"]:
        print(f"{name}: iso {info.iso!r} against {ref['iso']!r}")
        assert abs(info.iso - ref["iso"]) <= E_dev + E_ref
    for q in sorted(ref["levels"]):                                         # last: see the docstring
        rel = abs(binfo.bnorm[q] - ref["levels"][q]["bnorm"]) / ref["levels"][q]["bnorm"]
        print(f"{name} level {q}: bnorm {binfo.bnorm[q]!r} against {ref['levels'][q]['bnorm']!r}: relative {rel:.2e}")
        assert rel <= 1e-12, q


@pytest.mark.parametrize("name", ("all_active",) + BS.PARITY)
def test_the_mesh_equals_the_restatement_and_two_runs_agree(name):
    pts, nrm, _, _ = BS.scene(name)
    ref = BS.reference(name)
    v, f, info, binfo = P.RunPoissonBand(pts, nrm, params(name), bparams(name))
    assert info["depth"] == ref["depth"] and info["n_vertices"] == len(ref["vertices"]) == len(v) and info["n_faces"] == len(ref["faces"]) == len(f)
    assert f.dtype == np.int32 and np.array_equal(f, ref["faces"])
    assert binfo["n_open_edges"] == ref["n_open_edges"] == (316 if name == "cap" else 0)
    E_dev, E_ref = device_bound(ref, info["rel_residual"], binfo["rel_residual"], ref["depth"])
    E = E_dev + E_ref
    B = math.sqrt(3.0) * ref["h"] * 4.0 * E / (ref["gap"] - 2.0 * E)
    diff = float(np.sqrt(((v - ref["vertices"]) ** 2).sum(1)).max())
    print(f"{name}: V {len(v)} F {len(f)} open {binfo['n_open_edges']} max vertex distance {diff:.2e} ({diff / ref['h']:.2e} h) against B {B:.2e}; "
          f"iterations {binfo['iterations']} scratch {binfo['scratch_bytes']}")
    assert diff <= B
    v2, f2, info2, binfo2 = P.RunPoissonBand(pts, nrm, params(name), bparams(name))
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes() and binfo == binfo2 and info["iso"] == info2["iso"]
    if name == "all_active":                                                # the band is the whole grid: the faces of the dense call
        dv, df, dinfo = P.RunPoisson(pts, nrm, params(name))
        assert dinfo["depth"] == 5 and np.array_equal(f, df)


def test_at_or_below_the_base_depth_the_call_is_the_plain_one():
    pts, nrm, _, _ = BS.scene("at_base")
    v, f, info, binfo = P.RunPoissonBand(pts, nrm, params("at_base"), bparams("at_base"))
    dv, df, dinfo = P.RunPoisson(pts, nrm, params("at_base"))
    assert info["depth"] == dinfo["depth"] == 4 and len(v) > 100
    assert v.tobytes() == dv.tobytes() and f.tobytes() == df.tobytes() and info["iso"] == dinfo["iso"]
    zero = P._poisson_band_info(L.CPoissonBandInfo())
    assert binfo == dict(zero, base_depth=4)


def test_host_device_and_torch_forms_agree():
    import torch
    name = "two_spheres"
    pts, nrm, _, _ = BS.scene(name)
    v, f, info, binfo = P.RunPoissonBand(pts, nrm, params(name), bparams(name))
    tp, tn = torch.from_numpy(np.array(pts)).cuda(), torch.from_numpy(np.array(nrm)).cuda()
    torch.cuda.synchronize()
    dv, df, dinfo, dbinfo = P.RunPoissonBand(tp, tn, params(name), bparams(name))
    assert dv.is_cuda and df.is_cuda and dv.dtype == torch.float64 and df.dtype == torch.int32
    assert dv.cpu().numpy().tobytes() == v.tobytes() and df.cpu().numpy().tobytes() == f.tobytes()
    assert dinfo["iso"] == info["iso"] and dbinfo == binfo
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sp, sn = torch.from_numpy(np.array(pts)).cuda(), torch.from_numpy(np.array(nrm)).cuda()
    assert torch.cuda.current_stream() != st                            # the points are pending on st; the call must order itself there
    for capacity in (None, (3, 5)):                                     # (3, 5): the first attempt is too small and the call is repeated
        sv, sf, _, sb = P.RunPoissonBand(sp, sn, params(name), bparams(name), stream=st.cuda_stream, capacity=capacity)
        assert sv.cpu().numpy().tobytes() == v.tobytes() and sf.cpu().numpy().tobytes() == f.tobytes() and sb == binfo
    # the raw device entry
    cap_v, cap_f = len(v), len(f)
    ov, of = torch.empty((cap_v, 3), dtype=torch.float64, device="cuda"), torch.empty((cap_f, 3), dtype=torch.int32, device="cuda")
    prm, bprm, ci, bi = params(name), bparams(name), L.CPoissonInfo(), L.CPoissonBandInfo()
    L.check(L.lib().mvs_poisson_reconstruct_band_dev(len(pts), L.ptr(tp), L.ptr(tn), C.byref(prm), C.byref(bprm), C.byref(ci), C.byref(bi), L.ptr(ov), cap_v,
                                                     L.ptr(of), cap_f, None))
    assert ov.cpu().numpy().tobytes() == v.tobytes() and of.cpu().numpy().tobytes() == f.tobytes()


def test_capacities_that_are_too_small_report_the_need():
    ref = BS.reference("hemisphere")
    V, F = len(ref["vertices"]), len(ref["faces"])
    for vcap, fcap in ((V - 1, F), (V, F - 1), (0, 0)):
        rc, info, binfo, v, f = raw_call("hemisphere", vcap, fcap)
        assert rc == E_INVALID and b"capacity" in L.lib().mvs_last_error()
        assert (info.n_vertices, info.n_faces) == (V, F) and np.isnan(v).all() and (f == -1).all()          # nothing was written
        assert binfo.n_free[5] == ref["levels"][5]["n_free"]
    rc, info, binfo, v, f = raw_call("hemisphere", V, F)
    assert rc == 0 and np.array_equal(f, ref["faces"]) and not np.isnan(v).any()


def test_a_solve_that_cannot_converge_is_refused():
    """max_cycles = 1 allows 64 iterations, which level 6 of `clipped` (230 000 free nodes) cannot meet at 1e-12"""
    pts, nrm, _, _ = BS.scene("clipped")
    with pytest.raises(L.MvsError) as e:
        P.RunPoissonBand(pts, nrm, params("clipped", max_cycles=1), bparams("clipped"))
    binfo = e.value.band_info
    print(f"clipped, max_cycles 1: failed_level {binfo['failed_level']} rel_residual {binfo['rel_residual'][6]:.2e} iterations {binfo['iterations'][6]}")
    assert e.value.code == E_SOLVER and "residual" in str(e.value)
    assert binfo["failed_level"] == 6 and binfo["iterations"][6] == 64
    assert math.isfinite(binfo["rel_residual"][6]) and binfo["rel_residual"][6] > BS.TOL


def test_non_finite_rows_are_not_used():
    name = "two_levels"
    pts, nrm, _, _ = BS.scene(name)
    v, f, info, binfo = P.RunPoissonBand(pts, nrm, params(name), bparams(name))
    bad_p, bad_n = np.array(pts[:2]), np.array(nrm[:2])
    bad_p[0, 1] = np.nan
    bad_n[1, 2] = np.inf
    p2, n2 = np.concatenate([pts[:100], bad_p, pts[100:]]), np.concatenate([nrm[:100], bad_n, nrm[100:]])
    v2, f2, info2, binfo2 = P.RunPoissonBand(p2, n2, params(name), bparams(name))
    assert info2["n_used"] == info["n_used"] == len(pts) and v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    assert info2["iso"] == info["iso"] and binfo2 == binfo


def test_chain_into_model_obj(tmp_path):
    """PSR.npts -> Model.obj.  The file formats carry six significant digits, so the arrays are those of RunPoissonBand on the points as
    the file holds them, and a `v` line agrees with its vertex to those digits; the `f` lines are exact."""
    name = "hemisphere"
    pts, nrm, _, _ = BS.scene(name)
    src, dst = str(tmp_path / "PSR.npts"), str(tmp_path / "Model.obj")
    IO.write_npts(src, np.array(pts), np.array(nrm))
    fp, fn = IO.read_npts(src)
    v, f, info, binfo = P.RunPoissonBand(fp, fn, params(name), bparams(name))
    V, F = P.PoissonFiles(src, dst, params(name), bparams=bparams(name))
    assert (V, F) == (len(v), len(f)) and V > 1000 and info["depth"] == 5 and binfo["base_depth"] == 3
    lines = open(dst).read().split("\n")
    ov = np.array([[float(x) for x in q.split()[1:4]] for q in lines if q.startswith("v ")])
    of = np.array([[int(x.split("/")[0]) - 1 for x in q.split()[1:4]] for q in lines if q.startswith("f ")], np.int32)
    assert sum(q.startswith("vn ") for q in lines) == V
    assert ov.shape == v.shape and of.shape == f.shape and np.array_equal(of, f)
    err = float((np.abs(ov - v) / np.maximum(np.abs(v), 1e-30)).max())
    print(f"chain: Model.obj V {V} F {F}; max relative |v - v_obj| {err:.2e}")
    assert (np.abs(ov - v) <= 5.1e-6 * np.abs(v)).all()                   # %g: half a unit of the sixth digit
