"""Host side of mvs_point_sample (include/mvs.h): symbols, the layout of mvs_point_sample_params, the argument checks (they run before a
device is needed), properties of the numpy restatement tests/ref_pointsample.py, the conditions the scenes of tests/pointsample_scenes.py
must meet for the GPU comparison to be exact, and the shared rules header (csrc/pointsample_rules.h) as a stand-alone program under the
address and undefined-behaviour sanitizers — on its own cases and on scene B, against the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, io as IO, processor as P, scene as S
from tests import pointsample_scenes as SC, ref_pointsample as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE, E_IO = -1, -4, -10


def _cam(w=16, h=12, fx=20.0, fy=20.0):
    return S.Camera(fx, fy, w / 2 - 0.5, h / 2 - 0.5, np.eye(3), np.zeros(3), w, h)


def _call(cams=None, off=None, n_seq=1, cam_off=True, cam_ptr=True, depths=True, prm=True, soff=True, points=True, normals=True, cap=8, **fields):
    cams = [_cam(), _cam()] if cams is None else cams
    off = np.asarray([0, len(cams)] if off is None else off, np.int32)
    arr = (L.CCamera * max(1, len(cams)))(*[L.CCamera.of(c) for c in cams])
    d = np.zeros(max(1, sum(min(c.w, 64) * min(c.h, 64) for c in cams if c.w > 0 and c.h > 0)), np.float32)
    so, pts, nrm = np.zeros(len(off) + 1, np.int64), np.zeros((8, 3)), np.zeros((8, 3))
    p = P.point_sample_params(**fields)
    return L.lib().mvs_point_sample(n_seq, L.ptr(off) if cam_off else None, arr if cam_ptr else None, L.ptr(d) if depths else None,
                                    C.byref(p) if prm else None, L.ptr(so) if soff else None, L.ptr(pts) if points else None,
                                    L.ptr(nrm) if normals else None, None, None, cap)


def test_symbols_and_params_layout():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_point_sample_default_params", "mvs_point_sample", "mvs_point_sample_dev", "mvs_test_point_sample_candidates",
                 "mvs_processor_point_sample"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T = L.CPointSampleParams
    assert C.sizeof(T) == 56 and T.max_dsp_err.offset == 16 and T.edge_sz_thres.offset == 32 and T.pt_samp_rds.offset == 40 and T.reserved.offset == 52
    p = P.point_sample_params()
    assert (p.dsp_min, p.dsp_max, p.max_dsp_err, p.min_conf, p.edge_sz_thres) == (0.0025, 0.3, 0.01, 0.9, 4.0)
    assert (p.pt_samp_rds, p.nbr_frm_num, p.nbr_frm_step, p.reserved) == (2, 2, 1, 0)
    assert lib.mvs_abi_version() == 4
    with pytest.raises(L.MvsError):
        P.point_sample_params(radius=3)


BAD = [dict(cam_off=False), dict(cam_ptr=False), dict(depths=False), dict(prm=False), dict(soff=False), dict(points=False), dict(normals=False),
       dict(n_seq=0), dict(off=[1, 2]), dict(off=[0, 2, 1], n_seq=2), dict(cams=[_cam(w=0)]), dict(cams=[_cam(h=-3)]), dict(cams=[_cam(fx=0.0)]),
       dict(cams=[_cam(fy=0.0)]), dict(cams=[_cam(), _cam(w=18)]), dict(cams=[_cam(), _cam(h=10)]), dict(cams=[_cam(w=65536, h=32768)]),
       dict(dsp_min=math.nan), dict(dsp_max=math.inf), dict(max_dsp_err=math.nan), dict(min_conf=math.nan), dict(edge_sz_thres=math.inf),
       dict(dsp_min=0.0), dict(dsp_min=-0.1), dict(dsp_min=0.4), dict(max_dsp_err=-1e-9), dict(min_conf=-0.01), dict(min_conf=1.01),
       dict(edge_sz_thres=0.0), dict(edge_sz_thres=-4.0), dict(pt_samp_rds=0), dict(nbr_frm_num=-1), dict(nbr_frm_step=0), dict(cap=-1)]


def _id(kw):
    return ",".join(f"{k}={[(c.w, c.h, c.fx, c.fy) for c in v] if k == 'cams' else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BAD, ids=[_id(kw) for kw in BAD])
def test_argument_errors_need_no_device(kw):
    assert _call(**kw) == E_INVALID
    assert b"mvs_point_sample" in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    assert _call() in (0, E_NO_DEVICE)
    assert _call(cams=[_cam(), _cam(w=18), _cam(w=18)], off=[0, 1, 1, 3], n_seq=3) in (0, E_NO_DEVICE)      # sizes differ between sequences; one is empty
    assert _call(pt_samp_rds=2 ** 31 - 1, nbr_frm_num=2 ** 31 - 1, nbr_frm_step=2 ** 31 - 1, min_conf=0.0, max_dsp_err=0.0, dsp_min=0.3) in (0, E_NO_DEVICE)


def test_the_device_form_and_the_hook_check_their_arguments_too():
    cams = (L.CCamera * 1)(L.CCamera.of(_cam()))
    off, so, p = np.asarray([0, 1], np.int32), np.zeros(2, np.int64), P.point_sample_params(pt_samp_rds=0)
    buf = np.zeros(16 * 12, np.float32)
    assert L.lib().mvs_point_sample_dev(1, L.ptr(off), cams, L.ptr(buf), C.byref(p), L.ptr(so), L.ptr(buf), L.ptr(buf), None, None, 0, None) == E_INVALID
    assert b"mvs_point_sample_dev" in L.lib().mvs_last_error()
    assert L.lib().mvs_test_point_sample_candidates(1, L.ptr(off), cams, L.ptr(buf), C.byref(p), L.ptr(so), L.ptr(buf), 0) == E_INVALID


def test_the_file_entry_reports_a_missing_raster_before_it_writes(tmp_path):
    cams = [[_cam(), _cam()]]
    d = tmp_path / "seq0"
    os.makedirs(d / "DATA" / "CHECK")
    IO.SaveDepth(str(d / "DATA" / "CHECK" / "_depth0.raw"), np.zeros((12, 16)))
    with pytest.raises(L.MvsError) as e:
        P.PointSampleFiles([str(d)], cams)
    assert e.value.code == E_IO and "_depth1.raw" in str(e.value) and not (d / "Rec").exists()
    IO.SaveDepth(str(d / "DATA" / "CHECK" / "_depth1.raw"), np.zeros((12, 16)))       # both rasters there: the parameters are checked next
    with pytest.raises(L.MvsError) as e:
        P.PointSampleFiles([str(d)], cams, P.point_sample_params(min_conf=2.0))
    assert e.value.code == E_INVALID and "mvs_processor_point_sample" in str(e.value) and not (d / "Rec").exists()


@pytest.mark.parametrize("name", SC.NAMES)
def test_properties_of_the_restatement(name):
    cameras, depths, p = SC.scene(name)
    r = p["pt_samp_rds"]
    for cams, dsp, ref in zip(cameras, depths, SC.reference(name)):
        n, h, w = dsp.shape
        cw = -(-w // r)
        key = ref["frame"].astype(np.int64) * (w * h) + ref["pixel"]
        assert len(key) == ref["counts"]["emitted"] > 0 and (np.diff(key) > 0).all()                       # rule 8
        N, Pt = ref["normals"], ref["points"]
        assert np.abs(np.sqrt((N * N).sum(1)) - 1).max() < 1e-14
        centre = np.array([-(np.asarray(c.R).T @ np.asarray(c.t)) for c in cams])[ref["frame"]]
        assert (((Pt - centre) * N).sum(1) < 0).all()                                                      # towards the camera
        cell = (ref["pixel"] // w // r) * cw + ref["pixel"] % w // r
        assert len(np.unique(ref["frame"].astype(np.int64) * ref["cand"].shape[1] + cell)) == len(cell)     # one point per cell at most
        assert (ref["cand"][ref["frame"], cell] == ref["pixel"]).all()                                      # ... and it is the cell's candidate
        emitting = np.zeros(ref["cand"].shape, bool)
        emitting[ref["frame"], cell] = True
        mg = R.Margins()
        for f in range(n):                                                                                 # rule 7, from the result alone
            sel = ref["frame"] == f
            Ps = tuple(Pt[sel, i] for i in range(3))
            for g in range(f + 1, n):
                ok, u, v, _ = R.agrees(Ps, cams[g], dsp[g], p, mg)
                assert not emitting[g, (v[ok] // r) * cw + u[ok] // r].any()


@pytest.mark.parametrize("name", SC.NAMES)
def test_scene_conditions(name):
    """conditions on the inputs: every rule and the coverage have something to reject in A, B and C, rule 4 rejects an in-range coverage
    projection in E, and every decision an fp64 operation feeds clears MARGIN, so that a last-bit difference cannot move it"""
    for k, ref in enumerate(SC.reference(name)):
        c, mg = ref["counts"], ref["margins"]
        print(name, k, c, {kind: f"{v:.2e}" for kind, v in mg.items()})
        if name in ("A", "B", "C"):
            n, h, w = SC.scene(name)[1][k].shape
            assert n * h * w > c["valid"] > c["neighbours"] > c["edge"] > c["confidence"] > c["candidates"] > c["emitted"] > 0 and c["suppressed"] > 0
        if name == "D":
            assert c["confidence"] == c["edge"] and c["suppressed"] == 0 and c["emitted"] == c["candidates"] > 0   # count == 0
        assert set(mg) >= {"edge", "len", "flip"} and (name == "D" or set(mg) >= {"z", "coord", "dsp", "conf"})
        assert min(mg.values()) >= SC.MARGIN


def test_scene_e_rejects_what_lands_on_the_stray_surface():
    """frame 2 of E carries a nearer surface in a rectangle.  The points of frames 0 and 1 that land there (all that pass rules 1-3, taken
    here with rule 5 switched off) do not agree with frame 2 and so could not cover a cell there; with rule 5 on they lose their
    confidence — every frame of E has frame 2 among its neighbours, fewer pixels pass than in A — and none of them is emitted at all"""
    (a,), (e,) = SC.reference("A"), SC.reference("E")
    assert e["counts"]["cover_rejected"] >= 1 and e["counts"]["confidence"] < a["counts"]["confidence"]
    ((cams,), (dsp,), p) = SC.scene("E")
    rows, cols, _ = SC.STRAY
    landed = 0
    for f in (0, 1):
        counts = dict(valid=0, neighbours=0, edge=0, confidence=0)
        keep, Pt, _ = R.frame_rules(cams, dsp, f, dict(p, nbr_frm_num=0), R.Margins(), counts)
        ok, u, v, in_img = R.agrees(tuple(q[keep] for q in Pt), cams[2], dsp[2], p, R.Margins())
        inside = in_img & (v >= rows.start) & (v < rows.stop) & (u >= cols.start) & (u < cols.stop)
        landed += int(inside.sum())
        assert not ok[inside].any()
        sel = e["frame"] == f
        _, u, v, in_img = R.agrees(tuple(e["points"][sel, i] for i in range(3)), cams[2], dsp[2], p, R.Margins())
        assert not (in_img & (v >= rows.start) & (v < rows.stop) & (u >= cols.start) & (u < cols.stop)).any()
    print("pixels of frames 0 and 1 that land on the stray surface:", landed)
    assert landed >= 100


def test_rules_against_plain_loops():
    """scene B (partial cells), a handful of pixels with Python floats: rules 1-3 written out once more, scalar by scalar"""
    (cams,), (dsp,), p = SC.scene("B")
    (ref,) = SC.reference("B")
    f = 1
    c = cams[f]
    Rm, t = np.asarray(c.R, np.float64).reshape(9).tolist(), np.asarray(c.t, np.float64).tolist()

    def point(u, v):
        z = 1.0 / float(dsp[f, v, u])
        q = [(u - c.cx) * z / c.fx - t[0], (v - c.cy) * z / c.fy - t[1], z - t[2]]
        return [(Rm[0] * q[0] + Rm[3] * q[1]) + Rm[6] * q[2], (Rm[1] * q[0] + Rm[4] * q[1]) + Rm[7] * q[2], (Rm[2] * q[0] + Rm[5] * q[1]) + Rm[8] * q[2]]

    sel = np.nonzero(ref["frame"] == f)[0]
    assert len(sel) > 5
    for i in sel[:: max(1, len(sel) // 7)]:
        px = int(ref["pixel"][i])
        u, v = px % c.w, px // c.w
        Pc, Pl, Pr, Pu, Pd = point(u, v), point(u - 1, v), point(u + 1, v), point(u, v - 1), point(u, v + 1)
        assert Pc == ref["points"][i].tolist()
        a, b = [Pr[j] - Pl[j] for j in range(3)], [Pd[j] - Pu[j] for j in range(3)]
        n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        ln = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        n = [x / ln for x in n]
        C0 = [-t[0], -t[1], -t[2]]
        centre = [(Rm[0] * C0[0] + Rm[3] * C0[1]) + Rm[6] * C0[2], (Rm[1] * C0[0] + Rm[4] * C0[1]) + Rm[7] * C0[2], (Rm[2] * C0[0] + Rm[5] * C0[1]) + Rm[8] * C0[2]]
        e = [Pc[j] - centre[j] for j in range(3)]
        if (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2] > 0.0:
            n = [-x for x in n]
        assert n == ref["normals"][i].tolist()


def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "pointsample_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "pointsample_rules.cpp"), "-o", exe])
    return exe


def test_the_shared_rules_under_the_sanitizers(tmp_path):
    """tests/pointsample_rules.cpp: border pixels, a partial last cell, projections that land at u' = w and v' = -1, NaN and zero
    disparities on heap blocks of exact size; then rules 1-6 of the header on scene B (64 x 48, r = 3: partial cells) against the
    restatement: the candidate table exactly, points and normals bit for bit (host code, no contraction)"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "pointsample rules ok" in run.stdout, run.stdout + run.stderr
    (cams,), (dsp,), p = SC.scene("B")
    (ref,) = SC.reference("B")
    n, h, w = dsp.shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.asarray([n, w, h, p["pt_samp_rds"], p["nbr_frm_num"], p["nbr_frm_step"]], np.int32).tobytes())
        fh.write(np.asarray([p["dsp_min"], p["dsp_max"], p["max_dsp_err"], p["min_conf"], p["edge_sz_thres"]], np.float64).tobytes())
        for c in cams:
            fh.write(np.concatenate([[c.fx, c.fy, c.cx, c.cy], np.asarray(c.R, np.float64).reshape(9), np.asarray(c.t, np.float64).reshape(3)]).tobytes())
        fh.write(dsp.tobytes())
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    nc = ref["cand"].size
    cand = np.frombuffer(raw[:4 * nc], np.int32).reshape(ref["cand"].shape)
    assert np.array_equal(cand, ref["cand"])
    rows = np.frombuffer(raw[4 * nc:], np.float64).reshape(-1, 6)
    assert len(rows) == ref["counts"]["candidates"]
    # the emitted points are candidates: find each in the candidate order (frame, cell) and compare its row
    where = {(int(f), int(px)): i for i, (f, px) in enumerate((f, px) for f in range(n) for px in cand[f] if px >= 0)}
    idx = [where[(int(f), int(px))] for f, px in zip(ref["frame"], ref["pixel"])]
    assert np.array_equal(rows[idx, :3], ref["points"]) and np.array_equal(rows[idx, 3:], ref["normals"])
