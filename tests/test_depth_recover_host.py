"""Host side of mvs_recover_depth_maps (include/mvs.h): symbols, the layout of mvs_depth_recover_params, the argument checks (they run
before a device is needed), the file entries' errors, properties of the numpy restatement tests/ref_depth_recover.py, the conditions the
scenes of tests/depth_recover_scenes.py must meet for the GPU comparison to be exact, the agreement of the restatement with the one of the
refinement driven as a full sweep, what the sweep achieves on scenes A33 and B33, and the shared rules header
(csrc/depth_recover_rules.h) as a stand-alone program under the address and undefined-behaviour sanitizers — on its own cases and on scene
B33, against the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from multiviewstitch_amd import _lib as L, processor as P, scene as S
from tests import depth_recover_scenes as SC, ref_depth_recover as R, ref_depth_refine as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE, E_IO = -1, -4, -10


def _cam(w=16, h=12, fx=20.0, fy=20.0):
    return S.Camera(fx, fy, w / 2 - 0.5, h / 2 - 0.5, np.eye(3), np.zeros(3), w, h)


def _call(cams=None, off=None, n_seq=1, cam_off=True, cam_ptr=True, imgs=True, prm=True, out=True, fn="mvs_recover_depth_maps", **fields):
    cams = [_cam(), _cam()] if cams is None else cams
    off = np.asarray([0, len(cams)] if off is None else off, np.int32)
    arr = (L.CCamera * max(1, len(cams)))(*[L.CCamera.of(c) for c in cams])
    px = max(1, sum(min(c.w, 64) * min(c.h, 64) for c in cams if c.w > 0 and c.h > 0))
    o, im = np.zeros(px, np.float32), np.zeros(3 * px, np.uint8)
    p = P.depth_recover_params(**fields)
    args = (n_seq, L.ptr(off) if cam_off else None, arr if cam_ptr else None, L.ptr(im) if imgs else None, C.byref(p) if prm else None,
            L.ptr(o) if out else None, None, None, None)
    return getattr(L.lib(), fn)(*args, *((None,) if fn.endswith("_dev") else ()))


def test_symbols_and_params_layout():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("mvs_depth_recover_default_params", "mvs_recover_depth_maps", "mvs_recover_depth_maps_dev", "mvs_processor_recover_depths",
                 "mvs_processor_recover_depths_files"):
        assert hasattr(lib, name) and name in L.EXPORTS
    T = L.CDepthRecoverParams
    assert C.sizeof(T) == 56
    assert [getattr(T, k).offset for k, _ in T._fields_] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]
    assert [k for k, _ in T._fields_] == ["dsp_min", "dsp_max", "ssd_err", "peak", "ssd_win", "ref_frm_count", "levels", "min_refs", "flags", "reserved"]
    p = P.depth_recover_params()
    assert (p.dsp_min, p.dsp_max, p.ssd_err, p.peak) == (0.0025, 0.3, 40.0, 0.9)
    assert (p.ssd_win, p.ref_frm_count, p.levels, p.min_refs, p.flags, p.reserved) == (7, 5, 128, 2, L.RECOVER_SUBSTEP, 0)
    assert L.RECOVER_SUBSTEP == R.SUBSTEP == 1
    assert {k: getattr(p, k) for k, _ in T._fields_} == R.params()
    assert lib.mvs_abi_version() == 4
    with pytest.raises(L.MvsError):
        P.depth_recover_params(steps=3)


BAD = [dict(cam_off=False), dict(cam_ptr=False), dict(imgs=False), dict(prm=False), dict(out=False),
       dict(n_seq=0), dict(off=[1, 2]), dict(off=[0, 2, 1], n_seq=2), dict(cams=[_cam(w=0)]), dict(cams=[_cam(h=-3)]), dict(cams=[_cam(fx=0.0)]),
       dict(cams=[_cam(fy=0.0)]), dict(cams=[_cam(), _cam(w=18)]), dict(cams=[_cam(), _cam(h=10)]), dict(cams=[_cam(w=65536, h=32768)]),
       dict(dsp_min=math.nan), dict(dsp_max=math.inf), dict(ssd_err=math.inf), dict(ssd_err=math.nan), dict(peak=math.nan), dict(peak=math.inf),
       dict(dsp_min=0.0), dict(dsp_min=-0.1), dict(dsp_min=0.4), dict(dsp_min=0.3), dict(ssd_err=-1e-9),
       dict(peak=0.0), dict(peak=-0.5), dict(peak=1.0000001),
       dict(ssd_win=-1), dict(ssd_win=16), dict(ref_frm_count=0), dict(ref_frm_count=-1), dict(ref_frm_count=4), dict(ref_frm_count=11),
       dict(ref_frm_count=10), dict(levels=1), dict(levels=0), dict(levels=-5), dict(levels=1025), dict(min_refs=0), dict(min_refs=-1), dict(min_refs=9),
       dict(flags=2), dict(flags=3), dict(flags=-1), dict(reserved=1), dict(reserved=-1)]


def _id(kw):
    return ",".join(f"{k}={[(c.w, c.h, c.fx, c.fy) for c in v] if k == 'cams' else v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", BAD, ids=[_id(kw) for kw in BAD])
def test_argument_errors_need_no_device(kw):
    assert _call(**kw) == E_INVALID
    assert b"mvs_recover_depth_maps:" in L.lib().mvs_last_error()
    assert _call(fn="mvs_recover_depth_maps_dev", **kw) == E_INVALID
    assert b"mvs_recover_depth_maps_dev:" in L.lib().mvs_last_error()


def test_a_valid_call_gets_past_the_checks():
    assert _call() in (0, E_NO_DEVICE)
    assert _call(fn="mvs_recover_depth_maps_dev") in (0, E_NO_DEVICE)
    assert _call(cams=[_cam(), _cam(w=18), _cam(w=18)], off=[0, 1, 1, 3], n_seq=3) in (0, E_NO_DEVICE)      # sizes differ between sequences; one is empty
    assert _call(ssd_win=15, ref_frm_count=9, levels=1024, min_refs=8, peak=1.0, ssd_err=0.0, flags=0) in (0, E_NO_DEVICE)
    assert _call(ssd_win=0, ref_frm_count=1, levels=2, min_refs=1, peak=1e-300, dsp_min=0.29999) in (0, E_NO_DEVICE)


def test_the_file_entries_report_their_errors_before_they_write(tmp_path):
    cams = [[_cam(), _cam()]]
    imgs = [np.zeros((2, 12, 16, 3), np.uint8)]
    d = tmp_path / "seq0"
    d.mkdir()
    with pytest.raises(L.MvsError) as e:
        P.RecoverDepthFiles([str(d)], cams, imgs, P.depth_recover_params(levels=1))
    assert e.value.code == E_INVALID and "mvs_processor_recover_depths" in str(e.value) and not (d / "DATA").exists()
    with pytest.raises(L.MvsError):
        P.RecoverDepthFiles([str(d)], cams, [imgs[0][:, :, :8]])                         # an image stack of the wrong size never reaches the library
    with pytest.raises(L.MvsError):
        P.RecoverDepthFiles([str(d), str(d)], cams, imgs)
    with pytest.raises(L.MvsError) as e:                                                 # no frame files: reported with the path, nothing written
        P.RecoverDepthFilesFromJpeg([str(d)], cams)
    assert e.value.code == E_IO and "00000.jpg" in str(e.value) and not (d / "DATA").exists()
    lib = L.lib()
    off, arr = L.seq_cams(cams)
    dirs = (C.c_char_p * 1)(os.fsencode(str(d)))
    assert lib.mvs_processor_recover_depths(1, dirs, L.ptr(off), arr, None, None) == E_INVALID
    assert lib.mvs_processor_recover_depths(1, None, L.ptr(off), arr, L.ptr(imgs[0]), None) == E_INVALID
    assert lib.mvs_processor_recover_depths(0, dirs, L.ptr(off), arr, L.ptr(imgs[0]), None) == E_INVALID
    assert lib.mvs_processor_recover_depths_files(1, None, L.ptr(off), arr, None) == E_INVALID
    assert lib.mvs_processor_recover_depths(1, dirs, L.ptr(off), arr, L.ptr(imgs[0]), None) in (0, E_NO_DEVICE)      # NULL params: the defaults
    assert not (d / "DATA").exists() or L.device_count() > 0


# ------------------------------------------------------------------ the restatement ----
def test_levels_and_value():
    p = R.params()
    ds, step = R.level_values(p)
    assert len(ds) == 128 and ds[0] == 0.0025 and ds[-1] == 0.3 and step == (0.3 - 0.0025) / 127.0 and all(a < b for a, b in zip(ds, ds[1:]))
    v = R.value(np.array([0.0025, 0.3, 0.1]), p)
    assert v.dtype == np.float32 and float(v[0]) >= 0.0025 > float(np.float32(0.0025)) and float(v[1]) <= 0.3 < float(np.float32(0.3))
    assert v[0] == np.nextafter(np.float32(0.0025), np.float32(1)) and v[1] == np.nextafter(np.float32(0.3), np.float32(0)) and v[2] == np.float32(0.1)


def test_the_order_of_r6_on_constructed_pixels():
    sums = np.array([[12, 30, 6, 6, 12, 3, 9]], np.int64).T              # l = 0 .. 6
    cnts = np.array([[2, 1, 1, 1, 2, 0, 3]], np.int64).T
    # means 6, 30, 6, 6, 6, -, 3 -> the best is 6, the worst 1
    best, worst, have = R.choose(sums, cnts, 1)
    assert (best.tolist(), worst.tolist(), have.tolist()) == ([6], [1], [True])
    best, worst, _ = R.choose(sums, cnts, 2)                             # eligible: 0, 4, 6 with means 6, 6, 3
    assert (best.tolist(), worst.tolist()) == ([6], [0])                 # the worst is tied between 0 and 4: the lower one
    cnts[6] = 0                                                          # min_refs 1: 6 at 0, 2, 3, 4 -> the lowest
    assert R.choose(sums, cnts, 1)[0].tolist() == [0]
    cnts[0] = 0
    assert R.choose(sums, cnts, 1)[0].tolist() == [2]
    best, worst, have = R.choose(sums, cnts, 3)
    assert not have.any()
    big = np.array([[490000000, 499999999]], np.int64).T                 # products beyond 2^31
    best, worst, _ = R.choose(big, np.array([[8, 7]], np.int64).T, 1)
    assert (best.tolist(), worst.tolist()) == ([0], [1])


@pytest.mark.parametrize("name", SC.NAMES)
def test_outputs_are_consistent(name):
    """accepted pixels are exactly those with level >= 0; every accepted (double)out lies in [dsp_min, dsp_max]; every other pixel is
    +0.0f bit for bit; a candidate reports sum >= 0 exactly when it had an eligible level; the substep changes out alone"""
    _, _, p = SC.scene(name)
    for on, off in zip(SC.reference(name, R.SUBSTEP), SC.reference(name, 0)):
        assert np.array_equal(on["level"], off["level"]) and np.array_equal(on["sum"], off["sum"]) and np.array_equal(on["cnt"], off["cnt"])
        for ref in (on, off):
            acc = ref["level"] >= 0
            wide = ref["out"].astype(np.float64)
            assert ((wide[acc] >= p["dsp_min"]) & (wide[acc] <= p["dsp_max"])).all() and (ref["level"][acc] < p["levels"]).all()
            assert (ref["out"].view(np.uint32)[~acc] == 0).all() and (ref["level"][~acc] == R.NONE).all()
            assert ((ref["sum"] == -1) == (ref["cnt"] == 0)).all() and (ref["cnt"][acc] >= p["min_refs"]).all()
            for f, fr in enumerate(ref["frames"]):
                assert np.array_equal(fr["accepted"], ref["level"][f][fr["cand"]] >= 0)
                assert (ref["cnt"][f][~fr["cand"]] == 0).all() and (ref["level"][f][~fr["cand"]] == R.NONE).all()


def test_what_rejects_every_pixel():
    for name in ("D", "C_M2"):
        for ref in SC.reference(name):
            assert (ref["level"] == R.NONE).all() and (ref["out"].view(np.uint32) == 0).all() and (ref["sum"] == -1).all() and (ref["cnt"] == 0).all()
    (ref,) = SC.reference("C_M1")
    assert (ref["level"] >= 0).sum() > 300
    # scene E under ref_frm_count = 3: frame 0's only reference is frame 1, and both are of one colour
    (ref,) = SC.reference("E_R3")
    assert (ref["level"][0] == R.NONE).all() and (ref["out"][0].view(np.uint32) == 0).all()
    assert (ref["cnt"][0] > 0).sum() > 500 and (ref["sum"][0][ref["cnt"][0] > 0] == 0).all()
    assert (ref["level"][3] >= 0).sum() > 300                             # frames 2 and 4 are textured
    cameras, imgs, p = SC.scene("A33")                                    # an image set of one colour rejects every pixel
    (ref,) = R.recover(cameras, [np.full_like(imgs[0], 77)], p)
    assert (ref["level"] == R.NONE).all() and (ref["sum"][ref["cnt"] > 0] == 0).all() and (ref["cnt"] > 0).sum() > 3000


@pytest.mark.parametrize("name", ("A33", "A1024", "B33", "C_M1", "E_R9", "E_N0", "W15"))
def test_the_substep_stays_inside_half_a_level(name):
    _, _, p = SC.scene(name)
    step = (p["dsp_max"] - p["dsp_min"]) / (p["levels"] - 1)
    moved = 0
    for on, off in zip(SC.reference(name, R.SUBSTEP), SC.reference(name, 0)):
        for f, fr in enumerate(on["frames"]):
            # R8 never leaves [l* - 0.5, l* + 0.5]: c0 is the smallest of the three, so |c- - c+| <= (c- - c0) + (c+ - c0) = den.  In fp64
            # the bound holds to 1e-6: the means are quotients of integers below 5e8 over counts of at most 8, so two different means
            # lie at least 1 / 56 apart, and the rounding of c- - 2 c0 moves a den of 1 / 56 by less than 4e-7 of itself
            assert (np.abs(fr["offset"]) <= 0.5 + 1e-6).all(), float(np.abs(fr["offset"]).max())
            acc = on["level"][f] >= 0
            lv = on["level"][f][acc].astype(np.float64)
            pos = (on["out"][f][acc].astype(np.float64) - p["dsp_min"]) / step
            assert (np.abs(pos - lv) <= 0.5 + 1e-6 + 1e-6 / step).all()                                  # 1e-6 / step: the float32 of out
            moved += int((on["out"][f] != off["out"][f]).sum())
    assert moved > 50


@pytest.mark.parametrize("name", SC.NAMES)
def test_scene_conditions(name):
    """every decision an fp64 operation feeds clears its margin, so that a last-bit difference cannot move it; and the scenes hold what
    they are there for"""
    cameras, imgs, p = SC.scene(name)
    for k, ref in enumerate(SC.reference(name)):
        mg = ref["margins"]
        print(name, k, {kind: f"{v:.2e}" for kind, v in mg.items()})
        accepted = int((ref["level"] >= 0).sum())
        if accepted:
            assert set(mg) >= {"coord", "z", "accept", "peak", "nudge"}
        assert mg.get("coord", 1.0) >= SC.MARGIN and mg.get("z", 1.0) >= SC.MARGIN
        assert mg.get("accept", 1.0) >= SC.MARGIN and mg.get("peak", 1.0) >= SC.MARGIN
        assert mg.get("range", 1.0) >= SC.RANGE_MARGIN and mg.get("nudge", 1.0) >= SC.RANGE_MARGIN
        seen = {key: sum(fr["seen"][key] for fr in ref["frames"]) for key in ("behind", "outside")}
        rejected = int(((ref["level"] < 0) & (ref["cnt"] > 0)).sum())
        no_l = int(sum((fr["cand"] & (ref["cnt"][f] == 0)).sum() for f, fr in enumerate(ref["frames"])))
        print(name, k, seen, "accepted", accepted, "rejected", rejected, "candidates without an eligible level", no_l)
        if name in ("A33", "A1024", "B33", "C_M1", "AC", "E_N0"):
            assert accepted > 300 and rejected > 30 and seen["outside"] > 50
        if name == "A2":
            assert rejected > 1000
        if name == "B33":
            assert seen["behind"] > 1000 and no_l > 0 and len({int(c) for c in np.unique(ref["cnt"])}) >= 3       # 0, 2 and 3 references
        if name == "A33":
            w, h = cameras[k][0].w, cameras[k][0].h
            assert w % 16 and h % 16 and w > 32 and h > 16                                                 # several tiles, none of them whole
        if name == "A1024":
            same = sum(int(((fr["sums"][1:] == fr["sums"][:-1]) & (fr["cnts"][1:] == fr["cnts"][:-1]) & (fr["cnts"][1:] > 0)).sum()) for fr in ref["frames"])
            assert same > 100000                                                                           # consecutive levels share their landing pixels
        if name == "W15":
            assert int(ref["frames"][0]["cand"].sum()) == 60 and accepted > 100


# ------------------------------------------------------------------ the two restatements ----
def test_the_sweep_agrees_with_the_refinement_driven_as_a_full_sweep():
    """ref_depth_recover at L = 2 K + 1 over [mn, mx] against ref_depth_refine.refine on a constant raster (mn + mx) / 2 with rel_range =
    (mx - mn) / (mx + mn), steps = K, no substep — scene A, K = 16.  With mn = 0.125 and mx = 0.375 the two level sets are the same
    doubles: 0.125 + l / 128 and 0.25 * (1 + k / 32).  min_refs is 1 (the refinement's eligibility is cnt > 0) and peak is 1, which
    leaves m < m_W as the only difference of the acceptance.  R6 breaks a tie towards the lower level, the refinement towards the smaller
    |k|: where the winning mean is reached by more than one level the two may differ, and those pixels are counted and set aside."""
    K = 16
    (cams,), (imgs,), p = SC.scene("A33")
    p = dict(p, levels=2 * K + 1, min_refs=1, peak=1.0, flags=0)
    (rec,) = R.recover([cams], [imgs], p, SC.reference("A33"))
    mn, mx = p["dsp_min"], p["dsp_max"]
    q = RR.params(dsp_min=mn, dsp_max=mx, rel_range=(mx - mn) / (mx + mn), ssd_err=p["ssd_err"], ssd_win=p["ssd_win"], ref_frm_count=5, steps=K, flags=0)
    flat = np.full(imgs.shape[:3], (mn + mx) / 2, np.float32)
    (fin,) = RR.refine([cams], [imgs], [flat], q)
    covered = tied = 0
    for f, (a, b) in enumerate(zip(rec["frames"], fin["frames"])):
        assert np.array_equal(a["at"][0], b["at"][0]) and np.array_equal(a["at"][1], b["at"][1])
        vv, uu = a["at"]
        ds = [RR.hypothesis(np.float64(np.float32((mn + mx) / 2)), k, q["rel_range"] / K) for k in range(-K, K + 1)]
        _, _, _, own_b = R.costs_at(cams, RR.grey(imgs), f, uu, vv, ds, p["ssd_win"], 5, RR.Margins())
        clear = (a["own"] >= SC.MARGIN) & (own_b >= SC.MARGIN)
        assert np.array_equal(a["sums"][:, clear], b["sums"][:, clear]) and np.array_equal(a["cnts"][:, clear], b["cnts"][:, clear])
        idx = np.arange(len(vv))
        s, c = a["sums"], a["cnts"]
        ties = ((s * c[a["best"], idx] == s[a["best"], idx] * c) & (c > 0)).sum(axis=0) > 1
        decided = clear & a["any"] & ~ties
        assert np.array_equal(a["best"][decided], b["best"][decided] + K)
        both = decided & a["accepted"]
        assert (fin["k"][f][vv[both], uu[both]] == a["best"][both] - K).all() and np.array_equal(rec["level"][f][vv[both], uu[both]], a["best"][both])
        covered += int(decided.sum())
        tied += int((clear & a["any"] & ties).sum())
    print("pixels compared:", covered, "; set aside for a tie of the winning mean:", tied)
    assert covered > 3000


# ------------------------------------------------------------------ quality ----
@pytest.mark.parametrize("name", ("A33", "B33"))
def test_the_sweep_recovers_the_truth(name):
    """measured on the restatement alone; tests/depth_recover_scenes.py records the run.  A later edit may fall a tenth below the record"""
    q, want = SC.quality(name), SC.QUALITY[name]
    print(name, q, "recorded", want)
    assert q["accepted"] >= 0.9 * want["accepted"] and q["one_step"] >= 0.9 * want["one_step"] and q["two_pc"] >= 0.9 * want["two_pc"]
    if name == "A33":
        assert q["accepted"] > 3500 and q["one_step"] > 0.9
    else:
        assert q["accepted"] > 1000 and q["two_pc"] > 0.8


def test_the_refinement_lowers_the_error_of_the_plain_sweep():
    """A33 -> ref_depth_refine.refine with rel_range one level step (relative to the median accepted value) and steps 4.  On the plain
    sweep it lowers the rms relative error over the pixels both accept; on the sweep with the substep there is no quantisation left to
    remove and the error stays where it was — both pairs are recorded in depth_recover_scenes.QUALITY"""
    for flags in (0, R.SUBSTEP):
        q, want = SC.refined_quality(flags), SC.QUALITY["A33_refined"][flags]
        print("flags", flags, q, "recorded", want)
        assert q["both"] > 3500
        assert abs(q["rms_recovered"] - want["rms_recovered"]) <= 0.1 * want["rms_recovered"]
        assert q["rms_refined"] <= 1.1 * want["rms_refined"]
    plain = SC.refined_quality(0)
    assert plain["rms_refined"] < plain["rms_recovered"]


# ------------------------------------------------------------------ the shared rules ----
def _build_rules_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "depth_recover_rules")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "multiviewstitch_amd", "csrc"), os.path.join(ROOT, "tests", "depth_recover_rules.cpp"), "-o", exe])
    return exe


def test_the_shared_rules_under_the_sanitizers(tmp_path):
    """tests/depth_recover_rules.cpp: L = 2, the ties of R6, one eligible level, landing pixels one past the interior, the R9 nudge at
    both ends, chosen cost curves, border pixels and a window of one pixel on heap blocks of exact size; then R1-R9 of the header on scene
    B33 (40 x 32, a camera behind the scene) against the restatement, with and without the substep: level, sum and cnt exactly, out bit for
    bit (host code, no contraction)"""
    exe = _build_rules_program(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "depth recover rules ok" in run.stdout, run.stdout + run.stderr
    (cams,), (imgs,), p = SC.scene("B33")
    n, h, w = imgs.shape[:3]
    for flags in (0, R.SUBSTEP):
        (ref,) = SC.reference("B33", flags)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as fh:
            fh.write(np.asarray([n, w, h, p["ssd_win"], p["ref_frm_count"], p["levels"], p["min_refs"], flags], np.int32).tobytes())
            fh.write(np.asarray([p["dsp_min"], p["dsp_max"], p["ssd_err"], p["peak"]], np.float64).tobytes())
            for c in cams:
                fh.write(np.concatenate([[c.fx, c.fy, c.cx, c.cy], np.asarray(c.R, np.float64).reshape(9), np.asarray(c.t, np.float64).reshape(3)]).tobytes())
            fh.write(imgs.tobytes())
        run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        raw = open(fout, "rb").read()
        m = n * h * w
        assert len(raw) == 11 * m
        out = np.frombuffer(raw[:4 * m], np.uint32).reshape(n, h, w)
        sm = np.frombuffer(raw[4 * m:8 * m], np.int32).reshape(n, h, w)
        lv = np.frombuffer(raw[8 * m:10 * m], np.int16).reshape(n, h, w)
        cnt = np.frombuffer(raw[10 * m:], np.uint8).reshape(n, h, w)
        assert np.array_equal(lv, ref["level"]) and np.array_equal(sm, ref["sum"]) and np.array_equal(cnt, ref["cnt"])
        assert np.array_equal(out, ref["out"].view(np.uint32))
